"""A tiny Mixtral AQLM checkpoint in the published key layout (``model.layers.N.block_sparse_moe.experts.E.w{1,2,3}.{codes,
codebooks,scales}``, router at ``block_sparse_moe.gate.weight``) and its dense twin: every quantized Linear / expert of the twin
holds the dequantised weight of the checkpoint's codes (``gate_up_proj[e] = cat(W1_e, W3_e)``, ``down_proj[e] = W2_e``).  Shared by
tests/test_moe_host.py and tests/test_moe_gpu.py."""
import json

import numpy as np
import torch

from oracle import aqlm_oracle as orc

HID, INTER, LAYERS, HEADS, KV_HEADS, VOCAB, EXPERTS, TOP_K = 64, 128, 2, 4, 2, 128, 4, 2
SCHEME = dict(in_group_size=8, out_group_size=1, num_codebooks=1, nbits_per_codebook=16)


def quantized_weight(seed, in_features, out_features):
    """-> (codes int16, codebooks fp16, scales fp16, dense W fp16) of one random 1x16 g8 layer with tame activations."""
    L = orc.make_layer(seed, in_features, out_features, 1, 16, 8, batch=1, bias=False, edge_codes=False)
    cb = (L["codebooks"].astype(np.float32) * 0.05).astype(np.float16)
    sc = (np.abs(L["scales"].astype(np.float32)) * 0.2 + 0.05).astype(np.float16)
    W = orc.dequantize_weight(L["codes_unsigned"], cb, sc).astype(np.float16)
    return torch.from_numpy(L["codes"]), torch.from_numpy(cb), torch.from_numpy(sc), torch.from_numpy(W)


def config():
    from transformers import MixtralConfig

    return MixtralConfig(hidden_size=HID, intermediate_size=INTER, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         num_key_value_heads=KV_HEADS, vocab_size=VOCAB, max_position_embeddings=64, num_local_experts=EXPERTS,
                         num_experts_per_tok=TOP_K, tie_word_embeddings=False, router_jitter_noise=0.0)


def build(out_dir):
    """Write the quantized checkpoint to ``out_dir`` (created) and return the dense twin (fp16, cpu)."""
    from safetensors.torch import save_file
    from transformers import MixtralForCausalLM

    torch.manual_seed(0)
    cfg = config()
    dense = MixtralForCausalLM(cfg).to(torch.float16)
    qstate, covered = {}, set()
    seed = 300
    for name, mod in dense.named_modules():
        if isinstance(mod, torch.nn.Linear) and "lm_head" not in name:
            seed += 1
            codes, cb, sc, W = quantized_weight(seed, mod.in_features, mod.out_features)
            with torch.no_grad():
                mod.weight.copy_(W)
            qstate.update({f"{name}.codes": codes, f"{name}.codebooks": cb, f"{name}.scales": sc})
            covered.add(f"{name}.weight")
    for li, layer in enumerate(dense.model.layers):
        ex = layer.mlp.experts
        pub = f"model.layers.{li}.block_sparse_moe"
        for e in range(EXPERTS):
            ws = {}
            for w, (fin, fout) in (("w1", (HID, INTER)), ("w3", (HID, INTER)), ("w2", (INTER, HID))):
                seed += 1
                codes, cb, sc, ws[w] = quantized_weight(seed, fin, fout)
                qstate.update({f"{pub}.experts.{e}.{w}.codes": codes, f"{pub}.experts.{e}.{w}.codebooks": cb,
                               f"{pub}.experts.{e}.{w}.scales": sc})
            with torch.no_grad():
                ex.gate_up_proj[e].copy_(torch.cat([ws["w1"], ws["w3"]], 0))
                ex.down_proj[e].copy_(ws["w2"])
        covered |= {f"model.layers.{li}.mlp.experts.gate_up_proj", f"model.layers.{li}.mlp.experts.down_proj"}
        qstate[f"{pub}.gate.weight"] = layer.mlp.gate.weight.detach().clone()
        covered.add(f"model.layers.{li}.mlp.gate.weight")
    for k, v in dense.state_dict().items():
        if k not in covered:
            qstate[k] = v.contiguous()
    out_dir.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in qstate.items()}, str(out_dir / "model.safetensors"), metadata={"format": "pt"})
    c = cfg.to_dict()
    c["architectures"] = ["MixtralForCausalLM"]
    c["torch_dtype"] = "float16"
    c["quantization_config"] = dict(quant_method="aqlm", linear_weights_not_to_quantize=["lm_head"], **SCHEME)
    (out_dir / "config.json").write_text(json.dumps(c))
    return dense


def load(path, device, hook=True):
    """-> (model, loading_info) through aqlm_amd.moe.from_pretrained (hook) or plain AutoModelForCausalLM.from_pretrained."""
    from transformers import AutoModelForCausalLM

    from aqlm_amd import moe

    kw = dict(dtype=torch.float16, device_map=device, output_loading_info=True)
    return moe.from_pretrained(path, **kw) if hook else AutoModelForCausalLM.from_pretrained(path, **kw)
