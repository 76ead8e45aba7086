"""The expert-grouped MoE entries without a GPU: argument checks, the size / support queries, the ISA of the new kernels, and
gradients through the quantized experts on the host (the per-expert loop, tiny checkpoint of tests/moe_checkpoint.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.test_isa_invariants import FLAGS, dma_loops_with_full_drains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_grouped_entries_reject_bad_arguments_without_a_gpu():
    from aqlm_amd import _native as nat

    L = nat.lib
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    bucket = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("ids", p), ("i64", 1), ("pairs", 80), ("E", 8), ("tp", 16), ("bucket", p), ("stream", None))]
    assert L.aqlm_hip_moe_bucket(*bucket(ids=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert L.aqlm_hip_moe_bucket(*bucket(bucket=p + 4)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert L.aqlm_hip_moe_bucket(*bucket(ids=p + 4)) == nat.E_INVALID
    assert L.aqlm_hip_moe_bucket(*bucket(pairs=0)) == nat.E_INVALID
    assert L.aqlm_hip_moe_bucket(*bucket(pairs=nat.MAX_GROUPED_PAIRS + 1)) == nat.E_INVALID
    assert L.aqlm_hip_moe_bucket(*bucket(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_INVALID
    assert L.aqlm_hip_moe_bucket(*bucket(tp=24)) == nat.E_INVALID

    gemm = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("E", 8), ("S", 2), ("bucket", p), ("tp", 16), ("pairs", 80), ("k", 2), ("x", p), ("xs", 4096),
        ("per_pair", 0), ("y", p), ("out", 14336), ("inf", 4096), ("g", 8), ("dt", nat.F16), ("stream", None))]
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(table=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(bucket=None)) == nat.E_INVALID
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(table=p + 4)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(bucket=p + 8)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_INVALID
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(S=3)) == nat.E_INVALID
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(pairs=81)) == nat.E_INVALID  # not a multiple of top_k
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(pairs=nat.MAX_GROUPED_PAIRS + 2)) == nat.E_INVALID
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(tp=8)) == nat.E_INVALID
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(inf=4100)) == nat.E_INVALID  # not a multiple of the group
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(dt=7)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(g=4, inf=4096)) == nat.E_UNSUPPORTED and "8 or 16" in nat.last_error()
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(out=14344)) == nat.E_UNSUPPORTED  # out_features % 16
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(inf=4104)) == nat.E_UNSUPPORTED  # in_features % 64
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(inf=512, xs=512)) == nat.E_UNSUPPORTED  # too short for the kernel's rings
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(x=p + 8)) == nat.E_UNSUPPORTED  # x not 16-byte aligned
    assert L.aqlm_hip_gemm_1x16_grouped(*gemm(xs=4100)) == nat.E_UNSUPPORTED


def test_size_and_support_queries():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    L = nat.lib
    for P, E, tp in ((1, 8, 16), (80, 8, 16), (1024, 8, 128), (600, 256, 16), (5, 8, 64), (nat.MAX_GROUPED_PAIRS, 8, 16)):
        tiles = -(-P // tp) + min(E, P)
        n = L.aqlm_hip_moe_bucket_bytes(P, E, tp)
        assert n % 16 == 0 and n >= 4 * (4 + 4 * tiles + P) and n < 4 * (4 + 4 * tiles + P) + 16, (P, E, tp, n)
    for bad in ((0, 8, 16), (80, 0, 16), (80, 257, 16), (80, 8, 48), (nat.MAX_GROUPED_PAIRS + 1, 8, 16)):
        assert L.aqlm_hip_moe_bucket_bytes(*bad) == 0, bad
    for M, K, g in ((14336, 4096, 8), (4096, 14336, 8), (14336, 4096, 16), (4096, 14336, 16), (2048, 1024, 8), (1024, 2048, 16)):
        assert hk.grouped_supported(M, K, g), (M, K, g)
    for M, K, g in ((14344, 4096, 8), (4096, 4104, 8), (4096, 4096, 4), (4096, 512, 8), (128, 64, 8), (0, 4096, 8)):
        assert not hk.grouped_supported(M, K, g), (M, K, g)
    # tiles: the mean pairs per expert rounded up to a power of two in 16 .. 128, from the sizes alone
    assert [hk.grouped_tile_pairs(P, 8) for P in (1, 66, 128, 129, 256, 257, 512, 513, 1024, 100000)] == [16, 16, 16, 32, 32, 64, 64, 128,
                                                                                                         128, 128]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_grouped_kernels_isa_no_scratch_and_no_ring_drains(tmp_path):
    out = tmp_path / "moe_grouped.s"
    subprocess.run([HIPCC] + FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "moe_grouped.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(_ZN4aqlm\w+)", text, re.M)
    assert sum("gemm_1x16_grouped_kernel" in n for n in names) == 32 and sum("moe_bucket_kernel" in n for n in names) == 1, names
    for m in re.finditer(r"\.name:\s+(_ZN4aqlm\w+)(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
    code = text.split(".amdgpu_metadata")[0]
    assert not re.search(r"\bscratch_(load|store)", code)
    loops, bad = dma_loops_with_full_drains(text, "gemm_1x16_grouped_kernel")
    assert loops >= 16, f"only {loops} LDS-DMA loops found in the ISA"
    assert not bad, f"vmcnt(0) inside an LDS-DMA loop: {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------------------
# gradients on the host: the per-expert loop is differentiable
# ---------------------------------------------------------------------------------------------------------------------------
transformers = pytest.importorskip("transformers")


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    pytest.importorskip("safetensors.torch")
    from tests import moe_checkpoint as mc

    path = tmp_path_factory.mktemp("moe_grad") / "aqlm_tiny_mixtral"
    dense = mc.build(path)
    return dense, str(path)


def _moe64(gate_up, down, x, ids, w):
    """fp64 autograd reference of the experts block: out[t] = sum_j w[t, j] W2_e (silu(W1_e x_t) * W3_e x_t), e = ids[t, j]"""
    out = torch.zeros_like(x)
    inter = down.shape[2]
    for e in range(gate_up.shape[0]):
        tok, pos = torch.where(ids == e)
        if tok.numel() == 0:
            continue
        gu = x[tok] @ gate_up[e].T
        h = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        out = out.index_add(0, tok, (h @ down[e].T) * w[tok, pos, None])
    return out


def _rel(a, b):
    return ((a.double() - b.double()).abs().mean() / b.double().abs().mean()).item()


def test_host_gradients_through_the_loop_match_a_dense_fp64_twin(checkpoint):
    from tests import moe_checkpoint as mc

    dense, path = checkpoint
    model, _ = mc.load(path, "cpu")
    experts = model.model.layers[0].mlp.experts
    twin = dense.model.layers[0].mlp.experts
    gate_up, down = twin.gate_up_proj.detach().double(), twin.down_proj.detach().double()
    gen = torch.Generator().manual_seed(3)
    for T, ids in ((3, None), (9, None), (40, None), (5, torch.tensor([[0, 1], [1, 0], [3, 2], [2, 0], [3, mc.EXPERTS]]))):
        if ids is None:
            ids = torch.topk(torch.rand((T, mc.EXPERTS), generator=gen), mc.TOP_K, dim=-1).indices
        x0 = (torch.randn((T, mc.HID), generator=gen) * 0.5).half()
        w0 = torch.rand((T, mc.TOP_K), generator=gen)
        r = torch.randn((T, mc.HID), generator=gen)
        x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
        (experts(x, ids, w).float() * r).sum().backward()
        x64, w64 = x0.double().requires_grad_(), w0.double().requires_grad_()
        (_moe64(gate_up, down, x64, ids, w64) * r.double()).sum().backward()
        assert x.grad is not None and w.grad is not None, T
        assert _rel(x.grad, x64.grad) <= 5e-3, (T, "x.grad", _rel(x.grad, x64.grad))
        assert _rel(w.grad, w64.grad) <= 5e-3, (T, "top_k_weights.grad", _rel(w.grad, w64.grad))
        assert all(p.grad is None for p in experts.parameters())
