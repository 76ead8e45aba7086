"""Parity against the reference RUNNING: its own Triton gemv on the MI355X vs the HIP operators on the same seeded layers.  Its
outputs are stored under tests/golden/ (oracle/gen_triton_golden.py), so the check does not depend on the reference tree; where
the kernel is staged under oracle/_ref/ (`make -C oracle ref`) and Triton is present, it is run live as well."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_triton_golden.npz")


def _stored_case(K, nbits, g, fin, fout):
    """The seeded layer, the stored Triton output for it (inputs proven identical by their hash) and the fp64 oracle's output."""
    from oracle import aqlm_oracle as orc
    from oracle import gen_triton_golden as G

    L = orc.make_layer(G.SEED, fin, fout, K, nbits, g, batch=1, bias=True)
    name = G.case_name(K, nbits, g, fin, fout)
    with np.load(GOLDEN) as gold:
        assert str(gold[f"{name}/sha256"]) == G.inputs_sha256(L), f"{name}: make_layer no longer builds the recorded inputs"
        y_triton = gold[f"{name}/y_triton32"]
    y64 = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])
    return L, y_triton, y64


def _rel(a, b, ref):
    return float(np.mean(np.abs(a - b)) / np.mean(np.abs(ref)))


def test_loader_finds_nothing_without_the_staged_file(tmp_path, monkeypatch):
    import reference_triton as rt

    monkeypatch.setattr(rt, "REF_FILE", str(tmp_path / "missing.py"))
    assert rt.load_reference() is None
    assert rt.run(quick=True)["available"] is False


def test_stored_reference_triton_outputs_match_the_oracle():
    from oracle import gen_triton_golden as G

    for case in G.CASES:
        _, y_triton, y64 = _stored_case(*case)
        assert y_triton.shape == y64.shape and _rel(y_triton, y64, y64) < 1e-3, case


@pytest.mark.gpu
@pytest.mark.parametrize("K,nbits,g,fin,fout", [(1, 16, 8, 1024, 512), (2, 8, 8, 1024, 512), (8, 8, 32, 2048, 256)])
def test_hip_operator_matches_the_reference_triton_kernel(K, nbits, g, fin, fout):
    import torch

    import reference_triton as rt

    # north star: fp16 output within 1e-3 relative (mean over the outputs, relative to mean |y|)
    L, y_triton, y64 = _stored_case(K, nbits, g, fin, fout)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(L[k]).to(dev) for k in ("x", "codes", "codebooks", "scales", "bias")}
    y_hip = rt._hip_op(K, nbits)(t["x"], t["codes"], t["codebooks"], t["scales"], t["bias"]).float().cpu().numpy()
    assert _rel(y_triton, y64, y64) < 1e-3
    assert _rel(y_hip, y64, y64) < 1e-3
    assert _rel(y_hip, y_triton, y64) < 1e-3
    ref = rt.load_reference()
    if ref is not None:  # the staged kernel itself, on this GPU
        r = rt.parity_case(ref, K, nbits, g, fin, fout)
        assert r["reference_triton_vs_oracle"] < 1e-3, r
        assert r["hip_vs_oracle"] < 1e-3, r
        assert r["hip_vs_reference_triton"] < 1e-3, r
