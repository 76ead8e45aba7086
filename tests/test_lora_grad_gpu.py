"""The weight-gradient reduction of the dense LoRA route on the MI355X: the raw ``hip_kernel.lora_grad`` (aqlm_hip_lora_grad, the
row-split MFMA GEMM of aqlm_amd/csrc/lora_grad.hip) against fp64 of its definition, computed from the SAME fp32 ``w`` and storage
``V``:  G[r, i] = scaling * sum over the rows b with ids[b] == adapter of  w[b, :, r].sum() * V[b, i].

Bound, from the arithmetic (exact products of storage-type operands, fp32 sums, w split into hi + lo of the storage type):
    |G - G64| <= |scaling| * ((eps_T + (n + 2) * 2^-24) * sum_b |w| |V|  [+ 2^-25 * sum_b |V| for fp16: lo may be subnormal])
with n the number of matching rows, eps_T = 2^-16 (bf16: two 8-bit roundings) or 2^-22 (fp16).  Magnitudes are O(1), so the
absolute fp16 term is not what passes the test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALINGS = (2.0, 0.5, 1.25, 3.0)
# rows None: the smallest count at which the entry cuts >= 3 slabs with a ragged last one.  ids: "null" (NULL = adapter 0), "mixed"
# (every live adapter, a negative id, an id past the table and the dead entry, row by row) or "gap" (adapters 0 and 1 only, rows
# 32..63 all adapter 1: at 4100 rows a slab is 3 steps, so slab 0 has a step without a match between two with matches, adapter 2 is
# named by no row, and the rows of adapter 1 hold inf in V and NaN in w).  The table always ends with a dead entry (rank 4).
CASES = [
    dict(rows=1, dim=8, ranks=(8,), splits=1, pad=0, ids="null", targets=(0,)),
    dict(rows=33, dim=264, ranks=(8, 24, 128), splits=3, pad=8, ids="mixed", targets=(0, 1, 2)),
    dict(rows=None, dim=520, ranks=(8, 24, 128), splits=1, pad=0, ids="mixed", targets=(0, 1, 2)),
    dict(rows=4100, dim=264, ranks=(8, 24, 128), splits=1, pad=0, ids="gap", targets=(0, 2)),
]


def _ref64(v, w, ids, adapter, rank, scaling):
    """-> (G64, sum_b |w||V|, sum_b |V|, n) over the rows of ``adapter``, rows r >= rank zero."""
    sel = np.nonzero(ids == adapter)[0]
    V = v[sel].double().cpu().numpy()
    W = w[sel].double().cpu().numpy().sum(axis=1)
    W[:, rank:] = 0.0
    s = float(np.float32(scaling))
    return s * (W.T @ V), np.abs(W).T @ np.abs(V), np.abs(V).sum(axis=0)[None, :] * (np.arange(W.shape[1]) < rank)[:, None], len(sel)


def _bound(dtype, scaling, n, sum_wv, sum_v):
    eps = 2.0 ** -22 if dtype == torch.float16 else 2.0 ** -16
    absolute = 2.0 ** -25 * sum_v if dtype == torch.float16 else 0.0
    return abs(scaling) * ((eps + (n + 2) * 2.0 ** -24) * sum_wv + absolute)


@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["one-row", "step+1-strided-3slices", "three-ragged-slabs", "three-step-slabs-gap-poison"])
def test_lora_grad_matches_fp64_of_the_definition(case, dtype, ids_dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dim, ranks, splits = case["dim"], case["ranks"], case["splits"]
    rows = case["rows"] or next(r for r in range(1, 1 << 16) if r % 32 and hk.lora_grad_slabs(r, dim) >= 3)
    max_rank, n_live = max(ranks), len(ranks)
    gen = torch.Generator().manual_seed(rows + dim)
    ads = [(torch.zeros((r, dim), dtype=dtype, device=DEV), torch.zeros((dim, r), dtype=dtype, device=DEV), SCALINGS[i])
           for i, r in enumerate(ranks + (4,))]
    table = hk.lora_table(ads, torch.device(DEV))
    n = len(ads)
    if case["ids"] == "null":
        ids, idt = np.zeros(rows, dtype=np.int64), None
    else:
        pattern = (0, -1, 2, n, 1, n - 1) if case["ids"] == "mixed" else (0, 1, 0, 0)
        ids = np.array([1 if case["ids"] == "gap" and 32 <= b < 64 else pattern[b % len(pattern)] for b in range(rows)], dtype=np.int64)
        idt = torch.from_numpy(ids).to(ids_dtype).to(DEV)
    v = torch.randn((rows, dim + case["pad"]), generator=gen).to(dtype)[:, :dim]
    w = torch.randn((rows, splits, max_rank), generator=gen) / splits
    vd, wd = v.to(DEV), w.to(DEV)
    if case["pad"]:  # a V whose row stride is not its row length
        vd = torch.empty((rows, dim + case["pad"]), dtype=dtype, device=DEV)[:, :dim].copy_(v)
    if case["ids"] == "gap":  # rows of ANOTHER adapter: neither operand may reach G
        other = torch.from_numpy(ids == 1).to(DEV)
        vd[other] = float("inf")
        wd[other] = float("nan")
    assert hk.lora_grad_supported(dim, max_rank, rows)
    plane = max_rank * dim
    for a in case["targets"] + (n - 1,):
        buf = torch.full(((n + 1) * plane,), float("nan"), dtype=torch.float32, device=DEV)  # every entry, then a guard region
        out = buf[a * plane:(a + 1) * plane].view(max_rank, dim)
        got = hk.lora_grad(vd, wd, idt, table, [n, max_rank, dim, a], out=out)
        assert got.data_ptr() == out.data_ptr()
        rest = torch.cat([buf[:a * plane], buf[(a + 1) * plane:]])
        assert torch.isnan(rest).all(), f"adapter {a}: another entry or the guard region was written"
        if a == n - 1:
            assert torch.isnan(out).all(), "the dead entry's output was touched"
            continue
        g64, sum_wv, sum_v, matched = _ref64(v, w, ids, a, ranks[a], SCALINGS[a])
        assert ((sum_wv > 0) | (g64 == 0)).all(), "the bound vanishes where the reference does not"
        g = out.double().cpu().numpy()
        assert np.isfinite(g).all(), f"adapter {a}: non-finite (or unwritten) elements"
        err, bound = np.abs(g - g64), _bound(dtype, SCALINGS[a], matched, sum_wv, sum_v)
        print(f"adapter {a} rank {ranks[a]} rows {rows} ({matched} matching) dim {dim}: worst error / bound "
              f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}, max |G| {np.abs(g64).max():.3g}")
        assert not (err > bound).any(), f"adapter {a}: {(err > bound).sum()} elements outside the bound, worst {err.max():.4g}"
        if case["ids"] == "gap" and a == 2:
            assert matched == 0 and not g.any(), "an adapter no row names must give zeros"
        again = hk.lora_grad(vd, wd, idt, table, [n, max_rank, dim, a])
        assert torch.equal(again, out), f"adapter {a}: two calls differ"
