"""GPU: the input gradient of the dense 1x16 layers on the fused transposed MFMA GEMM (aqlm_hip_gemm_1x16_transposed through
``hip_kernel.code1x16_matmat_transposed``) against fp64 ``gy @ Wq``, Wq being the scaled storage weight restated by the oracle.
Shapes: (40, 192) for g 8 has a last step of 8 output rows, a last column block of 64 and, at 3 slices of its 2 steps, one empty
slice; (40, 208) for g 16 has 13 codes per row, so the dword that holds a code starts on either half, and a last column block of 80;
(96, 256) exact multiples.  Rows 1 (the 16-row tile) and 17 (two MFMA row blocks of a 64-row tile).  The launch's rule for the
tallest tile: more than 64 rows and ceil(rows / 256) x ceil(in / 128) >= 256 blocks.  TALL meets it with the fewest rows that end a
256-row tile on one row: 257 rows = 2 row tiles x 128 column blocks (in = 127 x 128 + the last block of 64 / 80 columns)."""
import gc

import numpy as np
import pytest

from oracle import aqlm_oracle as orc

torch = pytest.importorskip("torch")
from tests.test_hip_parity import check_close  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
SPLITS = [1, 3]
SMALL = {8: (40, 192), 16: (40, 208)}  # g -> (out, in)
TALL = {8: (40, 127 * 128 + 64, 257), 16: (40, 127 * 128 + 80, 257)}  # g -> (out, in, rows)
CASES = [(g, out, fin, rows) for g in (8, 16) for out, fin in (SMALL[g], (96, 256)) for rows in (1, 17)] + [(g,) + TALL[g] for g in (8, 16)]


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else "bfloat16"


def _w64(codes, books, scales, dtype):
    bits = orc.dequantize_weight_storage(codes.numpy().astype(np.int64) % 65536, books.float().numpy(), scales.float().numpy(), _np_dtype(dtype))
    return orc.storage_bits_to_float64(bits, _np_dtype(dtype))


def _integer_case(g, out, fin, rows, dtype, seed):
    """Codebook integers in [-4, 4], scales in {0.5, 1, 2}, gy integers in [-2, 2] with nz = 64 (fp16) / 8 (bf16) non-zeros per row at
    most: a result is a multiple of 0.5 below 16 nz, which the storage type holds exactly.  Row b has them at columns
    (7 b + 11 k + out - 1) mod out: row 0 takes the last output row, and 17 rows reach every step."""
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(-32768, 32768, (out, fin // g, 1), generator=gen).to(torch.int16)
    books = torch.randint(-4, 5, (1, 65536, 1, g), generator=gen).to(dtype)
    scales = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (out,), generator=gen)].reshape(out, 1, 1, 1).to(dtype)
    nz = min(out, 64 if dtype == torch.float16 else 8)
    cols = (7 * torch.arange(rows)[:, None] + 11 * torch.arange(nz)[None, :] + out - 1) % out
    values = torch.randint(1, 3, (rows, nz), generator=gen) * (2 * torch.randint(0, 2, (rows, nz), generator=gen) - 1)
    gy = torch.zeros(rows, out).scatter_(1, cols, values.float()).to(dtype)
    return codes, books, scales, gy


def _random_case(g, out, fin, rows, dtype, seed):
    L = orc.make_layer(seed, fin, out, 1, 16, g, batch=1, bias=False, float_dtype=_np_dtype(dtype))
    gy = torch.randn(rows, out, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return torch.from_numpy(L["codes"]), torch.from_numpy(L["codebooks"]).to(dtype), torch.from_numpy(L["scales"]).to(dtype), gy


def _run(hk, case, splits):
    codes, books, scales, gy = (t.to(DEV) for t in case)
    got = hk.code1x16_matmat_transposed(gy, codes, books, scales, splits=splits)
    assert got is not None and got.dtype == gy.dtype and got.shape == (gy.shape[0], codes.shape[1] * books.shape[3])
    return got


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("g,out,fin,rows", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_integers(hk, g, dtype, out, fin, rows, splits):
    case = _integer_case(g, out, fin, rows, dtype, g + out + rows)
    ref = case[3].double().numpy() @ _w64(*case[:3], dtype)
    assert np.abs(ref).max() > 0 and np.array_equal(torch.from_numpy(ref).to(dtype).double().numpy(), ref), "the reference is not exact in the storage type"
    assert np.array_equal(_run(hk, case, splits).double().cpu().numpy(), ref)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("g,out,fin,rows", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_data_against_the_restated_w(hk, g, dtype, out, fin, rows, splits):
    case = _random_case(g, out, fin, rows, dtype, 1300 + g + out + rows)
    ref = case[3].double().numpy() @ _w64(*case[:3], dtype)
    check_close(_run(hk, case, splits).float().cpu().numpy(), ref, dtype, f"1x16g{g} {fin}->{out} rows={rows} splits={splits}", el_scale=1.0)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("g", [8, 16])
def test_row_independence_and_strided_grad_output(hk, g, splits):
    out, fin = SMALL[g]
    codes, books, scales, gy = _random_case(g, out, fin, 17, torch.float16, 1400 + g)
    full = _run(hk, (codes, books, scales, gy), splits)
    pick = [3, 0, 9]
    assert torch.equal(_run(hk, (codes, books, scales, gy[pick]), splits), full[pick])
    wide = torch.zeros(17, out + 24, dtype=gy.dtype, device=DEV)
    wide[:, 4:4 + out] = gy.to(DEV)
    sliced = wide[:, 4:4 + out]  # (rows neither contiguous nor 16-byte aligned)
    assert not sliced.is_contiguous()
    assert torch.equal(hk.code1x16_matmat_transposed(sliced, codes.to(DEV), books.to(DEV), scales.to(DEV), splits=splits), full)


def _backward_peak(m, x, gy):
    """(x.grad, allocator peak above the level before backward()) of one step; the step before it warms workspaces and the allocator"""
    for _ in range(2):
        x.grad = None
        y = m(x)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y.backward(gy)
        torch.cuda.synchronize()
    return x.grad, torch.cuda.max_memory_allocated() - base


def test_module_route_peak_memory_and_capture(hk, monkeypatch):
    import aqlm
    from aqlm_amd import _native

    fin, fout, rows = 1024, 2048, 16
    gen = torch.Generator().manual_seed(5)
    m = aqlm.QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=True, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        m.codes.copy_(torch.randint(-32768, 32768, m.codes.shape, generator=gen).to(torch.int16))
        m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=gen) * 0.05)
        m.scales.copy_(torch.rand(m.scales.shape, generator=gen) * 0.2 + 0.05)
    x = torch.randn(rows, fin, generator=gen).half().to(DEV).requires_grad_()
    gy = (torch.randn(rows, fout, generator=gen) * 0.1).half().to(DEV)
    monkeypatch.setattr(hk, "FUSED_1X16_TRANSPOSED_ROWS", (1, 1 << 30))
    fused, peak = _backward_peak(m, x, gy)
    workspace = int(_native.lib.aqlm_hip_gemm_1x16_transposed_workspace_bytes(rows, fout, fin, 0))
    assert peak < rows * fin * 2 + workspace + (1 << 20), f"backward() allocated {peak} bytes above its start"
    assert torch.equal(fused, hk.code1x16_matmat_transposed(gy, m.codes, m.codebooks, m.scales))

    graph, sx, sgy = torch.cuda.CUDAGraph(), x.detach().clone().requires_grad_(), gy.clone()
    with torch.cuda.graph(graph):
        m(sx).backward(sgy)
    replays = []
    for _ in range(3):
        sx.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replays.append(sx.grad.clone())
    assert torch.equal(replays[0], fused) and torch.equal(replays[1], fused) and torch.equal(replays[2], fused)

    monkeypatch.setattr(hk, "USE_FUSED_1X16_TRANSPOSED", False)
    plain, peak = _backward_peak(m, x, gy)
    assert peak >= fout * fin * 2
    check_close(fused.float().cpu().numpy(), plain.double().cpu().numpy(), torch.float16, "module route, fused against dequantise + matmul", el_scale=1.0)
