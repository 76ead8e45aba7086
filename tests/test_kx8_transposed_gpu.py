"""GPU: the input gradient of the dense K x 8 layers on the fused transposed MFMA GEMM (aqlm_hip_gemm_kx8_transposed through
``hip_kernel.codekx8_matmat_transposed``) against fp64 ``gy @ Wq``, Wq being the scaled storage weight of DESIGN.md section 4.7
restated by the oracle.  Shapes: (40, 192) has a last step of 8 output rows and a last column block of 64, (96, 256) exact
multiples; rows 1 (the 16-row tile), 17 (two MFMA row blocks of a 64-row tile) and 129 (three 64-row tiles: with at most 2 column
blocks the launch never takes the 128-row tile).  TALL is the case of the 128-row tile, which the launch takes from 256 blocks of
it on: 32 column blocks (the last of 64 columns) x 8 row tiles, the last of them with one row, out = 40 as above.  3 slices of the
2 steps of out = 40 leave one slice empty."""
import gc

import numpy as np
import pytest

from oracle import aqlm_oracle as orc

torch = pytest.importorskip("torch")
from tests.test_hip_parity import check_close  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCHEMES = [(1, 8), (2, 8), (4, 16), (8, 32)]
SHAPES = [(40, 192), (96, 256)]  # (out, in)
SHAPE_OF = {(1, 8): (40, 192), (2, 8): (96, 256), (4, 16): (40, 192), (8, 32): (96, 256)}
DTYPES = [torch.float16, torch.bfloat16]
ROWS = [1, 17, 129]
TALL = (40, 4032, 7 * 128 + 1)  # (out, in, rows): one row more than 7 tiles of the largest row tile
CASES = [(out, fin, rows) for out, fin in SHAPES for rows in ROWS] + [TALL]
SPLITS = [1, 3]


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else "bfloat16"


def _w64(codes, books, scales, dtype):
    bits = orc.dequantize_weight_storage(codes.numpy().astype(np.int64) % 256, books.float().numpy(), scales.float().numpy(), _np_dtype(dtype))
    return orc.storage_bits_to_float64(bits, _np_dtype(dtype))


def _integer_case(K, g, out, fin, rows, dtype, seed):
    """Codebook integers in [-4, 4], scales in {0.5, 1, 2}, gy integers in [-2, 2] with at most nz non-zeros per row: a result is a
    multiple of 0.5 below 16 K nz, which the storage type holds exactly for K nz <= 64 (fp16, 11 bits) / 8 (bf16, 8 bits).  Row b has
    them at columns (7 b + 11 k + out - 1) mod out: row 0 takes the last output row, and 17 rows reach every step."""
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(-128, 128, (out, fin // g, K), generator=gen).to(torch.int8)
    books = torch.randint(-4, 5, (K, 256, 1, g), generator=gen).to(dtype)
    scales = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (out,), generator=gen)].reshape(out, 1, 1, 1).to(dtype)
    nz = min(out, (64 if dtype == torch.float16 else 8) // K)
    cols = (7 * torch.arange(rows)[:, None] + 11 * torch.arange(nz)[None, :] + out - 1) % out
    values = torch.randint(1, 3, (rows, nz), generator=gen) * (2 * torch.randint(0, 2, (rows, nz), generator=gen) - 1)
    gy = torch.zeros(rows, out).scatter_(1, cols, values.float()).to(dtype)
    return codes, books, scales, gy


def _random_case(K, g, out, fin, rows, dtype, seed):
    L = orc.make_layer(seed, fin, out, K, 8, g, batch=rows, bias=False, float_dtype=_np_dtype(dtype))
    gy = torch.randn(rows, out, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return torch.from_numpy(L["codes"]), torch.from_numpy(L["codebooks"]).to(dtype), torch.from_numpy(L["scales"]).to(dtype), gy


def _run(hk, case, splits):
    codes, books, scales, gy = (t.to(DEV) for t in case)
    got = hk.codekx8_matmat_transposed(gy, codes, books, scales, splits=splits)
    assert got is not None and got.dtype == gy.dtype and got.shape == (gy.shape[0], codes.shape[1] * books.shape[3])
    return got


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("out,fin,rows", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,g", SCHEMES)
def test_exact_on_integers(hk, K, g, dtype, out, fin, rows, splits):
    case = _integer_case(K, g, out, fin, rows, dtype, 10 * K + g + out + rows)
    ref = case[3].double().numpy() @ _w64(*case[:3], dtype)
    assert np.abs(ref).max() > 0 and np.array_equal(torch.from_numpy(ref).to(dtype).double().numpy(), ref), "the reference is not exact in the storage type"
    assert np.array_equal(_run(hk, case, splits).double().cpu().numpy(), ref)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_integers_runtime_k_and_gy_tail(hk, dtype, rows, splits):
    """K = 3 has no fixed-K instance (the kernel reads K at run time, codes byte by byte) and out = 44 is no multiple of 8: the last
    piece of a gy row (columns 40 .. 47) is read element by element.  gy is a view of 48-element rows, so it is neither copied nor
    declined."""
    K, g, out, fin = 3, 8, 44, 192
    codes, books, scales, gy = _integer_case(K, g, out, fin, rows, dtype, 10 * K + g + out + rows)
    assert bool((gy[:, 40:] != 0).any())
    ref = gy.double().numpy() @ _w64(codes, books, scales, dtype)
    assert np.abs(ref).max() > 0 and np.array_equal(torch.from_numpy(ref).to(dtype).double().numpy(), ref), "the reference is not exact in the storage type"
    wide = torch.zeros(rows, 48, dtype=dtype, device=DEV)
    view = wide[:, :out]
    view.copy_(gy)
    assert view.stride(0) == 48 and view.data_ptr() % 16 == 0
    got = hk.codekx8_matmat_transposed(view, codes.to(DEV), books.to(DEV), scales.to(DEV), splits=splits)
    assert got is not None and got.dtype == dtype and got.shape == (rows, fin)
    assert np.array_equal(got.double().cpu().numpy(), ref)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("rows", ROWS + [TALL[2]])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,g", SCHEMES)
def test_random_data_against_the_restated_w(hk, K, g, dtype, rows, splits):
    out, fin = TALL[:2] if rows == TALL[2] else SHAPE_OF[(K, g)]
    case = _random_case(K, g, out, fin, rows, dtype, 1300 + K + g + rows)
    ref = case[3].double().numpy() @ _w64(*case[:3], dtype)
    check_close(_run(hk, case, splits).float().cpu().numpy(), ref, dtype, f"{K}x8g{g} {fin}->{out} rows={rows} splits={splits}", el_scale=1.0)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("K,g", SCHEMES)
def test_row_independence_and_strided_grad_output(hk, K, g, splits):
    out, fin = SHAPE_OF[(K, g)]
    codes, books, scales, gy = _random_case(K, g, out, fin, 17, torch.float16, 1400 + K)
    full = _run(hk, (codes, books, scales, gy), splits)
    pick = [3, 0, 9]
    assert torch.equal(_run(hk, (codes, books, scales, gy[pick]), splits), full[pick])
    wide = torch.zeros(17, out + 24, dtype=gy.dtype, device=DEV)
    wide[:, 8:8 + out] = gy.to(DEV)
    sliced = wide[:, 8:8 + out]
    assert not sliced.is_contiguous()
    assert torch.equal(hk.codekx8_matmat_transposed(sliced, codes.to(DEV), books.to(DEV), scales.to(DEV), splits=splits), full)


def _backward_peak(m, x, gy):
    """(x.grad, allocator peak above the level before backward()) of one step; the step before it warms workspaces and the allocator.
    Garbage of earlier tests is collected first: device memory freed by a collection during backward() would hide its allocations
    under the level it started from."""
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


def test_module_route_and_peak_memory(hk, monkeypatch):
    import aqlm

    fin = fout = 2048
    gen = torch.Generator().manual_seed(5)
    m = aqlm.QuantizedLinear(fin, fout, 8, 1, 2, 8, bias=True, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        m.codes.copy_(torch.randint(-128, 128, m.codes.shape, generator=gen).to(torch.int8))
        m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=gen) * 0.05)
        m.scales.copy_(torch.rand(m.scales.shape, generator=gen) * 0.2 + 0.05)
    x = torch.randn(256, fin, generator=gen).half().to(DEV).requires_grad_()
    gy = (torch.randn(256, fout, generator=gen) * 0.1).half().to(DEV)
    monkeypatch.setattr(hk, "FUSED_KX8_TRANSPOSED_MIN_ROWS", 1)
    grad, peak = _backward_peak(m, x, gy)
    assert torch.equal(grad, hk.codekx8_matmat_transposed(gy, m.codes, m.codebooks, m.scales))
    assert peak < fout * fin * 2 // 2, f"backward() allocated {peak} bytes above its start"
    monkeypatch.setattr(hk, "USE_FUSED_KX8_TRANSPOSED", False)
    grad, peak = _backward_peak(m, x, gy)
    assert torch.equal(grad, torch.matmul(gy, hk.code2x8_dequant(m.codes, m.codebooks, m.scales)))
    assert peak >= fout * fin * 2


@pytest.mark.parametrize("K,g,splits", [(2, 8, 1), (8, 32, 3)])
def test_capture_replays_equal_eager(hk, K, g, splits):
    out, fin = SHAPE_OF[(K, g)]
    codes, books, scales, gy = (t.to(DEV) for t in _random_case(K, g, out, fin, 17, torch.float16, 1500 + K))
    hk.codekx8_matmat_transposed(gy, codes, books, scales, splits=splits)  # (the kernel's attributes are set outside the capture)
    torch.cuda.synchronize()
    graph, static = torch.cuda.CUDAGraph(), gy.clone()
    with torch.cuda.graph(graph):
        captured = hk.codekx8_matmat_transposed(static, codes, books, scales, splits=splits)
    for seed in (1, 2, 3):
        fresh = torch.randn(17, out, generator=torch.Generator().manual_seed(seed)).half().to(DEV)
        static.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, hk.codekx8_matmat_transposed(fresh, codes, books, scales, splits=splits))
