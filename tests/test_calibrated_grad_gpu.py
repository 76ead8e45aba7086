"""The calibrated-training entries (aqlm_hip_calib_delta / _rows / _codebook_grad_1x16 / _codebook_grad_kx8) and
``aqlm.tuning.calibrated_loss_and_grads`` / ``quantize_layer_`` on the MI355X.

Shapes: out = 48 for 1x16 and 80 for K x 8 (8x8 g32 has 4 codebook passes, so 64 row blocks of 1 or 2 rows), in = 70 g (one full pass of
a wave's 64 lanes and a tail of 6).  The 1x16 codes use one entry 600 times (three chunks of the inverted index: the finish launch adds
them), a few entries once and leave most unused; they include the wrap-around values -1 and -32768.  ``XTX = X^T X / n`` of a seeded X of
2 in rows.  The inputs of a scheme and their fp64 autograd are computed once.

Held bit for bit: delta against torch's fp32 ``_dequantize_weight(...) - W_ref``; rows and both codebook gradients against
tests/calib_grad_model.py on the same G.  The whole step is held to fp64 autograd of the definition with the fp32 torch route's own
error as the yardstick: per output tensor the kernel route's relative infinity-norm error may be at most twice the torch route's (the
margin covers a different but equally long summation order)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import calib_grad_model as model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SCHEMES = {"1x16g8": (1, 16, 8), "1x16g16": (1, 16, 16), "1x8g8": (1, 8, 8), "2x8g8": (2, 8, 8), "3x8g32": (3, 8, 32), "8x8g32": (8, 8, 32)}
REF_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
HEAVY = 12345  # the 1x16 entry of three chunks


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


@pytest.fixture(scope="module")
def tuning():
    from aqlm_amd import tuning

    return tuning


@functools.lru_cache(maxsize=None)
def case(name):
    """Seeded host tensors of a scheme: stored codes, fp32 codebooks / scales / target, symmetric fp32 XTX."""
    K, nbits, g = SCHEMES[name]
    out, nj = (48 if nbits == 16 else 80), 70
    fin = nj * g
    gen = torch.Generator().manual_seed(1000 + 37 * K + nbits + g)
    if nbits == 16:
        pool = torch.tensor([HEAVY, 65535, 32768, 7, 40000, 65000, 1, 2, 3, 4, 5, 6, 77, 78, 79, 80, 81, 82, 83, 84])  # -1 and -32768 stored
        unsigned = pool[4 + torch.randint(0, 16, (out * nj,), generator=gen)]
        where = torch.randperm(out * nj, generator=gen)
        unsigned[where[:600]] = HEAVY
        unsigned[where[600:603]] = torch.tensor([65535, 32768, 7])  # used once each
        unsigned = unsigned.reshape(out, nj, 1)
        codes = torch.where(unsigned >= 32768, unsigned - 65536, unsigned).to(torch.int16)
    else:
        unsigned = torch.randint(0, 256, (out, nj, K), generator=gen)
        codes = torch.where(unsigned >= 128, unsigned - 256, unsigned).to(torch.int8)
    codebooks = torch.randn((K, 2 ** nbits, 1, g), generator=gen) / K ** 0.5
    scales = (torch.rand((out, 1, 1, 1), generator=gen) + 0.5) * torch.where(torch.rand((out, 1, 1, 1), generator=gen) < 0.2, -1.0, 1.0)
    reference = torch.randn((out, fin), generator=gen)
    x = torch.randn((2 * fin, fin), generator=gen) * (0.5 + torch.rand((1, fin), generator=gen))
    xtx = (x.T @ x) / x.shape[0]
    xtx = 0.5 * (xtx + xtx.T)
    return dict(K=K, nbits=nbits, g=g, out=out, nj=nj, fin=fin, codes=codes, unsigned=unsigned, codebooks=codebooks, scales=scales,
                reference=reference, xtx=xtx)


@functools.lru_cache(maxsize=None)
def on_device(name):
    c = case(name)
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def definition(codes_unsigned, codebooks, scales, reference, xtx):
    """(loss, d_codebooks, d_scales) of the restated ``_compute_mse`` under autograd, in the dtype of the inputs."""
    from aqlm_amd.utils import _dequantize_weight

    books = codebooks.detach().clone().requires_grad_(True)
    factors = scales.detach().clone().requires_grad_(True)
    delta = _dequantize_weight(codes_unsigned, books, factors) - reference
    loss = (delta @ xtx).flatten() @ delta.flatten() / reference.shape[0]
    d_books, d_factors = torch.autograd.grad(loss, (books, factors))
    return loss.detach(), d_books, d_factors


@functools.lru_cache(maxsize=None)
def wide(name):
    """fp64 autograd of the definition on the device."""
    d = on_device(name)
    return definition(d["unsigned"], d["codebooks"].double(), d["scales"].double(), d["reference"].double(), d["xtx"].double())


def padded(t, extra):
    """The same values in a buffer with ``extra`` more elements per row."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def step_inputs(hk, name):
    """(D, G) of the kernel route for a scheme."""
    d = on_device(name)
    delta = hk.calib_delta(d["codes"], d["codebooks"], d["scales"], d["reference"])
    return delta, torch.mm(delta, d["xtx"])


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the entries, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_dtype", REF_DTYPES, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("name", list(SCHEMES))
def test_delta_equals_torch(hk, name, ref_dtype):
    from aqlm_amd.utils import _dequantize_weight

    d = on_device(name)
    reference = d["reference"].to(ref_dtype)
    want = _dequantize_weight(d["unsigned"], d["codebooks"], d["scales"]) - reference.float()
    got = hk.calib_delta(d["codes"], d["codebooks"], d["scales"], reference)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # padded rows of W_ref (an odd element stride) and of D (what lies between the rows stays untouched)
    out = padded(torch.zeros_like(want), 12)
    again = hk.calib_delta(d["codes"], d["codebooks"], d["scales"], padded(reference, 3), out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, want)
    assert torch.isnan(out.as_strided((want.shape[0], 12), (want.shape[1] + 12, 1), want.shape[1])).all()
    assert np.array_equal(model.delta(d["unsigned"].cpu().numpy(), d["codebooks"].cpu().numpy().reshape(d["K"], -1, d["g"]),
                                      d["scales"].cpu().numpy().reshape(-1), reference.float().cpu().numpy()).view(np.int32),
                          bits(got).numpy().reshape(got.shape))


@pytest.mark.parametrize("name", list(SCHEMES))
def test_rows_equal_the_model(hk, name):
    d = on_device(name)
    delta, product = step_inputs(hk, name)
    ds_raw, rowloss = hk.calib_rows(product, delta, d["codes"], d["codebooks"])
    want_ds, want_rl = model.rows(d["unsigned"].cpu().numpy(), d["codebooks"].cpu().numpy().reshape(d["K"], -1, d["g"]),
                                  product.cpu().numpy(), delta.cpu().numpy())
    assert np.array_equal(bits(ds_raw).numpy(), want_ds.view(np.int32))
    assert np.array_equal(bits(rowloss).numpy(), want_rl.view(np.int32))
    # padded rows of G and D
    ds2, rl2 = hk.calib_rows(padded(product, 4), padded(delta, 8), d["codes"], d["codebooks"])
    assert torch.equal(bits(ds2), bits(ds_raw)) and torch.equal(bits(rl2), bits(rowloss))


def codebook_grad(hk, name, product, index=None):
    d = on_device(name)
    if d["nbits"] == 16:
        index = index or hk.build_codebook_grad_index(d["codes"], d["g"])
        return hk.calib_codebook_grad_1x16(product, d["scales"], index)
    return hk.calib_codebook_grad_kx8(product, d["scales"], d["codes"], d["g"])


@pytest.mark.parametrize("name", list(SCHEMES))
def test_codebook_gradient_equals_the_model(hk, name):
    d = on_device(name)
    _, product = step_inputs(hk, name)
    got = codebook_grad(hk, name, product)
    values = d["unsigned"].cpu().numpy()
    if d["nbits"] == 16:
        assert int((values == HEAVY).sum()) == 600 and hk.CODEBOOK_GRAD_CHUNK == 256, "three chunks: the finish launch adds them"
        want = model.dc_1x16(values[:, :, 0], product.cpu().numpy(), d["scales"].cpu().numpy(), d["g"], hk.CODEBOOK_GRAD_CHUNK)
    else:
        want = model.dc_kx8(values, product.cpu().numpy(), d["scales"].cpu().numpy(), d["g"])
    assert np.array_equal(bits(got).numpy().reshape(want.shape), want.view(np.int32))
    again = codebook_grad(hk, name, padded(product, 4))
    assert torch.equal(bits(again), bits(got))


# ---------------------------------------------------------------------------------------------------------------------------
# the whole step against fp64 autograd of the definition
# ---------------------------------------------------------------------------------------------------------------------------
def relative_error(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", list(SCHEMES))
def test_step_is_as_accurate_as_the_fp32_torch_route(tuning, name):
    d = on_device(name)
    want = wide(name)
    args = (d["codes"], d["codebooks"], d["scales"], d["reference"], d["xtx"])
    assert tuning._calibrated_grad_route(*args)
    kernel = tuning.calibrated_loss_and_grads(*args)
    tuning.CALIBRATED_GRAD_KERNEL = False
    try:
        assert not tuning._calibrated_grad_route(*args)
        torch_route = tuning.calibrated_loss_and_grads(*args)
    finally:
        tuning.CALIBRATED_GRAD_KERNEL = True
    assert kernel[0].dim() == 0 and kernel[1].shape == d["codebooks"].shape and kernel[2].shape == d["scales"].shape
    for what, k, t, w in zip(("loss", "d_codebooks", "d_scales"), kernel, torch_route, want):
        ek, et = relative_error(k, w), relative_error(t, w)
        print(f"{name} {what}: kernel route {ek:.3e}, fp32 torch route {et:.3e}, ratio {ek / et:.3f}")
        assert ek <= 2 * et, (name, what, ek, et)


@pytest.mark.parametrize("name", ["1x16g8", "2x8g8", "8x8g32"])
def test_two_calls_give_the_same_bits_whatever_the_buffers_held(hk, name):
    from aqlm_amd import _native as nat

    d = on_device(name)
    delta, product = step_inputs(hk, name)
    first = (hk.calib_delta(d["codes"], d["codebooks"], d["scales"], d["reference"]),) + tuple(hk.calib_rows(product, delta, d["codes"], d["codebooks"])) \
        + (codebook_grad(hk, name, product),)
    # the cached workspace and the freed outputs are poisoned, then the C entry writes into a NaN-filled output of its own
    if d["nbits"] == 16:
        need = nat.lib.aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(d["out"], d["fin"], d["g"])
    else:
        need = nat.lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(d["out"], d["fin"], d["K"], d["g"])
    ws = hk._workspace(DEV, max(need, 16))
    ws.fill_(float("nan"))
    out = torch.full_like(first[3], float("nan"))
    scales = d["scales"].reshape(-1).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    if d["nbits"] == 16:
        ix = hk.build_codebook_grad_index(d["codes"], d["g"])
        rc = nat.lib.aqlm_hip_calib_codebook_grad_1x16(product.data_ptr(), product.stride(0), scales.data_ptr(), ix.starts.data_ptr(),
                                                       ix.order.data_ptr(), ix.chunks.data_ptr(), ix.chunk_starts.data_ptr(), d["out"], d["fin"],
                                                       d["g"], out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream)
    else:
        rc = nat.lib.aqlm_hip_calib_codebook_grad_kx8(product.data_ptr(), product.stride(0), scales.data_ptr(), d["codes"].data_ptr(), d["out"],
                                                      d["fin"], d["K"], d["g"], out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream)
    assert rc == 0, nat.last_error()
    assert torch.equal(bits(out), bits(first[3]))
    rows_out = torch.full((2, d["out"]), float("nan"), device=DEV)
    rc = nat.lib.aqlm_hip_calib_rows(product.data_ptr(), product.stride(0), delta.data_ptr(), delta.stride(0), d["codes"].data_ptr(),
                                     d["codebooks"].data_ptr(), d["out"], d["fin"], d["K"], d["nbits"], d["g"], rows_out[0].data_ptr(),
                                     rows_out[1].data_ptr(), stream)
    assert rc == 0, nat.last_error()
    assert torch.equal(bits(rows_out[0]), bits(first[1])) and torch.equal(bits(rows_out[1]), bits(first[2]))
    second = (hk.calib_delta(d["codes"], d["codebooks"], d["scales"], d["reference"], out=torch.full_like(delta, float("nan"))),) \
        + tuple(hk.calib_rows(product, delta, d["codes"], d["codebooks"])) + (codebook_grad(hk, name, product),)
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["1x16g16", "2x8g8", "8x8g32"])
def test_a_nan_poisons_its_row_and_the_whole_kx8_codebook_gradient(hk, name):
    d = on_device(name)
    delta, product = step_inputs(hk, name)
    ds_raw, rowloss = hk.calib_rows(product, delta, d["codes"], d["codebooks"])
    poisoned = product.clone()
    poisoned[5, 17] = float("nan")
    ds2, rl2 = hk.calib_rows(poisoned, delta, d["codes"], d["codebooks"])
    keep = torch.arange(d["out"], device=DEV) != 5
    assert torch.isnan(ds2[5]) and torch.isnan(rl2[5])
    assert torch.equal(bits(ds2[keep]), bits(ds_raw[keep])) and torch.equal(bits(rl2[keep]), bits(rowloss[keep]))
    got = codebook_grad(hk, name, poisoned)
    if d["nbits"] == 8:
        assert torch.isnan(got).all()
    else:  # ordinary propagation through the entry of the poisoned position only
        clean = codebook_grad(hk, name, product)
        entry = int(d["unsigned"][5, 17 // d["g"], 0])
        assert torch.isnan(got[entry, 17 % d["g"]])
        others = torch.ones_like(got, dtype=torch.bool)
        others[entry, 17 % d["g"]] = False
        assert torch.equal(bits(got[others]), bits(clean[others]))


@pytest.mark.parametrize("name", ["1x16g8", "2x8g8", "8x8g32"])
def test_a_captured_step_replays_the_eager_bits(hk, tuning, name):
    d = on_device(name)
    books, factors = d["codebooks"].clone(), d["scales"].clone()
    index = hk.build_codebook_grad_index(d["codes"], d["g"]) if d["nbits"] == 16 else None
    run = lambda: tuning.calibrated_loss_and_grads(d["codes"], books, factors, d["reference"], d["xtx"], index=index)  # noqa: E731
    run()  # (the library GEMM picks its kernel and workspace outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(2):
        books.copy_(torch.randn(books.shape, generator=gen, device=DEV))
        factors.copy_(torch.rand(factors.shape, generator=gen, device=DEV) + 0.5)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = run()
        for a, b in zip(replayed, eager):
            assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["2x8g8", "1x16g8"])
def test_quantize_layer_runs_the_kernel_routes_and_lowers_the_error(tuning, scheme):
    from aqlm import QuantizedLinear
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    K, nbits, g = SCHEMES[scheme]
    fin, fout = (128, 96) if scheme == "2x8g8" else (70 * g, 48)
    gen = torch.Generator().manual_seed(21)
    weight = (torch.randn((fout, fin), generator=gen) * 0.05).to(DEV)
    x = torch.randn((2 * fin, fin), generator=gen).to(DEV)
    xtx = x.T @ x / x.shape[0]
    layer = QuantizedLinear(fin, fout, g, 1, K, nbits, bias=False, device=DEV, dtype=torch.float16)
    # The step size.  2x8: the default.  1x16: 65536 centroids for 3360 groups, so the initialisation fits every group exactly and
    # the post-init error is nothing but the fp16 rounding of the codebook (entries of ~ 1 / sqrt(in) = 0.04: half a unit in the last
    # place is 1.5e-5).  Adam's first steps move every element by the full step size whatever the gradient, so ten steps of the default
    # 1e-4 would shake the entries by dozens of units in the last place and bury what the initialisation reached; at 1e-6 ten steps
    # stay below the storage rounding, and what lowers the error is the calibrated search over the rounded codebook.
    lr = 1e-4 if scheme == "2x8g8" else 1e-6
    report = tuning.quantize_layer_(layer, weight, xtx, lr=lr, max_epochs=2, steps_per_epoch=5, init_max_iter=10,
                                    generator=torch.Generator(device=DEV).manual_seed(3), seed=4)
    print(scheme, report)
    assert report["routes"]["grad"] == "kernel" and report["routes"]["search"] == "kernel" and report["epochs"] == 2
    assert len(report["losses"]) == 2 and len(report["changed"]) == 2
    assert report["error"] < report["initial_error"]
    # the derived copies were rebuilt: the forward agrees with F.linear on the layer's own dequantised weight
    dense = _dequantize_weight(unpack_int_data(layer.codes.detach(), nbits), layer.codebooks.detach().float(), layer.scales.detach().float())
    probe = torch.randn((3, fin), generator=gen).to(DEV).half()
    got = layer(probe).float()
    want = F.linear(probe.float(), dense)
    # (fp16 output: half a unit in the last place of the largest output, 2^-11, and as much again for the kernel's own fp32 sums over
    # fp16 products -- 2^-10 of the largest magnitude)
    assert float((got - want).abs().max()) <= 2.0 ** -10 * float(want.abs().max())
