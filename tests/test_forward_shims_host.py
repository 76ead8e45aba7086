"""CPU-only: the argument checks and the row-slab iterator of the forward shims (aqlm_amd/inference_kernels/hip_kernel.py).

The checks of the shims run before anything touches the device, so CPU tensors reach them.  Every expected message below is a
literal: the shims share one helper per message, and a helper that drifts must fail here in every shim at once.  The order cases
pass inputs that are wrong in two ways and pin the error that is raised first.
"""
import re
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def layer(K=1, size=256, g=8, fin=16, fout=4, dtype=F16, og=1, scales_dtype=None):
    """(codes, codebooks, scales) of a fin -> fout layer; contents do not matter."""
    codes = torch.zeros(fout, fin // g, K, dtype=torch.int8 if size == 256 else torch.int16)
    return codes, torch.zeros(K, size, og, g, dtype=dtype), torch.zeros(fout, dtype=scales_dtype or dtype)


def raises(kind, message):
    return pytest.raises(kind, match="^" + re.escape(message) + "$")


def lists(*layers):
    return [l[0] for l in layers], [l[1] for l in layers], [l[2] for l in layers], [None] * len(layers)


X16 = torch.zeros(2, 16, dtype=F16)
X24 = torch.zeros(2, 24, dtype=F16)


# ------------------------------------------------------------------ messages
@pytest.mark.parametrize("count", [0, 5])
def test_gemv_multi_layer_count(hk, count):
    with raises(ValueError, "shared-input ops take 1..4 layers with one entry per list"):
        hk._gemv_multi(X16, *lists(*[layer()] * count), "kx8")


def test_gemv_multi_list_lengths(hk):
    codes, codebooks, scales, bias = lists(layer(), layer())
    with raises(ValueError, "shared-input ops take 1..4 layers with one entry per list"):
        hk._gemv_multi(X16, codes, codebooks, scales[:1], bias, "kx8")
    with raises(ValueError, "shared-input ops take 1..4 layers with one entry per list"):
        hk._gemv_multi(X16, codes, codebooks[:1], scales, bias, "kx8")


def test_packed_multi_layer_count_and_list_lengths(hk):
    message = "code1x16_matmat_packed_multi takes 1..4 layers with one entry per list"
    for count in (0, 5):
        with raises(ValueError, message):
            hk.code1x16_matmat_packed_multi(X16, [None] * count, [None] * count, [None] * count, [None] * count)
    with raises(ValueError, message):
        hk.code1x16_matmat_packed_multi(X16, [None] * 2, [None] * 2, [None], [None] * 2)
    with raises(ValueError, "code8x8_matmat_planar_multi takes 1..4 layers with one entry per list"):
        hk.code8x8_matmat_planar_multi(X16, [None] * 2, [None] * 2, [None] * 2, [None])


def test_out_group_size(hk):
    codes, codebooks, scales = layer(og=2)
    with raises(NotImplementedError, "AQLM HIP kernels require out_group_size == 1"):
        hk._gemv(X16, codes, codebooks, scales, None, "kx8")
    with raises(NotImplementedError, "AQLM HIP kernels require out_group_size == 1"):
        hk._gemv_multi(X16, [codes], [codebooks], [scales], [None], "kx8")


def test_mixed_scheme_and_in_features(hk):
    with raises(NotImplementedError, "all layers of a shared-input launch must use one scheme; got codebooks "
                                     "(2, 256, 1, 8) next to (1, 256, 1, 8)"):
        hk._gemv_multi(X16, *lists(layer(), layer(K=2)), "kx8")
    with raises(ValueError, "all layers of a shared-input launch must have the same in_features and num_codebooks"):
        hk._gemv_multi(X16, *lists(layer(), layer(fin=24)), "kx8")
    with raises(ValueError, "all layers of a shared-input launch must have the same scheme and in_features"):
        hk._gemv_8x8_lut_multi(X16[:1], *lists(layer(K=8), layer(K=8, fin=24)))
    with raises(ValueError, "all layers of a shared-input launch must have the same scheme and in_features"):
        hk._gemv_8x8_lut_multi(X16[:1], *lists(layer(K=8), layer(K=8, g=16, fin=16)))


def test_dtype_mismatch(hk):
    codes, codebooks, scales = layer(dtype=BF16)
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._gemv(X16, codes, codebooks, scales, None, "kx8")
    codes, codebooks, scales = layer(scales_dtype=BF16)   # the message names the codebooks' dtype whichever tensor differs
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.float16"):
        hk._gemv(X16, codes, codebooks, scales, None, "1x16")
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._gemv_multi(X16, *lists(layer(), layer(dtype=BF16)), "kx8")
    packed = SimpleNamespace(in_features=16, device=X16.device)
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._check_packed_args(X16, packed, *layer(dtype=BF16)[1:])
    planar = SimpleNamespace(in_features=16, in_group_size=8, device=X16.device)
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._check_planar_args(X16, planar, *layer(K=8, dtype=BF16)[1:])
    with raises(NotImplementedError, "AQLM HIP kernels only support float16 and bfloat16. Got torch.float32. "
                                     "Please specify the correct `torch_dtype` when loading the model."):
        hk._gemv(X16.float(), *layer(), None, "kx8")


def test_feature_mismatch(hk):
    single, shared = "input has 24 features, layer expects 16", "input has 24 features, layers expect 16"
    with raises(ValueError, single):
        hk._gemv(X24, *layer(), None, "kx8")
    with raises(ValueError, single):
        hk._gemv_8x8_lut(X24, *layer(K=8), None)
    with raises(ValueError, single):
        hk._check_packed_args(X24, SimpleNamespace(in_features=16, device=X24.device), *layer()[1:])
    with raises(ValueError, single):
        hk._check_planar_args(X24, SimpleNamespace(in_features=16, in_group_size=8, device=X24.device), *layer(K=8)[1:])
    with raises(ValueError, single):
        hk.code1x16_matmat_dequant(X24, *layer(size=65536), None)
    with raises(ValueError, single):
        hk.code1x16_matmat_scan(X24, *layer(size=65536), None)
    with raises(ValueError, shared):
        hk._gemv_multi(X24, *lists(layer(), layer()), "kx8")
    with raises(ValueError, shared):
        hk._gemv_8x8_lut_multi(X24[:1], *lists(layer(K=8), layer(K=8)))


def test_codebook_shapes_of_the_shared_input_ops(hk):
    with raises(NotImplementedError, "code1x16_matmat_multi needs codebooks [1, 65536, 1, g], got (1, 256, 1, 8)"):
        hk.code1x16_matmat_multi(X16, *lists(layer()))
    with raises(NotImplementedError, "codekx8_matmat_multi needs codebooks [K, 256, 1, g], got (1, 16, 1, 8)"):
        hk.codekx8_matmat_multi(X16, *lists(layer(), layer(size=16)))
    planar = SimpleNamespace(in_features=16, in_group_size=8, device=X16.device)
    with raises(NotImplementedError, "planar codes of an 8x8 g8 layer need codebooks [8, 256, 1, 8], got (1, 256, 1, 8)"):
        hk._check_planar_args(X16, planar, *layer()[1:])
    with raises(ValueError, "input on cpu, layer on meta"):
        hk._check_packed_args(X16, SimpleNamespace(in_features=16, device=torch.device("meta")), *layer()[1:])


# ------------------------------------------------------------------ order: the first of two errors
def test_gemv_checks_out_group_size_then_dtypes_then_features(hk):
    codes, codebooks, scales = layer(og=2, dtype=BF16)
    with raises(NotImplementedError, "AQLM HIP kernels require out_group_size == 1"):
        hk._gemv(X24, codes, codebooks, scales, None, "kx8")
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._gemv(X24, *layer(dtype=BF16), None, "kx8")


def test_gemv_multi_checks_features_first_and_then_layer_by_layer(hk):
    with raises(ValueError, "input has 24 features, layers expect 16"):   # before any per-layer check
        hk._gemv_multi(X24, *lists(layer(), layer(K=2)), "kx8")
    # layer 0 has the wrong dtype and layer 1 the wrong scheme: every check of layer 0 runs before any check of layer 1
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._gemv_multi(X16, *lists(layer(dtype=BF16), layer(K=2, dtype=BF16)), "kx8")
    # within one layer: scheme, then in_features, then dtypes
    with raises(ValueError, "all layers of a shared-input launch must have the same in_features and num_codebooks"):
        hk._gemv_multi(X16, *lists(layer(), layer(fin=24, scales_dtype=BF16)), "kx8")


def test_packed_and_planar_checks_put_dtypes_first(hk):
    planar = SimpleNamespace(in_features=16, in_group_size=8, device=X24.device)
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._check_planar_args(X24, planar, *layer(dtype=BF16)[1:])   # also the wrong codebook shape and feature count
    with raises(NotImplementedError, "planar codes of an 8x8 g8 layer need codebooks [8, 256, 1, 8], got (1, 256, 1, 8)"):
        hk._check_planar_args(X24, planar, *layer()[1:])             # shape before features
    with raises(NotImplementedError, "input dtype torch.float16 must match codebooks/scales dtype torch.bfloat16"):
        hk._check_packed_args(X24, SimpleNamespace(in_features=16, device=torch.device("meta")), *layer(dtype=BF16)[1:])
    with raises(ValueError, "input has 24 features, layer expects 16"):   # features before devices
        hk._check_packed_args(X24, SimpleNamespace(in_features=16, device=torch.device("meta")), *layer()[1:])


# ------------------------------------------------------------------ the row-slab iterator
@pytest.mark.parametrize("dtype", [F16, torch.float32])
@pytest.mark.parametrize("rows", [1, 8, 9, 17])
def test_row_slabs_tile_the_rows(hk, rows, dtype):
    from aqlm_amd import _native

    x = torch.zeros(rows, 40, dtype=dtype)[:, :32]   # a row stride larger than the row
    assert x.stride(0) == 40
    slabs = list(hk._row_slabs(x))
    assert [b0 for b0, _, _, _ in slabs] == list(range(0, rows, _native.MAX_GEMV_BATCH))
    assert all(1 <= nb <= _native.MAX_GEMV_BATCH for _, nb, _, _ in slabs)
    covered = [r for b0, nb, _, _ in slabs for r in range(b0, b0 + nb)]
    assert covered == list(range(rows))              # every row once, in order
    y = torch.zeros(rows, 24, dtype=dtype)
    for b0, nb, xp, offset in slabs:
        assert xp == x.data_ptr() + b0 * x.stride(0) * x.element_size() == x[b0].data_ptr()
        assert y.data_ptr() + offset * y.shape[1] == y[b0].data_ptr()
