"""Numpy models of the K x 8 gradient entries (include/aqlm_hip.h, aqlm_hip_codebook_grad_kx8 / aqlm_hip_scales_grad_kx8).

``fixed_point_dc`` restates the documented arithmetic of the codebook gradient step by step -- int64 accumulation, ``np.rint``,
``astype(np.float32)``, ``ldexp`` -- so that a test can hold the kernel to it bit for bit; ``exact_dc`` / ``exact_ds`` are the plain
fp64 sums.  Shapes: ``values`` [out, in / g, K] unsigned entries (0..255), ``dw64`` [out, in] and ``s64`` [out] in float64 holding the
values the kernel reads (already rounded to the dtype of dW / the scales)."""
import numpy as np

UNIT = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8, "float32": 2.0 ** -24}
TINY = {"float16": 2.0 ** -25, "bfloat16": 2.0 ** -134, "float32": 2.0 ** -150}  # half the spacing of the output's subnormals


def shift_of(out_features, in_features, g):
    return 62 - int(out_features * (in_features // g)).bit_length()


def exponent_of(dw64, s64):
    """E of ``bound = max|s| * max|dW| = m * 2^E``, m in [0.5, 1); None when the bound is zero or not finite."""
    bound = float(np.abs(s64).max()) * float(np.abs(dw64).max())
    if not np.isfinite(bound) or bound == 0.0:
        return None
    return int(np.frexp(bound)[1])


def _scatter(values, terms, g):
    """terms [out, nj, g] (any dtype with an exact add) summed per (codebook, entry)."""
    out, nj, K = values.shape
    acc = np.zeros((K, 256, g), dtype=terms.dtype)
    flat = terms.reshape(-1, g)
    for c in range(K):
        np.add.at(acc[c], values[:, :, c].reshape(-1), flat)
    return acc


def counts(values):
    out, nj, K = values.shape
    return np.stack([np.bincount(values[:, :, c].reshape(-1), minlength=256) for c in range(K)])  # [K, 256]


def exact_dc(values, dw64, s64, g):
    """(dC [K, 256, g] in fp64, the sum of the terms' magnitudes)."""
    out, nj, K = values.shape
    terms = dw64.reshape(out, nj, g) * s64.reshape(out, 1, 1)
    return _scatter(values, terms, g), _scatter(values, np.abs(terms), g)


def fixed_point_dc(values, dw64, s64, g):
    """The kernel's arithmetic: fp32 [K, 256, g] before the rounding to the output dtype."""
    out, nj, K = values.shape
    if not (np.isfinite(dw64).all() and np.isfinite(s64).all()):
        return np.full((K, 256, g), np.nan, dtype=np.float32)
    E = exponent_of(dw64, s64)
    if E is None:
        return np.zeros((K, 256, g), dtype=np.float32)
    shift = shift_of(out, nj * g, g)
    scaled = (s64.reshape(out, 1, 1) * dw64.reshape(out, nj, g)) * 2.0 ** (shift - E)  # exact, exact
    q = np.rint(scaled).astype(np.int64)
    assert np.abs(q).max() <= 2 ** shift
    S = _scatter(values, q, g)
    return np.ldexp(S.astype(np.float32), E - shift).astype(np.float32)


def dc_bound(values, dw64, s64, g, out_dtype_name):
    """|got - exact| <= n * u / 2 + (2^-24 + u_out) * (|exact| + n * u / 2) + tiny_out, per element."""
    out, nj, K = values.shape
    E = exponent_of(dw64, s64)
    u = 2.0 ** (E - shift_of(out, nj * g, g))
    n = counts(values).astype(np.float64).reshape(K, 256, 1)
    exact, _ = exact_dc(values, dw64, s64, g)
    return n * u / 2 + (2.0 ** -24 + UNIT[out_dtype_name]) * (np.abs(exact) + n * u / 2) + TINY[out_dtype_name]


def exact_ds(values, dw64, cb64, g):
    """(ds [out] in fp64, the sum of the terms' magnitudes); cb64 [K, 256, g]."""
    out, nj, K = values.shape
    w = np.zeros((out, nj, g))
    wabs = np.zeros((out, nj, g))
    for c in range(K):
        w += cb64[c][values[:, :, c]]
        wabs += np.abs(cb64[c][values[:, :, c]])
    d = dw64.reshape(out, nj, g)
    return (d * w).sum((1, 2)), (np.abs(d) * wabs).sum((1, 2))
