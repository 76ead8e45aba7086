"""Numpy models of the calibrated-training entries (include/aqlm_hip.h, aqlm_hip_calib_*): the arithmetic of each, step by step, so that a
test can hold the kernels to it bit for bit.

``fma32`` is a correctly rounded fp32 fused multiply-add (the product of two fp32 values is exact in fp64; the sum is rounded to odd
in fp64 and then once to fp32).  ``wave_sum`` / ``row16_sum`` are the fixed trees of aqlm_common.h.  ``rows`` restates aqlm_hip_calib_rows
(lane l of a row's wave takes the groups l, l + 64, ..., products over t ascending), ``dc_1x16`` the chunk sums of
aqlm_hip_calib_codebook_grad_1x16 (16 lanes per chunk, positions l, l + 16, ... of the chunk, the butterfly, then the chunks of an entry in
order) and ``dc_kx8`` the fixed-point sums of aqlm_hip_calib_codebook_grad_kx8 (tests/kx8_grad_model.py with fp32 scales: the product of
two fp32 values is exact in fp64 as well).  ``values`` are UNSIGNED entries: [out, in / g] for 1x16, [out, in / g, K] for K x 8."""
import numpy as np

from tests import kx8_grad_model

F32 = np.float32


def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, elementwise on fp32 arrays."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b  # exact: 24 x 24 significant bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
        bits = s.view(np.int64).copy()
        inexact = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        step = np.where((err > 0) == (s > 0), 1, -1)
        bits = np.where(inexact, bits + step, bits)  # round to odd: the later rounding to fp32 sees which side of a tie it is on
        return bits.view(np.float64).astype(F32)


def _lane_perms(width):
    i = np.arange(width)
    return [i ^ 1, i ^ 2, (i & ~7) | (7 - (i & 7)), (i & ~15) | (15 - (i & 15))]


def row16_sum(v):
    """[..., 16 * n] fp32 -> the same shape: every lane holds the sum of its row of 16 lanes (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
    row_half_mirror, row_mirror)."""
    v = np.asarray(v, dtype=F32)
    for perm in _lane_perms(v.shape[-1]):
        v = (v + v[..., perm]).astype(F32)
    return v


def wave_sum(v):
    """[..., 64] fp32 -> [...]: the rows by ``row16_sum``, then (r0 + r1) + (r2 + r3)."""
    v = row16_sum(v)
    return ((v[..., 0] + v[..., 16]).astype(F32) + (v[..., 32] + v[..., 48]).astype(F32)).astype(F32)


def unscaled_rows(values, codebooks):
    """w [out, in / g, g] fp32: ((C_0[v_0] + C_1[v_1]) + ...) in codebook order; codebooks [K, S, g] fp32."""
    values = values.reshape(values.shape[0], values.shape[1], -1)
    w = codebooks[0][values[:, :, 0]].astype(F32)
    for c in range(1, values.shape[2]):
        w = (w + codebooks[c][values[:, :, c]]).astype(F32)
    return w


def delta(values, codebooks, scales, reference):
    """D [out, in] fp32 = fp32(fp32(s * w) - W_ref); ``reference`` already as fp32 values."""
    w = unscaled_rows(values, codebooks)
    scaled = (scales.astype(F32).reshape(-1, 1, 1) * w).astype(F32)
    return (scaled.reshape(reference.shape) - reference.astype(F32)).astype(F32)


def rows(values, codebooks, g_matrix, d_matrix):
    """(ds_raw [out], rowloss [out]) fp32."""
    w = unscaled_rows(values, codebooks)
    out, nj, g = w.shape
    gm = np.asarray(g_matrix, dtype=F32).reshape(out, nj, g)
    dm = np.asarray(d_matrix, dtype=F32).reshape(out, nj, g)
    ds = np.zeros((out, 64), dtype=F32)
    rl = np.zeros((out, 64), dtype=F32)
    for first in range(0, nj, 64):
        lanes = min(64, nj - first)
        for t in range(g):
            ds[:, :lanes] = fma32(gm[:, first:first + lanes, t], w[:, first:first + lanes, t], ds[:, :lanes])
            rl[:, :lanes] = fma32(gm[:, first:first + lanes, t], dm[:, first:first + lanes, t], rl[:, :lanes])
    with np.errstate(invalid="ignore", over="ignore"):
        return wave_sum(ds), wave_sum(rl)


def dc_1x16(values, g_matrix, scales, g, chunk):
    """dC [65536, g] fp32 through the inverted index: ascending positions per entry, chunks of ``chunk`` positions."""
    out, nj = values.shape
    gm = np.asarray(g_matrix, dtype=F32).reshape(out, nj, g)
    s = np.asarray(scales, dtype=F32).reshape(-1)
    flat = values.reshape(-1)
    order = np.argsort(flat, kind="stable")
    dc = np.zeros((65536, g), dtype=F32)
    for entry in np.unique(flat):
        positions = order[np.searchsorted(flat[order], entry, "left"):np.searchsorted(flat[order], entry, "right")]
        partials = []
        for begin in range(0, len(positions), chunk):
            part = positions[begin:begin + chunk]
            acc = np.zeros((16, g), dtype=F32)
            for i, p in enumerate(part):  # lane i % 16 takes the positions i % 16, i % 16 + 16, ... of the chunk in list order
                o, j = divmod(int(p), nj)
                acc[i % 16] = fma32(np.full(g, s[o], dtype=F32), gm[o, j], acc[i % 16])
            with np.errstate(invalid="ignore", over="ignore"):
                partials.append(row16_sum(acc.T)[:, 0])
        if len(partials) == 1:
            dc[entry] = partials[0]
        else:
            total = np.zeros(g, dtype=F32)
            with np.errstate(invalid="ignore", over="ignore"):
                for part in partials:
                    total = (total + part).astype(F32)
            dc[entry] = total
    return dc


def dc_kx8(values, g_matrix, scales, g):
    """dC [K, 256, g] fp32: the fixed-point scheme of aqlm_hip_codebook_grad_kx8 on fp32 G and fp32 scales."""
    return kx8_grad_model.fixed_point_dc(values, np.asarray(g_matrix, dtype=F32).astype(np.float64),
                                         np.asarray(scales, dtype=F32).astype(np.float64).reshape(-1), g)
