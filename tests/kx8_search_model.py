"""The arithmetic of aqlm_hip_code_search_kx8 (include/aqlm_hip.h) restated in numpy, operation for operation: every product and
every sum below is ONE IEEE operation of ``dtype`` (float32: what the kernel computes; float64: the check that inputs on the
dyadic grid are exact), rounded to nearest, no fused multiply-add (numpy does not contract).  For a group with previous codes p:

    r      = float(reference group) / float(scale of its row)                      (no scales: r = reference)
    dot    : acc = a0 * b0, then acc = acc + aj * bj for j = 1 .. d - 1
    cn     = dot(C_c[s], C_c[s])
    kept   = C_0[p_0], then kept = kept + C_c[p_c] for c = 1 .. K - 1;  res[0] = r - kept, one position whose beam is p
    step c of dim_order:  res[b] = res[b] + C_c[beam[b][c]];  rn[b] = dot(res[b], res[b]);
                          S(b, s) = (rn[b] - 2 * dot(res[b], C_c[s])) + cn[c][s]
                          keep the best 1 (last step) or min(beam_size, positions * 256) by (S, b * 256 + s) ascending (a stable sort
                          of the flat scores: equal floats -- -0 and +0 included -- go to the smaller flat index); rank i takes the
                          codes of its source position with code c replaced;
                          not the last step: res[i] = res_old[i] - C_c[chosen_i], POSITION BY POSITION (after the first step
                          every new position starts from old position 0)
    result = the codes of rank 0 and its S on the last step.

``dyadic_case`` generates inputs on a grid of 2^-6 small enough that every intermediate is an integer below 2^24 in units of the
grid (or its square): float32 and float64 then compute the same numbers."""
import numpy as np

SIZE = 256
GRID = 2.0 ** -6


def _dot(a, b):
    acc = a[..., 0] * b[..., 0]
    for j in range(1, a.shape[-1]):
        acc = acc + a[..., j] * b[..., j]
    return acc


def quotient(reference, scales, in_group_size, dtype=np.float32):
    """[N, g]: r of the definition for every group of ``reference`` [out, in] (``scales`` [out] or None)."""
    r = np.asarray(reference).astype(dtype)
    if scales is not None:
        r = r / np.asarray(scales).astype(dtype).reshape(-1, 1)
    return np.ascontiguousarray(r.reshape(-1, in_group_size))


def search_groups(r, codebooks, prev, beam_size, dim_order=None, dtype=np.float32):
    """r [N, d], codebooks [K, 256, d], prev [N, K] (any integer form: taken mod 256) -> (codes [N, K] int64 in 0 .. 255, the score of
    the returned hypothesis [N], tied [N] bool: some step of the group had two equal scores among its best keep + 1)."""
    books = np.asarray(codebooks).astype(dtype)
    K, size, d = books.shape
    assert size == SIZE
    r = np.asarray(r).astype(dtype)
    N = r.shape[0]
    order = list(range(K)) if dim_order is None else [int(c) for c in dim_order]
    assert sorted(order) == list(range(K))
    two = dtype(2)
    prev = np.asarray(prev).astype(np.int64) % SIZE
    norms = np.stack([_dot(books[c], books[c]) for c in range(K)])
    beams = prev[:, None, :].copy()
    kept = books[0][prev[:, 0]]
    for c in range(1, K):
        kept = kept + books[c][prev[:, c]]
    res = (r - kept)[:, None, :]
    tied = np.zeros((N,), dtype=bool)
    rows = np.arange(N)
    score = None
    for step, c in enumerate(order):
        last = step == K - 1
        res = res + books[c][beams[:, :, c]]
        positions = res.shape[1]
        rn = _dot(res, res)
        acc = res[:, :, 0, None] * books[c][None, None, :, 0]
        for j in range(1, d):
            acc = acc + res[:, :, j, None] * books[c][None, None, :, j]
        flat = ((rn[:, :, None] - two * acc) + norms[c][None, None, :]).reshape(N, positions * SIZE)
        keep = 1 if last else min(beam_size, positions * SIZE)
        ranked = np.argsort(flat, axis=1, kind="stable")[:, :keep + 1]
        best = np.take_along_axis(flat, ranked, axis=1)
        tied |= (best[:, 1:] == best[:, :-1]).any(axis=1)
        picked = ranked[:, :keep]
        source, chosen = picked // SIZE, picked % SIZE
        beams = np.take_along_axis(beams, source[:, :, None], axis=1).copy()
        beams[:, :, c] = chosen
        if last:
            score = flat[rows, picked[:, 0]]
        else:
            res = res - books[c][chosen]
    return beams[:, 0, :], score, tied


def search(reference, scales, codebooks, prev, in_group_size, beam_size, dim_order=None, dtype=np.float32):
    """The whole layer: ``reference`` [out, in], ``scales`` [out] or None, ``prev`` [out * in / g, K]."""
    return search_groups(quotient(reference, scales, in_group_size, dtype), codebooks, prev, beam_size, dim_order, dtype)


def dyadic_case(num_codebooks, in_group_size, out_features=64, groups_per_row=32, seed=0):
    """Inputs on the grid: codebook entries rint(N(0, m / 3)) clipped to +-m (m = 127; 31 for K = 8 at g 32) times 2^-6, targets
    the sum of planted codewords plus rint(N(0, 12)) clipped to +-255 (times 2^-6), scales powers of two.  Returns a dict of float32
    / int64 arrays: codebooks [K, 256, g], reference [out, in], scales [out], prev [N, K]."""
    K, g = num_codebooks, in_group_size
    m = 31 if (K == 8 and g == 32) else 127
    rng = np.random.default_rng(100000 * K + 1000 * g + seed)
    books = np.clip(np.rint(rng.normal(0.0, m / 3.0, size=(K, SIZE, g))), -m, m)
    N = out_features * groups_per_row
    planted = rng.integers(0, SIZE, size=(N, K))
    noise = np.clip(np.rint(rng.normal(0.0, 12.0, size=(N, g))), -255, 255)
    r = sum(books[c][planted[:, c]] for c in range(K)) + noise
    scales = 2.0 ** rng.integers(-3, 4, size=(out_features,))
    reference = (r * GRID).reshape(out_features, groups_per_row * g) * scales[:, None]
    # the previous codes: the planted ones, with one code of every second group (at random) drawn anew, so that about half of the
    # groups have something to find
    prev = planted.copy()
    moved = np.flatnonzero(rng.random(N) < 0.5)
    prev[moved, rng.integers(0, K, size=moved.shape[0])] = rng.integers(0, SIZE, size=moved.shape[0])
    return {"codebooks": (books * GRID).astype(np.float32), "reference": reference.astype(np.float32), "scales": scales.astype(np.float32),
            "prev": prev.astype(np.int64), "K": K, "g": g, "out": out_features, "in": groups_per_row * g}
