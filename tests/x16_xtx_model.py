"""The arithmetic of aqlm_hip_code_search_1x16_xtx (include/aqlm_hip.h) restated in numpy, operation for operation: it is
tests/kx8_xtx_model.py with ONE codebook of 65536 entries and the key ``b * 65536 + s'``.  Every product and every sum below is ONE
IEEE operation of ``dtype`` (float32: what the kernel computes; float64: the reference arithmetic the whole call is compared with),
rounded to nearest, no fused multiply-add (numpy does not contract), sums over f ascending from the first product.  For one input
group, every output row o with scale s (2s = 2 * s, ss = s * s) and P positions holding loss L[b], slice t[b] and code p:

    w[f]     = s * C[p][f]
    u[b][f'] = t[b][f'] + sum_f w[f] * H[f][f']
    base[b]  = (L[b] + 2s * sum_f C[p][f] * u[b][f]) - ss * q[p]
    S(b, s') = (base[b] - 2s * sum_f C[s'][f] * u[b][f]) + ss * q[s']        (-0 replaced by +0)
    keep beam_size by (S, b * 65536 + s') ascending (a stable sort of the flat scores: NaN last); rank i from (b, s'):
        code[i] = s';  source[i] = b;  L[i] = S(b, s')
        dw[f] = s * C[s'][f] - s * C[p][f];  delta[i] = dw;  t[i][f'] = t[b][f'] - sum_f dw[f] * H[f][f']

The 65536 * P scores of a row are never sorted whole: the best ``beam_size + 1`` are what a stable sort of the row would put first,
found through a partition (a row whose partition meets a NaN is sorted whole).  ``search_layer`` drives ``step`` group by group over a
layer with an exact (``dtype``) propagation of T."""
import numpy as np

SIZE = 65536
NEAR = 2.0 ** -18


def _dot(a, b):
    acc = a[..., 0] * b[..., 0]
    for f in range(1, a.shape[-1]):
        acc = acc + a[..., f] * b[..., f]
    return acc


def _vecmat(w, H):
    """out[..., f'] = sum over f ascending of w[..., f] * H[f, f']"""
    acc = w[..., 0, None] * H[0]
    for f in range(1, H.shape[0]):
        acc = acc + w[..., f, None] * H[f]
    return acc


def _first(flat, count):
    """The first ``count`` indices of a stable ascending sort of the 1-d ``flat`` (NaN last), without sorting it whole."""
    kth = np.partition(flat, count - 1)[count - 1]
    if not kth == kth:
        return np.argsort(flat, kind="stable")[:count]
    among = np.nonzero(flat <= kth)[0]  # ascending indices: a stable sort of these keeps equal scores in index order
    return among[np.argsort(flat[among], kind="stable")[:count]]


def step(t, loss, codes_in, H, q, codebook, scales, beam_size, dtype=np.float32, near=0.0):
    """t [P, out, g], loss [P, out], codes_in [P, out] or [P, out, 1] (any integer form: taken mod 65536), H [g, g], q [65536], codebook
    [65536, g], scales [out] or None -> dict: loss [B, out], codes [B, out] int64 in 0 .. 65535, source [B, out], delta [B, out, g],
    t [B, out, g], tied [out] bool (two adjacent scores among the row's best beam_size + 1 are equal, or closer than ``near`` times the
    row's largest finite |score|, or one of them is not finite)."""
    book = np.asarray(codebook).astype(dtype).reshape(SIZE, -1)
    g = book.shape[1]
    t = np.asarray(t).astype(dtype)
    loss = np.asarray(loss).astype(dtype)
    H, q = np.asarray(H).astype(dtype), np.asarray(q).astype(dtype).reshape(SIZE)
    P, out, _ = t.shape
    s = np.ones((out,), dtype=dtype) if scales is None else np.asarray(scales).astype(dtype).reshape(out)
    two_s, ss = dtype(2) * s, s * s
    code = np.asarray(codes_in).astype(np.int64).reshape(P, out) % SIZE
    keep = beam_size
    picked = np.zeros((keep, out), dtype=np.int64)
    values = np.zeros((keep, out), dtype=dtype)
    tied = np.zeros((out,), dtype=bool)
    with np.errstate(all="ignore"):
        prev_entry = book[code]  # [P, out, g]
        w = s[None, :, None] * prev_entry
        u = t + _vecmat(w, H)
        base = (loss + two_s[None, :] * _dot(prev_entry, u)) - ss[None, :] * q[code]
        for o in range(out):
            acc = u[:, o, 0, None] * book[None, :, 0]  # [P, 65536]
            for f in range(1, g):
                acc = acc + u[:, o, f, None] * book[None, :, f]
            S = (base[:, o, None] - two_s[o] * acc) + (ss[o] * q)[None, :]
            flat = (S + dtype(0)).reshape(P * SIZE)  # -0 -> +0
            ranked = _first(flat, keep + 1)
            best = flat[ranked]
            largest = np.where(np.isfinite(flat), np.abs(flat), 0).max()
            tied[o] = ((best[1:] - best[:-1]) <= near * largest).any() or not np.isfinite(best).all()
            picked[:, o], values[:, o] = ranked[:keep], best[:keep]
        rows = np.arange(out)[None, :]
        source, chosen = picked // SIZE, picked % SIZE
        dw = s[None, :, None] * book[chosen] - s[None, :, None] * book[code[source, rows]]
        t_new = t[source, rows] - _vecmat(dw, H)
    return {"loss": values, "codes": chosen, "source": source, "delta": dw, "t": t_new, "tied": tied}


def group_q(codebook, H, dtype=np.float64):
    """[65536]: C[s] H C[s]^T"""
    book = np.asarray(codebook).astype(dtype).reshape(SIZE, -1)
    return np.einsum("sf,fh,sh->s", book, np.asarray(H).astype(dtype), book)


def search_layer(XTX, reference, codebook, prev, scales, beam_size, group_order=None, dtype=np.float64, near=NEAR):
    """The whole call: XTX [in, in], reference [out, in], codebook [65536, g], prev [out, in / g] or [out, in / g, 1] (any integer form),
    scales [out] or None -> (codes [out, in / g, 1] int64 in 0 .. 65535, tied [out])."""
    book = np.asarray(codebook).astype(dtype).reshape(SIZE, -1)
    g = book.shape[1]
    XTX, reference = np.asarray(XTX).astype(dtype), np.asarray(reference).astype(dtype)
    out, fin = reference.shape
    ng = fin // g
    codes = (np.asarray(prev).astype(np.int64).reshape(out, ng) % SIZE)[None]  # [P, out, ng]
    s = np.ones((out,), dtype=dtype) if scales is None else np.asarray(scales).astype(dtype).reshape(out)
    weight = book[codes[0]].reshape(out, fin) * s[:, None]
    error = reference - weight
    T = (error @ XTX)[None]
    loss = (T[0] * error).sum(-1)[None]
    groups = list(range(ng)) if group_order is None else [int(j) for j in group_order]
    assert sorted(groups) == list(range(ng))
    tied = np.zeros((out,), dtype=bool)
    rows = np.arange(out)[None, :]
    for j in groups:
        cols = slice(j * g, (j + 1) * g)
        H = XTX[cols, cols]
        r = step(T[:, :, cols], loss, codes[:, :, j], H, group_q(book, H, dtype), book, s, beam_size, dtype, near)
        tied |= r["tied"]
        T = T[r["source"], rows] - r["delta"] @ XTX[cols, :]
        codes = codes[r["source"], rows].copy()
        codes[:, :, j] = r["codes"]
        loss = r["loss"]
    return codes[0][:, :, None], tied
