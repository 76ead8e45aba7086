"""The arithmetic of aqlm_hip_code_search_kx8_xtx (include/aqlm_hip.h) restated in numpy, operation for operation: every product and
every sum below is ONE IEEE operation of ``dtype`` (float32: what the kernel computes; float64: the reference arithmetic the whole
call is compared with), rounded to nearest, no fused multiply-add (numpy does not contract), sums over f ascending.  For one input
group, every output row o with scale s (2s = 2 * s, ss = s * s) and P positions holding loss L[b], slice t[b], codes beam[b], entry
position src[b] = b and weight change d[b] = 0:

    step c of dim_order, p = beam[b][c]:
        w[b][f]  = s * C_c[p][f]
        u[b][f'] = t[b][f'] + sum_f w[b][f] * H[f][f']
        base[b]  = (L[b] + 2s * sum_f C_c[p][f] * u[b][f]) - ss * q[c][p]
        S(b, s') = (base[b] - 2s * sum_f C_c[s'][f] * u[b][f]) + ss * q[c][s']        (-0 replaced by +0)
        keep min(beam_size, P * 256) by (S, b * 256 + s') ascending (a stable sort of the flat scores); rank i from (b, s'):
            beam[i] = beam[b] with code c = s';  src[i] = src[b];  L[i] = S(b, s')
            dw[f] = s * C_c[s'][f] - s * C_c[p][f];  d[i] = d[b] + dw;  t[i][f'] = t[b][f'] - sum_f dw[f] * H[f][f']

``search_layer`` drives ``step`` group by group over a layer with an exact (``dtype``) propagation of T: the whole calibrated search
of the reference's src/beam_search_xtx.py in the incremental form of DESIGN.md 4.8o."""
import numpy as np

SIZE = 256
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


def step(t, loss, codes_in, H, q, codebooks, scales, beam_size, dim_order=None, dtype=np.float32, near=0.0):
    """t [P, out, g], loss [P, out], codes_in [P, out, K] (any integer form: taken mod 256), H [g, g], q [K, 256], codebooks [K, 256, g],
    scales [out] or None -> dict: loss [B, out], codes [B, out, K] int64 in 0 .. 255, source [B, out], delta [B, out, g], t [B, out, g],
    tied [out] bool (some step of the row had two adjacent scores among its best keep + 1 that are equal, or closer than ``near`` times
    the step's largest finite |score|)."""
    books = np.asarray(codebooks).astype(dtype)
    K, size, g = books.shape
    assert size == SIZE
    t = np.asarray(t).astype(dtype).copy()
    loss = np.asarray(loss).astype(dtype).copy()
    H, q = np.asarray(H).astype(dtype), np.asarray(q).astype(dtype)
    P, out, _ = t.shape
    s = np.ones((out,), dtype=dtype) if scales is None else np.asarray(scales).astype(dtype).reshape(out)
    two_s, ss = dtype(2) * s, s * s
    order = list(range(K)) if dim_order is None else [int(c) for c in dim_order]
    assert sorted(order) == list(range(K))
    beams = np.asarray(codes_in).astype(np.int64) % SIZE
    src = np.broadcast_to(np.arange(P)[:, None], (P, out)).copy()
    d = np.zeros((P, out, g), dtype=dtype)
    tied = np.zeros((out,), dtype=bool)
    rows = np.arange(out)[None, :]
    with np.errstate(all="ignore"):
        for c in order:
            P = t.shape[0]
            code = beams[:, :, c]
            prev_entry = books[c][code]
            w = s[None, :, None] * prev_entry
            u = t + _vecmat(w, H)
            base = (loss + two_s[None, :] * _dot(prev_entry, u)) - ss[None, :] * q[c][code]
            acc = u[:, :, 0, None] * books[c][None, None, :, 0]
            for f in range(1, g):
                acc = acc + u[:, :, f, None] * books[c][None, None, :, f]
            S = (base[:, :, None] - two_s[None, :, None] * acc) + (ss[:, None] * q[c][None, :])[None]
            S = S + dtype(0)  # -0 -> +0
            flat = S.transpose(1, 0, 2).reshape(out, P * SIZE)
            keep = min(beam_size, P * SIZE)
            ranked = np.argsort(flat, axis=1, kind="stable")[:, :keep + 1]
            best = np.take_along_axis(flat, ranked, axis=1)
            largest = np.where(np.isfinite(flat), np.abs(flat), 0).max(axis=1)
            tied |= ((best[:, 1:] - best[:, :-1]) <= near * largest[:, None]).any(axis=1) | ~np.isfinite(best).all(axis=1)
            picked = ranked[:, :keep].T  # [keep, out]
            source, chosen = picked // SIZE, picked % SIZE
            dw = s[None, :, None] * books[c][chosen] - s[None, :, None] * books[c][code[source, rows]]
            d = d[source, rows] + dw
            t = t[source, rows] - _vecmat(dw, H)
            beams = beams[source, rows].copy()
            beams[:, :, c] = chosen
            src = src[source, rows]
            loss = best[:, :keep].T.copy()
    return {"loss": loss, "codes": beams, "source": src, "delta": d, "t": t, "tied": tied}


def group_q(codebooks, H, dtype=np.float64):
    """[K, 256]: C_c[s] H C_c[s]^T"""
    books = np.asarray(codebooks).astype(dtype)
    return np.einsum("ksf,fh,ksh->ks", books, np.asarray(H).astype(dtype), books)


def search_layer(XTX, reference, codebooks, prev, scales, beam_size, group_order=None, dim_orders=None, dtype=np.float64, near=NEAR):
    """The whole call: XTX [in, in], reference [out, in], codebooks [K, 256, g], prev [out, in / g, K] (any integer form), scales [out] or
    None -> (codes [out, in / g, K] int64 in 0 .. 255, tied [out]).  ``dim_orders``: None, one permutation, or one per visited group."""
    books = np.asarray(codebooks).astype(dtype)
    K, _, g = books.shape
    XTX, reference = np.asarray(XTX).astype(dtype), np.asarray(reference).astype(dtype)
    out, fin = reference.shape
    ng = fin // g
    codes = (np.asarray(prev).astype(np.int64) % SIZE)[None]  # [P, out, ng, K]
    s = np.ones((out,), dtype=dtype) if scales is None else np.asarray(scales).astype(dtype).reshape(out)
    weight = sum(books[c][codes[0, :, :, c]] for c in range(K)).reshape(out, fin) * s[:, None]
    error = reference - weight
    T = (error @ XTX)[None]
    loss = (T[0] * error).sum(-1)[None]
    groups = list(range(ng)) if group_order is None else [int(j) for j in group_order]
    assert sorted(groups) == list(range(ng))
    if dim_orders is None or not isinstance(dim_orders[0], (list, tuple)):
        dim_orders = [dim_orders] * ng
    tied = np.zeros((out,), dtype=bool)
    rows = np.arange(out)[None, :]
    for j, order in zip(groups, dim_orders):
        cols = slice(j * g, (j + 1) * g)
        H = XTX[cols, cols]
        r = step(T[:, :, cols], loss, codes[:, :, j], H, group_q(books, H, dtype), books, s, beam_size, order, dtype, near)
        tied |= r["tied"]
        T = T[r["source"], rows] - r["delta"] @ XTX[cols, :]
        codes = codes[r["source"], rows].copy()
        codes[:, :, j] = r["codes"]
        loss = r["loss"]
    return codes[0], tied
