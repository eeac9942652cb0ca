"""The yardstick of product-quantized search (tests/test_pq_search.py; the definition: include/quake_hip.h, "product-quantized
search") in numpy, float32 throughout: dot products are the oracle's fmaf chain (O.pair_values, "ip"), fmaf(-2, v, n)
is n - 2 v in float32 (the product by 2 is exact, one rounding is left), codes by argmin with the tie rule, the table by a float32
subtraction and division, keys as integer sums, candidates by np.lexsort on (key, row), exact keys and the final order through the
oracle as tests/bin_yardstick.py does it.  The input is the CSR in arena order: rows are named by their position in it."""
import numpy as np

import oracle as O

F = np.float32
BINS = 8192


def _dots(a, cb, m):
    """[n, 256]: dot(a_m, w[m][c]) for the rows of a [n, d]"""
    dsub = cb.shape[2]
    return O.pair_values(np.ascontiguousarray(a[:, m * dsub:(m + 1) * dsub]), cb[m], "ip")


def norms(cb):
    """n [M, 256]: dot(w, w)"""
    return np.stack([np.diagonal(O.pair_values(cb[m], cb[m], "ip")).astype(F) for m in range(cb.shape[0])])


def codes(vecs, cb):
    """[n, M] uint8: per sub-space the c smallest under (e is NaN, e, c)"""
    n = norms(cb)
    out = np.zeros((vecs.shape[0], cb.shape[0]), np.uint8)
    for m in range(cb.shape[0]):
        with np.errstate(all="ignore"):
            e = n[m][None, :] - F(2) * _dots(vecs, cb, m)
        assert e.dtype == F
        nan = np.isnan(e)
        out[:, m] = np.argmin(np.where(nan, F(np.inf), e), 1)  # (the first of equal e: -0 and +0 are equal)
        for r in np.nonzero(nan.any(1))[0]:  # (a NaN comes behind +inf)
            out[r, m] = min(range(256), key=lambda c: (bool(nan[r, c]), float(e[r, c]) if not nan[r, c] else 0.0, c))
    return out


def table(q, cb, metric):
    """u [Q, M, 256] uint16"""
    Q, M = q.shape[0], cb.shape[0]
    n = norms(cb)
    T = np.empty((Q, M, 256), F)
    with np.errstate(all="ignore"):
        for m in range(M):
            v = _dots(q, cb, m)
            T[:, m] = (n[m][None, :] - F(2) * v) if metric == "l2" else -v
        lo, hi = T.min(2), T.max(2)
        R = np.zeros(Q, F)
        for m in range(M):
            R = R + (hi[:, m] - lo[:, m])
        delta = R / F(8000.0)
        assert R.dtype == F and delta.dtype == F
        u = np.rint((T - lo[:, :, None]) / delta[:, None, None])
    zero = ~np.isfinite(T).all((1, 2)) | ~np.isfinite(R) | (R == 0)
    u[zero] = 0
    u = u.astype(np.uint16)
    assert (u.max(2).astype(np.int64).sum(1) < BINS).all()
    return u


def keys(u_q, cx):
    """h [n]: the sum over m of u_q[m][cx[row][m]]"""
    return u_q[np.arange(u_q.shape[0])[None, :], cx].astype(np.int64).sum(1)


def case(q, vecs, ids, offsets, pids, k, fetch_k, metric, cb, want_cut=False):
    """expected (ids [Q, k], dist [Q, k]) over the lists pids [Q, P] of the CSR (vecs, ids, offsets); want_cut: also, per query, how
    many probed rows share the key of the fetch_k-th place (0: fewer probed rows than fetch_k)"""
    q, vecs, ids = np.ascontiguousarray(q, F), np.ascontiguousarray(vecs, F), np.asarray(ids, np.int64)
    cb = np.ascontiguousarray(cb, F)
    cx, u = codes(vecs, cb), table(q, cb, metric)
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, F)
    at_cut = np.zeros(Q, np.int64)
    for qi in range(Q):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[qi] if p >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
        if rows.shape[0] == 0:
            continue
        h = keys(u[qi], cx[rows])
        if rows.shape[0] >= fetch_k:
            at_cut[qi] = (h == np.sort(h)[fetch_k - 1]).sum()
        rows = rows[np.lexsort((rows, h))[:fetch_k]]
        v = O.pair_values(q[qi:qi + 1], vecs[rows], metric)[0]
        keep = ~np.isnan(v)
        v, rid = v[keep], ids[rows][keep]
        best = sorted(range(v.shape[0]), key=lambda i: (float(-v[i]) if metric == "ip" else float(v[i]), int(rid[i])))[:k]
        out_i[qi, :len(best)] = rid[best]
        with np.errstate(invalid="ignore"):
            out_d[qi, :len(best)] = (v[best] + F(0.0)) if metric == "ip" else np.sqrt(v[best])
    return (out_i, out_d, at_cut) if want_cut else (out_i, out_d)
