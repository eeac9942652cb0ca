"""The yardstick of binary search (tests/test_bin_search.py; the definition: include/quake_hip.h, "binary search")
in numpy: centres in float32, bits by an ordered float32 comparison, keys as counts of differing bits, candidates by np.lexsort on
(key, row), exact keys and the final order through the oracle as tests/sq8_yardstick.py does it.  The input is the CSR in arena
order: rows are named by their position in it."""
import numpy as np

import oracle as O

F = np.float32


def params(vecs, metric):
    """m [d] of a store whose live rows are vecs: quantized search's L2 centre, 0 for the inner product"""
    d = vecs.shape[1]
    if metric == "ip" or vecs.shape[0] == 0:
        return np.zeros(d, F)
    assert np.isfinite(vecs).all()
    m = F(0.5) * vecs.min(0) + F(0.5) * vecs.max(0)
    assert m.dtype == F
    return m


def codes(x, m):
    with np.errstate(invalid="ignore"):
        return np.asarray(x, F) > m  # (ordered: False for NaN, and for -0 and +0 against the centre 0)


def keys(bq, bx):
    """the Hamming distances of one query's bits to the rows' bits"""
    return (bx != bq).sum(1).astype(np.int64)


def case(q, vecs, ids, offsets, pids, k, fetch_k, metric):
    """expected (ids [Q, k], dist [Q, k]) over the lists pids [Q, P] of the CSR (vecs, ids, offsets)"""
    q, vecs, ids = np.ascontiguousarray(q, F), np.ascontiguousarray(vecs, F), np.asarray(ids, np.int64)
    m = params(vecs, metric)
    bx, bq = codes(vecs, m), codes(q, m)
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, F)
    for qi in range(Q):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[qi] if p >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
        if rows.shape[0] == 0:
            continue
        rows = rows[np.lexsort((rows, keys(bq[qi], bx[rows])))[:fetch_k]]
        v = O.pair_values(q[qi:qi + 1], vecs[rows], metric)[0]
        keep = ~np.isnan(v)
        v, rid = v[keep], ids[rows][keep]
        best = sorted(range(v.shape[0]), key=lambda i: (float(-v[i]) if metric == "ip" else float(v[i]), int(rid[i])))[:k]
        out_i[qi, :len(best)] = rid[best]
        with np.errstate(invalid="ignore"):
            out_d[qi, :len(best)] = (v[best] + F(0.0)) if metric == "ip" else np.sqrt(v[best])
    return out_i, out_d
