"""The yardstick of quantized search (tests/test_sq8_search.py; the definition: include/quake_hip.h, "quantized search", DESIGN.md
5.23) in numpy: code parameters and codes in float32 (np.rint rounds half to even, float32 / is the IEEE division), keys in int64,
candidates by np.lexsort on (key, row), exact keys and the final order through the oracle as tests/funnel_yardstick.py does it.
The input is the CSR in arena order: rows are named by their position in it."""
import numpy as np

import oracle as O

F = np.float32


def params(vecs, metric):
    """(m [d], s) of a store whose live rows are vecs"""
    d = vecs.shape[1]
    if vecs.shape[0] == 0:
        return np.zeros(d, F), F(1)
    if metric == "ip":
        m, s = np.zeros(d, F), np.abs(vecs).max() / F(127)
    else:
        lo, hi = vecs.min(0), vecs.max(0)
        m, s = F(0.5) * lo + F(0.5) * hi, (hi - lo).max() / F(254)
    assert np.isfinite(vecs).all() and np.isfinite(s) and m.dtype == F and s.dtype == F
    return m, (F(1) if s == 0 else s)


def codes(x, m, s):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.rint((x - m) / s), -127, 127)
    return np.where(np.isnan(x), 0, c).astype(np.int64)


def query_codes(q, m, s, metric):
    if metric != "ip":
        return codes(q, m, s)
    a = np.where(np.isfinite(q), np.abs(q), F(0)).max(1, keepdims=True) / F(127)
    return codes(q, F(0), np.where(a == 0, F(1), a).astype(F))


def keys(cq, cx, metric):
    """the approximate keys of one query's codes against the rows' codes"""
    return -(cx @ cq) if metric == "ip" else ((cx - cq) ** 2).sum(1)


def case(q, vecs, ids, offsets, pids, k, fetch_k, metric, cut_in_one_list=False):
    """expected (ids [Q, k], dist [Q, k]) over the lists pids [Q, P] of the CSR (vecs, ids, offsets).  cut_in_one_list: assert that
    the rows that share the key of the fetch_k-th place lie in one list (a store whose lists have moved keeps arena order only
    inside a list)."""
    q, vecs, ids = np.ascontiguousarray(q, F), np.ascontiguousarray(vecs, F), np.asarray(ids, np.int64)
    m, s = params(vecs, metric)
    cx, cq = codes(vecs, m, s), query_codes(q, m, s, metric)
    list_of = np.repeat(np.arange(offsets.shape[0] - 1), np.diff(offsets))
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, F)
    for qi in range(Q):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[qi] if p >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
        if rows.shape[0] == 0:
            continue
        key = keys(cq[qi], cx[rows], metric)
        order = np.lexsort((rows, key))
        if cut_in_one_list and rows.shape[0] > fetch_k and key[order[fetch_k - 1]] == key[order[fetch_k]]:
            assert np.unique(list_of[rows[key == key[order[fetch_k]]]]).shape[0] == 1, "equal keys at the cut in two lists (query %d)" % qi
        rows = rows[order[:fetch_k]]
        v = O.pair_values(q[qi:qi + 1], vecs[rows], metric)[0]
        keep = ~np.isnan(v)
        v, rid = v[keep], ids[rows][keep]
        best = sorted(range(v.shape[0]), key=lambda i: (float(-v[i]) if metric == "ip" else float(v[i]), int(rid[i])))[:k]
        out_i[qi, :len(best)] = rid[best]
        with np.errstate(invalid="ignore"):
            out_d[qi, :len(best)] = (v[best] + F(0.0)) if metric == "ip" else np.sqrt(v[best])
    return out_i, out_d
