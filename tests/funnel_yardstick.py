"""The yardstick of funnel search (tests/test_funnel_search.py; the definition: include/quake_hip.h, "funnel search"),
from the oracle alone.  O.batched_serial_scan over the CSR of x[:, :d'] with k = fetch_k gives a query's candidates -- the rows are
named by their position in the CSR, so that a row stored twice and bit-equal rows stay apart --, the oracle's full-d values of those
rows, sorted by (key, id), give the answer."""
import numpy as np

import oracle as O


def case(q, vecs, ids, offsets, pids, k, fetch_k, dp, metric):
    """expected (ids [Q, k], dist [Q, k]) of a funnel search over the lists pids [Q, P] of the CSR (vecs, ids, offsets).  Asserts the
    condition on the inputs that makes the candidate SET unique: the fetch_k-th and the next prefix key of every query differ."""
    q = np.ascontiguousarray(q, np.float32)
    vecs = np.ascontiguousarray(vecs, np.float32)
    ids = np.asarray(ids, np.int64)
    rows_of = np.arange(vecs.shape[0], dtype=np.int64)
    ci, cd = O.batched_serial_scan(np.ascontiguousarray(q[:, :dp]), np.ascontiguousarray(vecs[:, :dp]), rows_of, offsets,
                                   np.ascontiguousarray(pids, np.int64), fetch_k + 1, metric)
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, np.float32)
    for qi in range(Q):
        if ci[qi, fetch_k] >= 0:
            assert cd[qi, fetch_k - 1] != cd[qi, fetch_k], "the fetch_k-th and the next prefix key must differ (query %d)" % qi
        rows = ci[qi, :fetch_k]
        rows = rows[rows >= 0]
        if rows.shape[0] == 0:
            continue
        v = O.pair_values(q[qi:qi + 1], vecs[rows], metric)[0]
        keep = ~np.isnan(v)
        v, rid = v[keep], ids[rows][keep]
        order = sorted(range(v.shape[0]), key=lambda i: (float(-v[i]) if metric == "ip" else float(v[i]), int(rid[i])))[:k]
        n = len(order)
        out_i[qi, :n] = rid[order]
        with np.errstate(invalid="ignore"):
            out_d[qi, :n] = (v[order] + np.float32(0.0)) if metric == "ip" else np.sqrt(v[order])
    return out_i, out_d
