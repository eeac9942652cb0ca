"""Yardstick of multi-vector search (include/quake_hip.h, "multi-vector search"): sum-of-MaxSim document scores.

The definition, in numpy: a logical query l is T sub-queries.  Every (sub-query, probed row) pair comes from the oracle as it is
(grouped_yardstick.candidates: O.pair_values in stored row order); a pair is a hit when its reported float32 distance passes the
radius (range_yardstick.passes; a NaN never does), a filter is applied by deleting the other rows from the CSR first
(filter_yardstick).  A hit whose id has a value g in the column is a candidate of (l, t, g); the term of (l, t, g) is the best
reported distance among them -- smallest for L2, largest for the inner product, both zeros being +0 -- or `missing` without one.
The score of g is +0 plus the terms of t = 0 .. n_tokens[l] - 1, added one after the other in float32.  The k best values -- the
better score first, NaN behind every number, ties to the smaller value -- are the answer.  Nothing here knows about keys, tables or
kernels."""
import numpy as np

import filter_yardstick as FY
import grouped_yardstick as GY
import range_yardstick as RY

NAMES = ("groups", "scores", "matched", "n_groups", "hits")
CANONICAL_NAN = np.uint32(0x7FC00000)


def _terms(dist, groups, metric):
    """the best reported distance per distinct value: (values ascending, best float32)"""
    uniq, inv = np.unique(groups, return_inverse=True)
    if metric == "l2":
        best = np.full(uniq.shape[0], np.inf, np.float32)
        np.minimum.at(best, inv, dist)
    else:
        best = np.full(uniq.shape[0], -np.inf, np.float32)
        np.maximum.at(best, inv, dist)
    return uniq, (best + np.float32(0.0)).astype(np.float32)   # (-0 + 0 == +0: both zeros are one value)


def reduce(cand, T, rowval, rowhas, k, metric, radius, n_tokens=None, missing=0.0, squared=False):
    """(groups [L, k], scores [L, k], matched [L, k] int32, n_groups [L], hits [L, T]) from grouped_yardstick.candidates() over
    the L * T sub-queries"""
    lims, rows, val = cand
    L = (lims.shape[0] - 1) // T
    inf = np.float32(-np.inf if metric == "ip" else np.inf)
    if radius is None:
        radius = inf
    out_g = np.zeros((L, k), np.int64)
    out_s = np.full((L, k), inf, np.float32)
    out_m = np.zeros((L, k), np.int32)
    out_n = np.zeros(L, np.int64)
    out_h = np.zeros((L, T), np.int64)
    miss = np.float32(missing)
    for l in range(L):
        nt = T if n_tokens is None else int(n_tokens[l])
        per_t = []
        for t in range(nt):
            a, b = lims[l * T + t], lims[l * T + t + 1]
            r, v = rows[a:b], val[a:b]
            with np.errstate(invalid="ignore"):
                dist = np.sqrt(v) if (metric == "l2" and not squared) else v
            hit = RY.passes(dist, radius, metric)
            out_h[l, t] = int(hit.sum())
            c = hit & rowhas[r]
            per_t.append(_terms(dist[c], rowval[r[c]], metric))
        values = np.unique(np.concatenate([u for u, _ in per_t] + [np.zeros(0, np.int64)]))
        out_n[l] = values.shape[0]
        if values.shape[0] == 0:
            continue
        score = np.zeros(values.shape[0], np.float32)
        matched = np.zeros(values.shape[0], np.int32)
        with np.errstate(invalid="ignore"):
            for u, best in per_t:   # one float32 addition per term, in token order
                term = np.full(values.shape[0], miss, np.float32)
                at = np.searchsorted(values, u)
                term[at] = best
                matched[at] += 1
                score = (score + term).astype(np.float32)
        nan = np.isnan(score)
        key = np.where(nan, np.float32(0.0), -score if metric == "ip" else score)
        order = np.lexsort((values, key, nan))[:k]
        n = order.shape[0]
        out_g[l, :n], out_s[l, :n], out_m[l, :n] = values[order], score[order], matched[order]
    return out_g, out_s, out_m, out_n, out_h


def scan(q3, vecs, ids, offsets, pids, k, metric, attr_ids, attr_vals, radius=None, n_tokens=None, missing=0.0, S=None, mode="allow",
         keep=None, squared=False):
    """maxsim_scan's expected outputs: q3 [L, T, d], pids [L * T, P] (or [P]); S / mode (an id set) or keep (bool per row): a filter"""
    q3 = np.ascontiguousarray(q3, np.float32)
    L, T, d = q3.shape
    if S is not None:
        keep = FY.allowed_rows(ids, S, mode)
    if keep is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, keep)
    rowval, rowhas = GY.row_values(ids, attr_ids, attr_vals)
    cand = GY.candidates(q3.reshape(L * T, d), vecs, ids, offsets, pids, metric)
    return reduce(cand, T, rowval, rowhas, k, metric, radius, n_tokens, missing, squared)


def search(q3, centroids, vecs, ids, offsets, nprobe, k, metric, attr_ids, attr_vals, **kw):
    """maxsim_search's expected outputs: the lists O.coarse ranks for every sub-query (None: every list)"""
    q3 = np.ascontiguousarray(q3, np.float32)
    pids = GY.probed(q3.reshape(-1, q3.shape[2]), centroids, offsets, nprobe, metric)
    return scan(q3, vecs, ids, offsets, pids, k, metric, attr_ids, attr_vals, **kw)


def bits(out):
    """the outputs as integer arrays for a bit-for-bit comparison; a NaN score counts as the canonical quiet NaN the library reports"""
    g, s, m, n, h = (np.asarray(o) for o in out[:5])
    sb = np.ascontiguousarray(s, np.float32).view(np.uint32).copy()
    sb[np.isnan(s)] = CANONICAL_NAN
    return g.astype(np.int64), sb, m.astype(np.int32), n.astype(np.int64), h.astype(np.int64)


def assert_equal(got, want, what=""):
    for name, a, b in zip(NAMES, bits(got), bits(want)):
        assert a.shape == b.shape, "%s %s: shape %s != %s" % (what, name, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[0]
            raise AssertionError("%s %s differs at %s: got %s want %s (%d entries differ)" % (what, name, tuple(bad), a[tuple(bad)], b[tuple(bad)],
                                                                                      int((a != b).sum())))
