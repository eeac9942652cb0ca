"""The yardstick of adaptive probing under a filter (qk_search_filtered_adaptive; shared by tests/test_adaptive_oracle.py and
tests/test_adaptive_search.py).  It is the definition of include/quake_hip.h written out, one query at a time:

  M = min(max_nprobe, lists), n0 = min(nprobe, M); r_1 .. r_M the oracle's coarse ranking at M (-1 padding = a list of 0 rows);
  c(p) = candidate rows of list p under the query's filter; nprobed = the smallest t in [n0, M] whose first t lists hold
  min_candidates candidates, M if none does; the row = the oracle's batched_serial_scan of the reduced CSR over r_1 .. r_nprobed.

Nothing here knows about masks, counts, tiles or kernels.  A filter is (S, mode) as in tests/filter_yardstick.py, or a bool array
over the CSR rows (a predicate evaluated by tests/attr_yardstick.py)."""
import numpy as np

import filter_yardstick as Y
import oracle as O


def keep_of(flt, ids):
    """bool per CSR row: is it a candidate of the filter"""
    if isinstance(flt, np.ndarray) and flt.dtype == np.bool_:
        assert flt.shape[0] == ids.shape[0]
        return flt
    S, mode = flt
    return Y.allowed_rows(ids, S, mode)


def list_counts(keep, offsets):
    """candidates per list"""
    csum = np.zeros(keep.shape[0] + 1, np.int64)
    csum[1:] = np.cumsum(keep)
    offsets = np.asarray(offsets, np.int64)
    return csum[offsets[1:]] - csum[offsets[:-1]]


def nprobed_of(rank_row, counts, n0, min_candidates):
    """the definition: rank_row [M] list numbers (-1 = 0 rows)"""
    M = rank_row.shape[0]
    total = 0
    for t in range(1, M + 1):
        p = int(rank_row[t - 1])
        total += int(counts[p]) if p >= 0 else 0
        if t >= n0 and total >= min_candidates:
            return t
    return M


def pad_of(metric):
    return np.float32(np.inf) if metric == "l2" else np.float32(-np.inf)


def search(q, centroids, vecs, ids, offsets, nprobe, max_nprobe, min_candidates, k, metric, filters, qf=None, centroid_ids=None):
    """(ids [Q, k], dist [Q, k], nprobed int32 [Q], probed int64 [Q, M]); query i under filters[qf[i]] (qf None: filters[0]); a qf
    value outside [0, len(filters)) gives nprobed 0, an all -1 probed row and a padded result"""
    q = np.ascontiguousarray(q, np.float32)
    Q = q.shape[0]
    nlist = centroids.shape[0]
    M = min(int(max_nprobe), nlist)
    n0 = min(int(nprobe), M)
    rank, _ = O.coarse(q, centroids, centroid_ids, M, metric, num_threads=8)
    assert rank.shape == (Q, M)
    reduced, counts = {}, {}
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), pad_of(metric), np.float32)
    nprobed = np.zeros(Q, np.int32)
    probed = np.full((Q, M), -1, np.int64)
    for i in range(Q):
        f = 0 if qf is None else int(qf[i])
        if not 0 <= f < len(filters):
            continue
        if f not in reduced:
            keep = keep_of(filters[f], ids)
            reduced[f] = Y.reduced_csr(vecs, ids, offsets, keep)
            counts[f] = list_counts(keep, offsets)
        t = nprobed_of(rank[i], counts[f], n0, min_candidates)
        nprobed[i] = t
        probed[i, :t] = rank[i, :t]
        pref = rank[i, :t]
        pref = pref[pref >= 0]  # (padding of the ranking: a list of 0 rows)
        if pref.shape[0] == 0:
            continue
        fv, fi, fo = reduced[f]
        out_i[i], out_d[i] = O.batched_serial_scan(q[i:i + 1], fv, fi, fo, np.ascontiguousarray(pref[None, :]), k, metric)
    return out_i, out_d, nprobed, probed
