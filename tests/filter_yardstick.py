"""The yardstick of filtered search (shared by tests/test_filtered_oracle.py and tests/test_filtered_search.py).

A filtered search over a store X equals the existing search over a store that holds the same lists with the disallowed rows
taken out, probed with the same list numbers: expected values are the oracle's search / batched_serial_scan (the canonical arithmetic) over that reduced CSR (same
centroids, same list numbers, offsets recomputed).  Nothing here knows about masks, tiles or kernels."""
import numpy as np

import oracle as O


def allowed_rows(ids, S, mode):
    """bool per CSR row: is it a candidate under the id set S and the mode ('allow' / 'deny')"""
    inS = np.isin(ids, np.asarray(S, dtype=np.int64))
    return inS if mode == "allow" else ~inS


def reduced_csr(vecs, ids, offsets, keep):
    """the CSR with the rows where keep is False deleted: same lists, offsets recomputed"""
    offsets = np.asarray(offsets, np.int64)
    nlist = offsets.shape[0] - 1
    csum = np.zeros(keep.shape[0] + 1, np.int64)
    csum[1:] = np.cumsum(keep)
    new_off = csum[offsets]
    assert new_off.shape[0] == nlist + 1
    return np.ascontiguousarray(vecs[keep]), np.ascontiguousarray(ids[keep]), new_off


def search(q, centroids, vecs, ids, offsets, nprobe, k, metric, S, mode, centroid_ids=None):
    keep = allowed_rows(ids, S, mode)
    fv, fi, fo = reduced_csr(vecs, ids, offsets, keep)
    return O.search(q, centroids, fv, fi, fo, nprobe, k, metric, batched_scan=True, num_threads=8, centroid_ids=centroid_ids)


def scan(q, vecs, ids, offsets, pids, k, metric, S, mode):
    keep = allowed_rows(ids, S, mode)
    fv, fi, fo = reduced_csr(vecs, ids, offsets, keep)
    return O.batched_serial_scan(q, fv, fi, fo, pids, k, metric)


def draw_set(all_ids, selectivity, rng):
    """ids drawn uniformly: a fraction `selectivity` of all_ids (at least one id unless the fraction is 0)"""
    n = all_ids.shape[0]
    m = 0 if selectivity <= 0 else n if selectivity >= 1 else max(1, int(round(selectivity * n)))
    return np.ascontiguousarray(rng.permutation(all_ids)[:m])
