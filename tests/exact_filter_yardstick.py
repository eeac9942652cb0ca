"""The yardstick of exact filtered search (shared by tests/test_exact_filter_oracle.py, tests/test_exact_filter_search.py and
tests/test_exact_filter_random.py).

The exact answer under a filter is the filter yardstick (tests/filter_yardstick.py) with EVERY list in every query's pids: the
oracle's batched scan over the CSR with the disallowed rows deleted.  one_list() is the other side of the contract of
qk_search_filtered_exact -- the kept rows as ONE list, in stored order -- and tests/test_exact_filter_oracle.py pins that the two
agree bit for bit.  Nothing here knows about masks, tiles or kernels."""
import numpy as np

import filter_yardstick as Y
import oracle as O


def all_pids(nq, nlist):
    return np.ascontiguousarray(np.tile(np.arange(nlist, dtype=np.int64), (nq, 1)))


def search(q, vecs, ids, offsets, k, metric, S, mode):
    """the k best candidates of (S, mode) over the whole CSR"""
    nlist = np.asarray(offsets).shape[0] - 1
    return Y.scan(q, vecs, ids, offsets, all_pids(q.shape[0], nlist), k, metric, S, mode)


def one_list(q, vecs, ids, k, metric, S, mode):
    """the same rows as ONE list in stored order"""
    keep = Y.allowed_rows(ids, S, mode)
    fv, fi = np.ascontiguousarray(vecs[keep]), np.ascontiguousarray(ids[keep])
    return O.batched_serial_scan(q, fv, fi, np.array([0, fi.shape[0]], np.int64), np.zeros((q.shape[0], 1), np.int64), k, metric)


def candidates(ids, S, mode):
    return int(Y.allowed_rows(ids, S, mode).sum())


def recall(got_ids, want_ids):
    """mean over the queries of |got & want| / |want| (padding excluded; a query without expected ids counts as 1)"""
    r = []
    for g, w in zip(np.asarray(got_ids), np.asarray(want_ids)):
        w = w[w >= 0]
        r.append(1.0 if w.shape[0] == 0 else np.isin(w, g[g >= 0]).mean())
    return float(np.mean(r))
