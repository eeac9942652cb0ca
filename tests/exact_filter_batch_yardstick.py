"""The yardstick of exact filtered search with one filter per query (shared by tests/test_exact_filter_batch_oracle.py,
tests/test_exact_filter_batch_search.py and tests/test_exact_filter_batch_random.py).

Query i is answered by the single-filter yardstick (tests/exact_filter_yardstick.py) under filter qfilter[i]; a qfilter value
outside [0, F) gives an all-padding row.  pool_scan() is the other side of the contract of qk_search_filtered_exact_batch -- the
kept rows of filter j as list j of ONE CSR, in stored order, and every query scanning the one list of its filter -- and
tests/test_exact_filter_batch_oracle.py pins that the two agree bit for bit.  Nothing here knows about masks, tiles or kernels."""
import numpy as np

import exact_filter_yardstick as E
import filter_yardstick as Y
import oracle as O


def search(q, vecs, ids, offsets, k, metric, specs, qfilter):
    """specs: [(S, mode)] per filter; qfilter int [Q]"""
    qfilter = np.asarray(qfilter)
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), np.inf if metric == "l2" else -np.inf, np.float32)
    for j, (S, mode) in enumerate(specs):
        rows = np.nonzero(qfilter == j)[0]
        if rows.shape[0]:
            out_i[rows], out_d[rows] = E.search(np.ascontiguousarray(q[rows]), vecs, ids, offsets, k, metric, S, mode)
    return out_i, out_d


def pool_csr(vecs, ids, specs):
    """list j = the kept rows of filter j in stored order"""
    keeps = [Y.allowed_rows(ids, S, mode) for S, mode in specs]
    offsets = np.zeros(len(specs) + 1, np.int64)
    offsets[1:] = np.cumsum([int(kp.sum()) for kp in keeps])
    pv = np.ascontiguousarray(np.concatenate([vecs[kp] for kp in keeps])) if keeps else vecs[:0]
    pi = np.ascontiguousarray(np.concatenate([ids[kp] for kp in keeps])) if keeps else ids[:0]
    return pv, pi, offsets


def pool_scan(q, vecs, ids, k, metric, specs, qfilter):
    pv, pi, offsets = pool_csr(vecs, ids, specs)
    qfilter = np.asarray(qfilter).astype(np.int64)
    pids = np.where((qfilter >= 0) & (qfilter < len(specs)), qfilter, -1).reshape(-1, 1)
    return O.batched_serial_scan(q, pv, pi, offsets, np.ascontiguousarray(pids), k, metric)


def candidates(ids, specs):
    return [E.candidates(ids, S, mode) for S, mode in specs]
