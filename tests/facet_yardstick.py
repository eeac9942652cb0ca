"""The yardstick of facet counts (shared by tests/test_facet_oracle.py, tests/test_facet_search.py and tests/test_facet_random.py).

A column is a Python dict id -> int.  expected() counts the values of a column over each query's hit ids in plain numpy; the hits
come from tests/range_yardstick.py -- the oracle-based expectation range search is pinned to -- and a filter is applied the way
that yardstick applies it, the allowed id set coming from filter_yardstick / attr_yardstick / expr_yardstick.  Nothing here knows
about keys, tables, slots or kernels."""
import numpy as np

import attr_yardstick as AY
import range_yardstick as RY


def expected(hit_ids_per_query, column_dict, n_values):
    """(values [Q, n], counts [Q, n], distinct [Q], missing [Q], total [Q]) of ONE column: per query the n_values values with the
    most hits, ordered by (-count, value) with the value compared as a signed integer, padded with value 0 / count 0"""
    Q = len(hit_ids_per_query)
    values = np.zeros((Q, n_values), np.int64)
    counts = np.zeros((Q, n_values), np.int64)
    distinct = np.zeros(Q, np.int64)
    missing = np.zeros(Q, np.int64)
    total = np.zeros(Q, np.int64)
    for q, hit in enumerate(hit_ids_per_query):
        hit = np.asarray(hit, np.int64).reshape(-1)
        total[q] = hit.shape[0]
        has, v = AY._lookup(hit, column_dict)
        missing[q] = int((~has).sum())
        uv, uc = np.unique(v[has], return_counts=True)
        distinct[q] = uv.shape[0]
        order = np.lexsort((uv, -uc))[:n_values]    # last key first: by -count, ties by the signed value
        values[q, :order.shape[0]] = uv[order]
        counts[q, :order.shape[0]] = uc[order]
    return values, counts, distinct, missing, total


def expected_cols(hit_ids_per_query, column_dicts, n_values):
    """the same for a list of columns: (values [C, Q, n], counts [C, Q, n], distinct [C, Q], missing [C, Q], total [Q])"""
    per = [expected(hit_ids_per_query, col, n_values) for col in column_dicts]
    return (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]),
            np.stack([p[3] for p in per]), per[0][4])


def split(lims, ids):
    """a range result as a list of per-query id arrays"""
    lims = np.asarray(lims, np.int64)
    return [np.asarray(ids, np.int64)[lims[q]:lims[q + 1]] for q in range(lims.shape[0] - 1)]


def hits_search(q, centroids, vecs, ids, offsets, nprobe, radius, metric, allowed=None):
    """per-query hit ids of range_search; allowed: the id set of a filter (None: no filter)"""
    lims, hid, _ = RY.search(q, centroids, vecs, ids, offsets, nprobe, radius, metric,
                             S=None if allowed is None else np.asarray(allowed, np.int64), mode="allow")
    return split(lims, hid)


def hits_scan(q, vecs, ids, offsets, pids, radius, metric, allowed=None):
    """per-query hit ids of range_scan over the pids rows"""
    lims, hid, _ = RY.scan(q, vecs, ids, offsets, pids, radius, metric, S=None if allowed is None else np.asarray(allowed, np.int64),
                           mode="allow")
    return split(lims, hid)


def allowed_ids(ids, keep):
    """the id set of a filter from a bool per CSR row (filter_yardstick.allowed_rows, attr_yardstick.eval_where,
    expr_yardstick.eval_any_of)"""
    return AY.allowed_set(np.asarray(keep, bool), ids)
