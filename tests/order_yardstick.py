"""Yardstick of ordered search (include/quake_hip.h, "ordered search"): per query, the k first range hits by an attribute column.

The definition, in Python: take a query's candidates in the search order (key ascending, then id ascending -- paging_yardstick's
`ordering`), keep those that pass the radius (range_yardstick.passes on the reported float32 distance), look the column up
(attr_yardstick._lookup) and sort the hits that have a value by it with a STABLE sort -- ascending or descending -- so that equal
values stay in (key, id) order.  Hits without a value are left out, or, with missing_last, follow in (key, id) order.  The first k
are the answer.  Nothing here knows how the library finds them."""
import numpy as np

import attr_yardstick as AY
import oracle as O
import paging_yardstick as PY
import range_yardstick as RY

NAMES = ("ids", "dist", "values", "count", "missing", "total")


def _first_k(ids, dist, column_dict, k, descending, missing_last):
    """ids / dist: one query's hits in (key, id) order -> (ids, dist, values of the first k entries, count, missing)"""
    has, vals = AY._lookup(ids, column_dict)
    has, value_of = np.asarray(has, bool), np.asarray(vals, np.int64).tolist()              # (Python ints)
    with_value = sorted(np.nonzero(has)[0].tolist(), key=value_of.__getitem__, reverse=bool(descending))   # (stable, also when reversed)
    without = np.nonzero(~has)[0].tolist()
    take = np.array((with_value + (without if missing_last else []))[:k], np.int64)
    return (np.asarray(ids, np.int64)[take], np.asarray(dist, np.float32)[take],
            np.where(has[take], np.asarray(vals, np.int64)[take], 0).astype(np.int64), len(with_value), len(without))


def _pack(per_query, k, metric):
    Q = len(per_query)
    ids = np.full((Q, k), -1, np.int64)
    dist = np.full((Q, k), -np.inf if metric == "ip" else np.inf, np.float32)
    values = np.zeros((Q, k), np.int64)
    count, missing = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    for q, (i, d, v, c, m) in enumerate(per_query):
        ids[q, :len(i)], dist[q, :len(i)], values[q, :len(i)] = i, d, v
        count[q], missing[q] = c, m
    return ids, dist, values, count, missing, count + missing


def expected(order, radius, column_dict, k, descending=False, missing_last=False):
    """(ids [Q, k], dist [Q, k], values [Q, k], count [Q], missing [Q], total [Q]) from paging_yardstick.ordering's Order"""
    per = []
    for q in range(len(order)):
        keep = RY.passes(order.dist[q], radius, order.metric)
        per.append(_first_k(order.ids[q][keep], order.dist[q][keep], column_dict, k, descending, missing_last))
    return _pack(per, k, order.metric)


def expected_pairs(q, vecs, ids, pairs, radius, metric, column_dict, k, descending=False, missing_last=False):
    """the same from range_yardstick.all_pairs' (lims, rows, dist): the multiset of (query, probed row) pairs, for a store that holds
    a row twice (`ordering` assumes distinct ids).  The (key, id) order comes from the keys of the oracle's pair values"""
    lims, rows, dist = pairs
    ids = np.asarray(ids, np.int64)
    per = []
    for i in range(q.shape[0]):
        r, d = rows[lims[i]:lims[i + 1]], dist[lims[i]:lims[i + 1]]
        val = O.pair_values(q[i:i + 1], vecs[r], metric)[0] if r.shape[0] else np.zeros(0, np.float32)
        key = PY.key_of(val, metric)
        keep = RY.passes(d, radius, metric) & (key != 0xFFFFFFFF)
        hid, hd, hk = ids[r][keep], d[keep], key[keep]
        o = np.lexsort((hid, hk))
        per.append(_first_k(hid[o], hd[o], column_dict, k, descending, missing_last))
    return _pack(per, k, metric)
