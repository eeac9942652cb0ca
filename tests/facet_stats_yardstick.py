"""The yardstick of facet statistics (shared by tests/test_facet_stats_oracle.py, tests/test_facet_stats_search.py and
tests/test_facet_stats_random.py).

A column is a Python dict id -> int.  expected() reduces the values of a column over each query's hit ids in plain numpy and Python
integers; the hits come from tests/facet_yardstick.py (hits_search / hits_scan), that is from tests/range_yardstick.py.  Nothing
here knows about keys, slices, accumulators or kernels."""
import numpy as np

import attr_yardstick as AY

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
NAMES = ("count", "missing", "min", "max", "sum_lo", "sum_hi", "hist", "total")


def split128(x):
    """a Python int inside [-2^127, 2^127) as its two's-complement words (hi, lo): hi the signed high 64 bits, lo the low 64 bits
    read as a SIGNED int64 (the way out_sum_lo stores them)"""
    x = int(x)
    assert -(1 << 127) <= x < (1 << 127)
    u = x % (1 << 128)
    hi, lo = u >> 64, u & ((1 << 64) - 1)
    return (hi - (1 << 64) if hi >= (1 << 63) else hi), (lo - (1 << 64) if lo >= (1 << 63) else lo)


def join128(hi, lo):
    """the inverse of split128"""
    return int(hi) * (1 << 64) + (int(lo) % (1 << 64))


def expected(hit_ids_per_query, column_dict, edges):
    """(count [Q], missing [Q], min [Q], max [Q], sums: a list of Q Python ints, hist [Q, len(edges) + 1], total [Q]) of ONE column;
    edges: a strictly ascending list of ints (may be empty)"""
    Q = len(hit_ids_per_query)
    e = np.array(list(edges), np.int64)
    count, missing, total = np.zeros(Q, np.int64), np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    vmin, vmax = np.full(Q, I64MAX, np.int64), np.full(Q, I64MIN, np.int64)
    hist = np.zeros((Q, e.shape[0] + 1), np.int64)
    sums = []
    for q, hit in enumerate(hit_ids_per_query):
        hit = np.asarray(hit, np.int64).reshape(-1)
        total[q] = hit.shape[0]
        has, v = AY._lookup(hit, column_dict)
        v = v[has]
        count[q] = v.shape[0]
        missing[q] = total[q] - count[q]
        if v.shape[0]:
            vmin[q], vmax[q] = v.min(), v.max()
        sums.append(sum(int(x) for x in v))
        hist[q] = np.bincount(np.searchsorted(e, v, side="right"), minlength=e.shape[0] + 1)
    return count, missing, vmin, vmax, sums, hist, total


def expected_cols(hit_ids_per_query, column_dicts, edges_per_column):
    """the same for a list of columns, in the shape of the call's outputs: (count, missing, min, max, sum_lo, sum_hi [C, Q],
    hist [C, Q, 1 + the most edges of a column] padded with 0, total [Q]) and, last, the sums as [C][Q] Python ints"""
    per = [expected(hit_ids_per_query, col, e) for col, e in zip(column_dicts, edges_per_column)]
    Q = len(hit_ids_per_query)
    hs = 1 + max(len(e) for e in edges_per_column)
    hist = np.zeros((len(per), Q, hs), np.int64)
    for c, p in enumerate(per):
        hist[c, :, :p[5].shape[1]] = p[5]
    words = [[split128(s) for s in p[4]] for p in per]
    lo = np.array([[w[1] for w in row] for row in words], np.int64).reshape(len(per), Q)
    hi = np.array([[w[0] for w in row] for row in words], np.int64).reshape(len(per), Q)
    return (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), np.stack([p[3] for p in per]),
            lo, hi, hist, per[0][6], [p[4] for p in per])
