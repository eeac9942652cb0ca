"""The yardstick of attribute filters (shared by tests/test_attr_filter_host.py and tests/test_attr_filter.py).

A column is a Python dict id -> int.  A clause list is evaluated over (ids, columns) in plain numpy / Python integers -- nothing
here knows about layouts, masks, tiles or kernels -- which gives the allowed id set; the search over that set is
tests/filter_yardstick.py's: the oracle's search over the CSR with the other rows deleted.

Two clause forms are evaluated, independently of each other and of quake_amd/where.py:
  eval_clauses  the C ABI's (name, QK_OP_*, a, b) over int64
  eval_where    the mirrors' (name, op, a[, b]) over the integers (operands of any size)"""
import numpy as np

import filter_yardstick as Y

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
QK_OP_RANGE, QK_OP_NOT_RANGE, QK_OP_ANY_BITS, QK_OP_ALL_BITS, QK_OP_NO_BITS = 0, 1, 2, 3, 4
OP_CODES = {"range": 0, "not_range": 1, "any_bits": 2, "all_bits": 3, "no_bits": 4}


def _lookup(ids, col):
    """(has bool [n], values int64 [n]) of the ids in the dict `col`"""
    ids = np.asarray(ids, np.int64)
    if not col:
        return np.zeros(ids.shape[0], bool), np.zeros(ids.shape[0], np.int64)
    keys = np.fromiter(col.keys(), np.int64, len(col))
    vals = np.fromiter(col.values(), np.int64, len(col))
    o = np.argsort(keys)
    keys, vals = keys[o], vals[o]
    pos = np.minimum(np.searchsorted(keys, ids), keys.shape[0] - 1)
    has = keys[pos] == ids
    return has, np.where(has, vals[pos], 0)


def eval_clauses(clauses, ids, columns):
    """bool per id: does every C-level clause (name, op, a, b) hold -- an id without a value fails every op"""
    ids = np.asarray(ids, np.int64)
    keep = np.ones(ids.shape[0], bool)
    for name, op, a, b in clauses:
        op = OP_CODES[op] if isinstance(op, str) else int(op)
        has, v = _lookup(ids, columns[name])
        a64, b64 = np.int64(a), np.int64(b)
        if op == QK_OP_RANGE:
            r = (a64 <= v) & (v <= b64)
        elif op == QK_OP_NOT_RANGE:
            r = ~((a64 <= v) & (v <= b64))
        elif op == QK_OP_ANY_BITS:
            r = (v & a64) != 0
        elif op == QK_OP_ALL_BITS:
            r = (v & a64) == a64
        elif op == QK_OP_NO_BITS:
            r = (v & a64) == 0
        else:
            raise ValueError(op)
        keep &= has & r
    return keep


def _holds(op, v, a, b):
    """one value against one high-level clause, over the integers; bit ops see v and the mask as 64-bit patterns"""
    if op == "==":
        return v == a
    if op == "!=":
        return v != a
    if op == "<":
        return v < a
    if op == "<=":
        return v <= a
    if op == ">":
        return v > a
    if op == ">=":
        return v >= a
    if op == "between":
        return a <= v <= b
    m64 = (1 << 64) - 1
    if op == "any_bits":
        return (v & a) & m64 != 0
    if op == "all_bits":
        return (v & a) & m64 == a & m64
    if op == "no_bits":
        return (v & a) & m64 == 0
    raise ValueError(op)


def eval_where(where, ids, columns):
    """bool per id: does every (name, op, a[, b]) hold, in Python integers"""
    keep = np.ones(len(ids), bool)
    for cl in where:
        name, op, a = cl[0], cl[1], int(cl[2])
        b = int(cl[3]) if len(cl) > 3 else None
        col = columns[name]
        for i, id_ in enumerate(ids):
            id_ = int(id_)
            keep[i] = keep[i] and id_ in col and bool(_holds(op, int(col[id_]), a, b))
    return keep


def allowed_set(keep, ids):
    return np.unique(np.asarray(ids, np.int64)[keep])


def search(q, centroids, vecs, ids, offsets, nprobe, k, metric, keep, centroid_ids=None):
    """the filtered yardstick over the allowed id set {ids[keep]}"""
    return Y.search(q, centroids, vecs, ids, offsets, nprobe, k, metric, allowed_set(keep, ids), "allow", centroid_ids=centroid_ids)


def scan(q, vecs, ids, offsets, pids, k, metric, keep):
    return Y.scan(q, vecs, ids, offsets, pids, k, metric, allowed_set(keep, ids), "allow")


def tile_words(keep, offsets):
    """the 16-bit word of every FULL 16-row tile of every list (rows of a list are tiled from its first row)"""
    words = []
    for p in range(len(offsets) - 1):
        rows = keep[offsets[p]:offsets[p + 1]]
        nt = rows.shape[0] // 16
        if nt:
            words.append((rows[:nt * 16].reshape(nt, 16) * (1 << np.arange(16))).sum(1))
    return np.concatenate(words) if words else np.zeros(0, np.int64)
