"""The yardstick of grouped search (shared by tests/test_grouped_oracle.py and tests/test_grouped_search.py).

Expected values come from the oracle as it is: for every probed list O.pair_values gives the canonical value of EVERY row in stored
order (squared L2 / inner product, before any square root, NaN included).  A query's candidates are the rows of its probed lists
that have a value in the column, are allowed, and whose canonical value is not NaN; they are ordered by that canonical value -- L2
ascending, IP descending, -0 == +0 -- then by id (ordering on the reported L2 distance would invent ties: sqrt is not injective
in float32); the first row of every group value is its representative, the first k representatives are the answer, padded like a
short search() result.  Distances are reported as search() does (sqrt of the squared form).  A filter: the same over the reduced
CSR of tests/filter_yardstick.py.  Nothing here knows about keys, hash tables or kernels."""
import numpy as np

import filter_yardstick as FY
import oracle as O


def row_values(ids, attr_ids, attr_vals):
    """(value int64, has bool) per CSR row of the column {attr_ids[i]: attr_vals[i]} (attr_ids unique)"""
    ids = np.asarray(ids, np.int64)
    attr_ids, attr_vals = np.asarray(attr_ids, np.int64), np.asarray(attr_vals, np.int64)
    assert np.unique(attr_ids).shape[0] == attr_ids.shape[0]
    if attr_ids.shape[0] == 0:
        return np.zeros(ids.shape[0], np.int64), np.zeros(ids.shape[0], bool)
    order = np.argsort(attr_ids, kind="stable")
    si, sv = attr_ids[order], attr_vals[order]
    at = np.minimum(np.searchsorted(si, ids), si.shape[0] - 1)
    has = si[at] == ids
    return np.where(has, sv[at], 0), has


def candidates(q, vecs, ids, offsets, pids, metric):
    """Every (query, probed row) of the call: (lims [Q + 1], rows, val) -- query i owns [lims[i], lims[i+1]), rows are CSR row
    numbers, val the oracle's canonical float32 values (squared L2 / inner product).  -1, out-of-range and empty lists contribute
    nothing."""
    q = np.ascontiguousarray(q, np.float32)
    offsets = np.asarray(offsets, np.int64)
    nlist = offsets.shape[0] - 1
    Q = q.shape[0]
    pids = np.asarray(pids, np.int64)
    if pids.ndim == 1:
        pids = np.broadcast_to(pids[None, :], (Q, pids.shape[0]))
    sizes = np.diff(offsets)
    ok = (pids >= 0) & (pids < nlist)
    psz = np.where(ok, sizes[np.where(ok, pids, 0)], 0)
    base = np.zeros(Q * pids.shape[1] + 1, np.int64)
    base[1:] = np.cumsum(psz.reshape(-1))
    pair_base = base[:-1].reshape(pids.shape)
    lims = np.ascontiguousarray(base[::pids.shape[1]] if pids.shape[1] > 0 else np.zeros(Q + 1, np.int64))
    rows = np.empty(base[-1], np.int64)
    val = np.empty(base[-1], np.float32)
    assert np.unique(ids).shape[0] == np.asarray(ids).shape[0], "ids must be unique within a store"
    for p in np.unique(pids[ok]):
        n = int(sizes[p])
        if n == 0:
            continue
        qi, ri = np.nonzero(pids == p)
        assert np.unique(qi).shape[0] == qi.shape[0], "a pids row names list %d twice" % p
        v = O.pair_values(q[qi], vecs[offsets[p]:offsets[p + 1]], metric)   # [nq, n] in stored row order, NaN included
        dst = pair_base[qi, ri][:, None] + np.arange(n, dtype=np.int64)[None, :]
        val[dst] = v
        rows[dst] = offsets[p] + np.arange(n, dtype=np.int64)[None, :]
    return lims, rows, val


def reduce(cand, ids, rowval, rowhas, k, metric):
    """(ids [Q, k], dist [Q, k], groups [Q, k]) from candidates(): representatives, then the k best, then padding"""
    lims, rows, val = cand
    ids = np.asarray(ids, np.int64)
    Q = lims.shape[0] - 1
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, np.float32)
    out_g = np.zeros((Q, k), np.int64)
    for i in range(Q):
        r, v = rows[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
        keep = rowhas[r] & ~np.isnan(v)
        r, v = r[keep], v[keep]
        if r.shape[0] == 0:
            continue
        key = (-v if metric == "ip" else v) + np.float32(0.0)   # (-0 + 0 == +0: both zeros are one value)
        order = np.lexsort((ids[r], key))
        r, v = r[order], v[order]
        _, first = np.unique(rowval[r], return_index=True)
        first = np.sort(first)[:k]
        n = first.shape[0]
        out_i[i, :n] = ids[r[first]]
        with np.errstate(invalid="ignore"):
            out_d[i, :n] = np.sqrt(v[first]) if metric == "l2" else v[first]
        out_g[i, :n] = rowval[r[first]]
    return out_i, out_d, out_g


def scan(q, vecs, ids, offsets, pids, k, metric, attr_ids, attr_vals, S=None, mode="allow", keep=None):
    """scan_grouped's expected (ids, dist, groups); S / mode (an id set) or keep (bool per row): a filter, applied by deleting the
    other rows from the CSR first"""
    if S is not None:
        keep = FY.allowed_rows(ids, S, mode)
    if keep is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, keep)
    rowval, rowhas = row_values(ids, attr_ids, attr_vals)
    return reduce(candidates(q, vecs, ids, offsets, pids, metric), ids, rowval, rowhas, k, metric)


def probed(q, centroids, offsets, nprobe, metric):
    if centroids is None:
        return np.arange(np.asarray(offsets).shape[0] - 1, dtype=np.int64)
    return O.coarse(q, centroids, None, nprobe, metric, num_threads=8)[0]


def search(q, centroids, vecs, ids, offsets, nprobe, k, metric, attr_ids, attr_vals, S=None, mode="allow", keep=None):
    """search_grouped's expected (ids, dist, groups): the lists O.coarse ranks (None: every list)"""
    return scan(q, vecs, ids, offsets, probed(q, centroids, offsets, nprobe, metric), k, metric, attr_ids, attr_vals, S, mode, keep)
