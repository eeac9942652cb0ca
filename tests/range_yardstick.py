"""The yardstick of range search (shared by tests/test_range_oracle.py and tests/test_range_search.py).

Expected values come from the oracle as it is: for every list p and the queries that probe it, O.pair_values gives the canonical
distance of EVERY row of the list in stored row order -- the values the batched scan selects on, before its top-k drops a NaN
(DESIGN 5.8.1), so a NaN pair is still here and passes() is what refuses it.  A query's lists are then walked in the order of its pids row (O.coarse's rank order for a search) and the rows that pass
the radius in float32 are kept.  A filter: the same over the reduced CSR of tests/filter_yardstick.py.  Nothing here knows about
keys, slices or kernels."""
import numpy as np

import filter_yardstick as FY
import oracle as O


def all_pairs(q, vecs, ids, offsets, pids, metric):
    """Every (query, probed row) of the call in scan order: (lims [Q + 1], rows, dist) -- query i owns [lims[i], lims[i+1]), rows
    are CSR row numbers (int64), dist the oracle's float32 distances.  -1, out-of-range and empty lists contribute nothing."""
    q = np.ascontiguousarray(q, np.float32)
    offsets = np.asarray(offsets, np.int64)
    nlist = offsets.shape[0] - 1
    Q = q.shape[0]
    pids = np.asarray(pids, np.int64)
    if pids.ndim == 1:
        pids = np.broadcast_to(pids[None, :], (Q, pids.shape[0]))
    sizes = np.diff(offsets)
    ok = (pids >= 0) & (pids < nlist)
    psz = np.where(ok, sizes[np.where(ok, pids, 0)], 0)           # [Q, P] rows of every pair
    base = np.zeros(Q * pids.shape[1] + 1, np.int64)
    base[1:] = np.cumsum(psz.reshape(-1))
    pair_base = base[:-1].reshape(pids.shape)
    lims = np.ascontiguousarray(base[::pids.shape[1]] if pids.shape[1] > 0 else np.zeros(Q + 1, np.int64))
    assert lims.shape[0] == Q + 1
    rows = np.empty(base[-1], np.int64)
    dist = np.empty(base[-1], np.float32)
    for p in np.unique(pids[ok]):
        n = int(sizes[p])
        if n == 0:
            continue
        qi, ri = np.nonzero(pids == p)
        assert np.unique(qi).shape[0] == qi.shape[0], "a pids row names list %d twice" % p
        lid = ids[offsets[p]:offsets[p + 1]]
        assert np.unique(lid).shape[0] == n, "ids must be unique"
        val = O.pair_values(q[qi], vecs[offsets[p]:offsets[p + 1]], metric)   # [nq, n] in stored row order, NaN included
        with np.errstate(invalid="ignore"):
            od = np.sqrt(val) if metric == "l2" else val                     # (what a search returns: sqrt of the squared form)
        dst = pair_base[qi, ri][:, None] + np.arange(n, dtype=np.int64)[None, :]
        dist[dst] = od
        rows[dst] = offsets[p] + np.arange(n, dtype=np.int64)[None, :]
    return lims, rows, dist


def passes(dist, radius, metric):
    """the float32 test of the interface: inclusive, NaN never passes"""
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        return dist <= r if metric == "l2" else dist >= r


def select(pairs, ids, radius, metric):
    """(lims, ids, dist) of the rows of all_pairs() that pass the radius, scan order kept"""
    lims, rows, dist = pairs
    keep = passes(dist, radius, metric)
    csum = np.zeros(keep.shape[0] + 1, np.int64)
    csum[1:] = np.cumsum(keep)
    return csum[lims], np.asarray(ids, np.int64)[rows[keep]], dist[keep]


def scan(q, vecs, ids, offsets, pids, radius, metric, S=None, mode="allow"):
    """range_scan's expected (lims, ids, dist); S / mode: a filter, applied by deleting the other rows from the CSR first"""
    if S is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, FY.allowed_rows(ids, S, mode))
    return select(all_pairs(q, vecs, ids, offsets, pids, metric), ids, radius, metric)


def search(q, centroids, vecs, ids, offsets, nprobe, radius, metric, S=None, mode="allow"):
    """range_search's expected (lims, ids, dist): the lists O.coarse ranks (None: every list, in list order)"""
    return scan(q, vecs, ids, offsets, probed(q, centroids, offsets, nprobe, metric), radius, metric, S, mode)


def probed(q, centroids, offsets, nprobe, metric):
    if centroids is None:
        return np.arange(np.asarray(offsets).shape[0] - 1, dtype=np.int64)
    return O.coarse(q, centroids, None, nprobe, metric, num_threads=8)[0]


# ---- the corpus both test files use (the pattern of tests/test_filtered_search.py) ------------------------------------------------
def corpus(d, nlist, n, metric, seed, empty=2):
    """clustered rows in skewed lists: `empty` empty lists, two lists of a handful of rows (shorter than a tile), the rest of
    whatever length the draw gives (almost never a multiple of 16); unique ids in no order"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 0.05
    w[:empty + 2] = 0.0
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    assign[:5] = empty          # a list of 5 rows
    assign[5:12] = empty + 1    # ... and one of 7
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) + 7
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return dict(cent=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets, x=x, d=d,
                metric=metric)


def queries(c, Q, seed):
    rng = np.random.default_rng(seed)
    q = (c["x"][rng.integers(0, c["x"].shape[0], size=Q)] + 0.05 * rng.standard_normal((Q, c["d"]))).astype(np.float32)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q)
