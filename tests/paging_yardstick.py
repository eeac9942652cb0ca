"""The yardstick of paged search (shared by tests/test_paging_oracle.py and tests/test_paging_search.py; the definition:
include/quake_hip.h, "paged search").

One query at a time.  The candidates of a query are the rows of its probed lists whose canonical value (O.pair_values) is not NaN,
restricted to a filter by deleting the other rows from the CSR first (tests/filter_yardstick.py).  Their order is the one the
oracle's search gives them when it is asked for all of them (K = every probed row); the integer key of a row is the documented
image of its canonical value, and the order is checked here to be ascending in (key, id).  A cursor is a (key, id); the page behind
it starts at its position in that order.  Nothing here knows about masks, tiles or kernels."""
import numpy as np

import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

START = (0, -1)                                  # below every row
EXHAUSTED = (0xFFFFFFFF, np.iinfo(np.int64).max)  # behind every row


def key_of(val, metric):
    """uint32 keys of canonical values: smaller = better; NaN -> 0xFFFFFFFF (never a candidate); -0 and +0 share a key.
    L2: the bits of the squared distance (>= +0).  IP: the order-reversing image of the value's bits."""
    val = np.ascontiguousarray(val, np.float32)
    b = val.view(np.uint32).copy()
    if metric == "ip":
        b[b == 0x80000000] = 0
        neg = (b >> 31).astype(bool)
        asc = np.where(neg, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000))
        b = ~asc
    b = b.astype(np.uint32)
    b[np.isnan(val)] = 0xFFFFFFFF
    return b


class Order:
    """every candidate of every query in result order: ids[i], dist[i] (what a search reports), keys[i] -- arrays of one length"""

    def __init__(self, ids, dist, keys, metric):
        self.ids, self.dist, self.keys, self.metric = ids, dist, keys, metric

    def __len__(self):
        return len(self.ids)


def ordering(q, centroids, vecs, ids, offsets, nprobe, metric, S=None, mode="allow", pids=None):
    """the full (key, id) order of every query's candidates.  centroids None: a flat index (every list); pids: the scan form"""
    q = np.ascontiguousarray(q, np.float32)
    if S is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, FY.allowed_rows(ids, S, mode))
    ids = np.asarray(ids, np.int64)
    probed = RY.probed(q, centroids, offsets, nprobe, metric) if pids is None else np.asarray(pids, np.int64)
    lims, rows, _ = RY.all_pairs(q, vecs, ids, offsets, probed, metric)
    K = max(1, int(np.diff(lims).max()) if q.shape[0] else 1)
    if pids is None:
        oi, od = O.search(q, centroids, vecs, ids, offsets, nprobe, K, metric, batched_scan=True, num_threads=8)
    else:
        oi, od = O.batched_serial_scan(q, vecs, ids, offsets, probed, K, metric)
    out_i, out_d, out_k = [], [], []
    for i in range(q.shape[0]):
        r = rows[lims[i]:lims[i + 1]]
        val = O.pair_values(q[i:i + 1], vecs[r], metric)[0] if r.shape[0] else np.zeros(0, np.float32)
        key = key_of(val, metric)
        n = int((key != 0xFFFFFFFF).sum())
        assert (oi[i, :n] >= 0).all() and (oi[i, n:] == -1).all(), "the oracle returns every candidate, and only candidates"
        by_id = dict(zip(ids[r].tolist(), key.tolist()))
        k_sorted = np.array([by_id[int(t)] for t in oi[i, :n]], np.uint32)
        i_sorted = oi[i, :n].copy()
        # the oracle's order IS the (key, id) order
        order = np.lexsort((i_sorted, k_sorted))
        assert (order == np.arange(n)).all(), "query %d: the oracle's order is not ascending in (key, id)" % i
        out_i.append(i_sorted)
        out_d.append(od[i, :n].copy())
        out_k.append(k_sorted)
    return Order(out_i, out_d, out_k, metric)


def position(order, i, cursor):
    """how many of query i's candidates lie at or before the cursor (key, id)"""
    ck, cid = int(cursor[0]) & 0xFFFFFFFF, int(cursor[1])
    k, d = order.keys[i].astype(np.int64), order.ids[i]
    return int(((k < ck) | ((k == ck) & (d <= cid))).sum())


def page_at(order, i, pos, k):
    """(ids [k], dist [k], next cursor) of the page that starts at position pos of query i's order"""
    ids, dist, keys = order.ids[i], order.dist[i], order.keys[i]
    out_i = np.full(k, -1, np.int64)
    out_d = np.full(k, -np.inf if order.metric == "ip" else np.inf, np.float32)
    n = max(0, min(k, ids.shape[0] - pos))
    out_i[:n] = ids[pos:pos + n]
    out_d[:n] = dist[pos:pos + n]
    nxt = (int(keys[pos + k - 1]), int(ids[pos + k - 1])) if n == k else EXHAUSTED
    return out_i, out_d, nxt


def page(order, cursors, k):
    """the batch: cursors = list of (key, id), one per query -> (ids [Q, k], dist [Q, k], next cursors)"""
    Q = len(order)
    oi = np.empty((Q, k), np.int64)
    od = np.empty((Q, k), np.float32)
    nxt = []
    for i in range(Q):
        oi[i], od[i], c = page_at(order, i, position(order, i, cursors[i]), k)
        nxt.append(c)
    return oi, od, nxt


def cursor_arrays(cursors):
    """a list of (key, id) as the arrays the interface takes: keys int32 holding the uint32 bit pattern, ids int64"""
    keys = np.array([c[0] & 0xFFFFFFFF for c in cursors], np.uint32).view(np.int32)
    return keys, np.array([c[1] for c in cursors], np.int64)


def cursor_list(keys, ids):
    keys = np.asarray(keys).astype(np.int32).view(np.uint32)
    return [(int(a), int(b)) for a, b in zip(keys, np.asarray(ids))]
