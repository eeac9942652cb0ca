"""A numpy model of the exact finish of the fp16 shadow form (k_shadow_finish, quake_amd/csrc/qk_shadow.hip) on
caller-built records, and the builder of such records.  No GPU here: tests/test_shadow_finish_oracle.py pins the model on the host,
tests/test_shadow_finish.py compares the kernel with it bit for bit through qk_debug_shadow_finish.

The rule, per query (keys are the integer keys the kernels order by, smaller = better):
  1. a_k = the k-th smallest approximate key of all entries of the query's records (none: 0xFFFFFFFF); thr = a_k moved by 2E
  2. the candidates are the entries with key <= thr; their exact keys come from the oracle's canonical chain (oracle.pair_values),
     the k best under (key, id) are the answer, tau = the k-th exact key
  3. verified if no record is full (32 entries), or the smallest last key of the full records is > tau moved by E
  4. not verified, no record, or no bound (E negative or NaN): the probed list is scanned exactly (the fallback), if it has rows
"""
import numpy as np

import oracle as O

KP = 32       # entries per record
SLOTS = 32    # ints per slot line: the count and 31 record numbers
NONE = np.uint32(0xFFFFFFFF)


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
def key_of(v, metric):
    """ord_from_l2 / ord_from_ip of float32 values (qk_device.h)"""
    v = np.asarray(v, np.float32)
    b = v.view(np.uint32).copy()
    if metric == "l2":
        out = b
    else:
        b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)
        asc = b ^ np.where((b >> np.uint32(31)) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
        out = ~asc
    return np.where(np.isnan(v), NONE, out).astype(np.uint32)


def value_of(key, metric):
    """the float32 value behind a key (L2: the squared distance; IP: ip_from_ord)"""
    key = np.asarray(key, np.uint32)
    if metric == "l2":
        return key.view(np.float32)
    asc = ~key
    b = np.where((asc & np.uint32(0x80000000)) != 0, asc ^ np.uint32(0x80000000), ~asc).astype(np.uint32)
    return b.view(np.float32)


def widen(key, E, metric):
    """qk_ord_widen: the key moved by E towards worse in float32, rounded to nearest and then one step outwards; none stays"""
    key = np.uint32(key)
    if key == NONE:
        return key
    E = np.float32(E)
    with np.errstate(all="ignore"):
        if metric == "l2":
            f = np.float32(value_of(key, "l2") + E)
            return key_of(np.nextafter(f, np.float32(np.inf)), "l2")[()]
        f = np.float32(value_of(key, "ip") - E)
        return key_of(np.nextafter(f, np.float32(-np.inf)), "ip")[()]


# ---- records ---------------------------------------------------------------------------------------------------------------------------
class Records:
    """the scan's record structures for Q queries with one pair each: add(q, keys, lists, positions) appends a record to query q the
    way the scan does -- the first 31 into the slot line, the rest chained in front of pair_head"""

    def __init__(self, Q, max_recs):
        self.Q = Q
        self.pair_slots = np.zeros((Q, SLOTS), np.int32)
        self.pair_slots[:, 1:] = -1
        self.pair_head = np.full(Q, -1, np.int32)
        self.rec_hdr = np.zeros((max_recs, 2), np.int32)
        self.rec_hdr[:, 0] = -1
        self.rec_ord = np.full((max_recs, KP), 0xFFFFFFFF, np.uint32)
        self.ent_list = np.zeros((max_recs, KP), np.int64)
        self.ent_pos = np.zeros((max_recs, KP), np.int64)
        self.n = 0

    def add(self, q, keys, lists, pos):
        r = self.n
        self.n += 1
        m = len(keys)
        assert m <= KP and r < self.rec_hdr.shape[0]
        self.rec_hdr[r] = (-1, m)
        self.rec_ord[r, :m] = keys
        self.ent_list[r, :m] = lists
        self.ent_pos[r, :m] = pos
        slot = int(self.pair_slots[q, 0])
        self.pair_slots[q, 0] = slot + 1
        if slot < SLOTS - 1:
            self.pair_slots[q, 1 + slot] = r
        else:
            self.rec_hdr[r, 0] = self.pair_head[q]
            self.pair_head[q] = r
        return r

    def of_query(self, q):
        """record numbers in the order the kernel walks them"""
        n = int(self.pair_slots[q, 0])
        recs = [int(r) for r in self.pair_slots[q, 1:1 + min(n, SLOTS - 1)] if r >= 0]
        if n > SLOTS - 1:
            r = int(self.pair_head[q])
            while r >= 0:
                recs.append(r)
                r = int(self.rec_hdr[r, 0])
        return recs

    def arrays(self):
        return dict(pair_slots=self.pair_slots, pair_head=self.pair_head, rec_hdr=self.rec_hdr, rec_ord=self.rec_ord,
                    ent_list=self.ent_list, ent_pos=self.ent_pos)


def consistent_records(x, E, lists, offsets, vecs, metric, seed, seg=(20, 90)):
    """records a shadow scan could have left: every query's probed list cut into segments of seg[0]..seg[1] rows, each keeping its
    32 smallest approximate keys, ascending.  Consistent: an approximate key lies within E of the exact one (0.9 E here, in the
    value's domain), so a dropped row's key is at or above its full record's last one."""
    rng = np.random.default_rng(seed)
    Q = x.shape[0]
    sizes = [int(offsets[p + 1] - offsets[p]) if p >= 0 else 0 for p in lists]
    recs = Records(Q, max(1, sum((n + seg[0] - 1) // seg[0] for n in sizes)))
    for q in range(Q):
        p, n = int(lists[q]), sizes[q]
        if n == 0:
            continue
        ev = O.pair_values(x[q:q + 1], vecs[offsets[p]:offsets[p + 1]], metric)[0]
        approx = (ev + (0.9 * max(float(E[q]), 0.0) * rng.uniform(-1, 1, n)).astype(np.float32)).astype(np.float32)
        if metric == "l2":
            approx = np.maximum(approx, np.float32(0))
        keys = key_of(approx, metric)
        lo = 0
        while lo < n:
            hi = min(n, lo + int(rng.integers(seg[0], seg[1] + 1)))
            order = lo + np.argsort(keys[lo:hi], kind="stable")[:KP]
            recs.add(q, keys[order], np.full(len(order), p), order)
            lo = hi
    return recs


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _best(q, rows, ids, k, metric):
    """the k best of rows under (exact key, id): keys, ids"""
    if len(ids) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64)
    keys = key_of(O.pair_values(q[None, :], rows, metric)[0], metric)
    live = keys != NONE
    keys, ids = keys[live], np.asarray(ids, np.int64)[live]
    order = np.lexsort((ids, keys))[:k]
    return keys[order], ids[order]


def model(x, E, lists, recs, offsets, vecs, ids, k, metric, sqrt_l2=True):
    """offsets / vecs / ids: the store's lists in CSR form (list p = rows offsets[p]:offsets[p + 1], positions in that order).
    Returns a dict: ids [Q, k], dist [Q, k], verified / fallback [Q] bool, candidates [Q], chained [Q] bool, tau [Q] (the k-th
    exact key of the candidates, 0xFFFFFFFF if fewer), fullmin [Q]."""
    Q = x.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), np.inf if metric == "l2" else -np.inf, np.float32)
    res = dict(ids=out_i, dist=out_d, verified=np.zeros(Q, bool), fallback=np.zeros(Q, bool), candidates=np.zeros(Q, np.int64),
               chained=np.zeros(Q, bool), tau=np.full(Q, NONE, np.uint32), fullmin=np.full(Q, NONE, np.uint32))
    for q in range(Q):
        flagged = not (E[q] >= 0)
        nrecs = int(recs.pair_slots[q, 0])
        bk, bi = np.zeros(0, np.uint32), np.zeros(0, np.int64)
        if not flagged and nrecs > 0:
            res["chained"][q] = nrecs > SLOTS - 1
            rl = recs.of_query(q)
            keys = np.concatenate([recs.rec_ord[r, :recs.rec_hdr[r, 1]] for r in rl] + [np.zeros(0, np.uint32)])
            el = np.concatenate([recs.ent_list[r, :recs.rec_hdr[r, 1]] for r in rl] + [np.zeros(0, np.int64)])
            ep = np.concatenate([recs.ent_pos[r, :recs.rec_hdr[r, 1]] for r in rl] + [np.zeros(0, np.int64)])
            full = [recs.rec_ord[r, KP - 1] for r in rl if recs.rec_hdr[r, 1] >= KP]
            fullmin = np.uint32(min(full)) if full else NONE
            a_k = np.sort(keys)[k - 1] if len(keys) >= k else NONE
            thr = widen(a_k, np.float32(2.0) * np.float32(E[q]), metric)
            cand = keys <= thr
            res["candidates"][q] = int(cand.sum())
            rows = offsets[el[cand]] + ep[cand]
            bk, bi = _best(x[q], vecs[rows], ids[rows], k, metric)
            tau = bk[k - 1] if len(bk) >= k else NONE
            res["tau"][q], res["fullmin"][q] = tau, fullmin
            res["verified"][q] = fullmin == NONE or (tau != NONE and fullmin > widen(tau, E[q], metric))
        if not res["verified"][q]:
            p = int(lists[q])
            bk, bi = np.zeros(0, np.uint32), np.zeros(0, np.int64)
            if p >= 0 and offsets[p + 1] > offsets[p]:
                res["fallback"][q] = True
                bk, bi = _best(x[q], vecs[offsets[p]:offsets[p + 1]], ids[offsets[p]:offsets[p + 1]], k, metric)
        out_i[q, :len(bi)] = bi
        v = value_of(bk, metric)
        out_d[q, :len(bk)] = np.sqrt(v) if (metric == "l2" and sqrt_l2) else v
    return res
