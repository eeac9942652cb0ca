"""The yardstick of the merge stage (shared by tests/test_merge_oracle.py, tests/test_merge_records.py, tests/test_merge_ranks.py and
tests/test_sharded_gpu.py).  Written from the contract -- include/quake_hip.h, DESIGN.md sections 3, 5.8.1 and 5.12 --, not from
the kernels:

  * the key maps as integer arithmetic on uint32 views: a float becomes a key whose unsigned order is the order of the answer
    (ascending distance for L2, descending inner product for IP), NaN becomes 0xFFFFFFFF, -0 and +0 share a key under IP;
  * a builder that lays records out the way the scan leaves them (pair slot lines, chains, record headers, keys and ids);
  * the reference merge: the union of a query's entries sorted under (key, id), its first k, the padding, the next cursor;
  * the same for the cross-rank merge over [G][Q][k] runs."""
import numpy as np

QK_SLOTS = 32                      # ints of a pair's slot line: the record count + 31 record numbers
NAN_KEY = np.uint32(0xFFFFFFFF)
INT64_MAX = np.iinfo(np.int64).max
POISON_KEY, POISON_ID = np.uint32(0), np.int64(0)   # behind a record's count: the best key there is, a valid id


# ---- key maps --------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def ord_from_l2(v):
    """squared distances (>= +0, or NaN) -> keys: the float's bits order non-negative floats; NaN -> 0xFFFFFFFF"""
    v = np.ascontiguousarray(v, np.float32)
    return np.where(np.isnan(v), NAN_KEY, _bits(v)).astype(np.uint32)


def ord_from_ip(v):
    """inner products -> keys, the larger product the smaller key; -0 -> the key of +0; NaN -> 0xFFFFFFFF"""
    v = np.ascontiguousarray(v, np.float32)
    b = _bits(v).copy()
    b[b == np.uint32(0x80000000)] = 0
    asc = b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)  # ascending in the float
    return np.where(np.isnan(v), NAN_KEY, ~asc).astype(np.uint32)


def ip_from_ord(o):
    asc = ~np.ascontiguousarray(o, np.uint32)
    b = np.where(asc & np.uint32(0x80000000) != 0, asc ^ np.uint32(0x80000000), ~asc).astype(np.uint32)
    return b.view(np.float32)


def ord_of(v, metric):
    return ord_from_ip(v) if metric == "ip" else ord_from_l2(v)


def dist_from_ord(o, metric, sqrt_l2):
    """what the answer shows for a key: the inner product / the squared distance, or its square root when asked"""
    o = np.ascontiguousarray(o, np.uint32)
    if metric == "ip":
        return ip_from_ord(o)
    d2 = o.view(np.float32)
    return np.sqrt(d2) if sqrt_l2 else d2.copy()


def pad_dist(metric):
    return np.float32(-np.inf) if metric == "ip" else np.float32(np.inf)


# ---- records as the scan leaves them ----------------------------------------------------------------------------------------------
def build_records(queries, k, rng, spare=3):
    """queries[q][p] = the records of pair (q, p) in the order they arrived, each record a tuple (keys uint32 [n], ids int64 [n]) with
    1 <= n <= k, or (keys, ids, True) for a record that did NOT FIT: it takes its place in the pair's count and, where it arrived
    among the first 31, a slot holding -1, but no record exists (its entries are no candidates).  Every query has the same number
    of pairs P.  Returns a dict with the arrays of MergeParams:
        pair_slots int32 [Q, P, 32]   {count, first 31 record numbers}; slots behind the count hold stale but valid record numbers
        pair_head  int32 [Q, P]       head of the chain of the records beyond 31, -1 without one
        rec_hdr    int32 [R, 2]       {next record of the chain or -1, entry count}
        rec_ord    uint32 [R, k], rec_id int64 [R, k]: the record's entries sorted under (key, id), poison behind the count
    and max_recs = R (records + `spare` unused ones; record numbers are a random permutation, so a pair's records are scattered),
    plus `entries`: per query the (keys, ids) of every candidate, for the reference."""
    Q = len(queries)
    P = len(queries[0])
    assert P >= 1 and all(len(qp) == P for qp in queries)
    nrec = sum(1 for qp in queries for pr in qp for rec in pr if not (len(rec) > 2 and rec[2]))
    R = nrec + spare
    number = rng.permutation(R)
    slots = np.zeros((Q, P, QK_SLOTS), np.int32)
    head = np.full((Q, P), -1, np.int32)
    hdr = np.zeros((R, 2), np.int32)
    hdr[:, 0] = -1
    rord = np.full((R, k), POISON_KEY, np.uint32)
    rid = np.full((R, k), POISON_ID, np.int64)
    entries = []
    nxt = 0
    for q in range(Q):
        ek, ei = [np.zeros(0, np.uint32)], [np.zeros(0, np.int64)]
        for p in range(P):
            count = 0
            for rec in queries[q][p]:
                keys, ids = np.asarray(rec[0], np.uint32), np.asarray(rec[1], np.int64)
                lost = len(rec) > 2 and bool(rec[2])
                n = keys.shape[0]
                assert 1 <= n <= k and ids.shape[0] == n
                r = -1
                if not lost:
                    r = int(number[nxt])
                    nxt += 1
                    o = np.lexsort((ids, keys))
                    rord[r, :n], rid[r, :n] = keys[o], ids[o]
                    hdr[r, 1] = n
                    ek.append(keys)
                    ei.append(ids)
                if count < QK_SLOTS - 1:
                    slots[q, p, 1 + count] = r
                elif not lost:                        # beyond the line: pushed onto the chain, naming the previous head
                    hdr[r, 0] = head[q, p]
                    head[q, p] = r
                count += 1
            slots[q, p, 0] = count
            if count < QK_SLOTS - 1 and nrec > 0:     # what a slot line holds behind its count is left over: valid numbers, not ours
                slots[q, p, 1 + count:] = number[rng.integers(0, nrec, size=QK_SLOTS - 1 - count)]
        entries.append((np.concatenate(ek), np.concatenate(ei)))
    assert nxt == nrec
    return dict(pair_slots=slots, pair_head=head, rec_hdr=hdr, rec_ord=rord, rec_id=rid, max_recs=R, k=k, P=P, Q=Q, entries=entries,
                n_records=nrec)


def walk_records(rb, q, p):
    """the record numbers of pair (q, p) as the layout names them: the slot line's (without the -1 of a record that did not fit),
    then the chain from pair_head; fails on a number outside the arrays or a chain that does not end"""
    line = rb["pair_slots"][q, p]
    count = int(line[0])
    out = []
    for r in line[1:1 + min(count, QK_SLOTS - 1)]:
        assert -1 <= r < rb["max_recs"]
        if r >= 0:
            assert rb["rec_hdr"][r, 0] == -1
            out.append(int(r))
    r = int(rb["pair_head"][q, p])
    if count <= QK_SLOTS - 1:
        assert r == -1
    steps = 0
    while r != -1:
        assert 0 <= r < rb["max_recs"] and steps <= rb["max_recs"], "malformed chain"
        out.append(r)
        r = int(rb["rec_hdr"][r, 0])
        steps += 1
    return out


# ---- the reference merge ----------------------------------------------------------------------------------------------------------
def first_k(keys, ids, k):
    """the first k of the entries under (key, id)"""
    o = np.lexsort((np.asarray(ids, np.int64), np.asarray(keys, np.uint32)))[:k]
    return np.asarray(keys, np.uint32)[o], np.asarray(ids, np.int64)[o]


def merge_reference(entries, k, metric, sqrt_l2):
    """entries: per query (keys, ids).  Returns ids int64 [Q, k], dist float32 [Q, k] (padding -1 / +inf (L2) / -inf (IP)) and the
    next cursor (key uint32 [Q], id int64 [Q]): (key, id) of the k-th result, (0xFFFFFFFF, INT64_MAX) for a row short of k"""
    Q = len(entries)
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), pad_dist(metric), np.float32)
    nk = np.full(Q, NAN_KEY, np.uint32)
    ni = np.full(Q, INT64_MAX, np.int64)
    for q, (keys, ids) in enumerate(entries):
        bk, bi = first_k(keys, ids, k)
        n = bk.shape[0]
        out_i[q, :n] = bi
        out_d[q, :n] = dist_from_ord(bk, metric, sqrt_l2)
        if n == k:
            nk[q], ni[q] = bk[k - 1], bi[k - 1]
    return out_i, out_d, nk, ni


def merge_ranks_reference(ids, keys, metric, sqrt_l2=True):
    """ids int64 / keys float32 [G, Q, k]: per-rank results (keys = squared L2 distances / inner products).  An entry with id < 0 or
    a NaN key is no candidate; the answer is the first k of the union of the candidates under (key, id)."""
    ids, keys = np.asarray(ids, np.int64), np.asarray(keys, np.float32)
    G, Q, k = ids.shape
    entries = []
    for q in range(Q):
        i, o = ids[:, q, :].reshape(-1), ord_of(keys[:, q, :].reshape(-1), metric)
        ok = (i >= 0) & (o != NAN_KEY)
        entries.append((o[ok], i[ok]))
    out_i, out_d, _, _ = merge_reference(entries, k, metric, sqrt_l2)
    return out_i, out_d


def sorted_runs(ids, keys, metric):
    """[G, Q, k] entries -> the same entries with every run sorted under (key, id), the NaN keys behind the candidates and the -1 ids
    behind those: what a rank sends"""
    ids, keys = np.asarray(ids, np.int64).copy(), np.asarray(keys, np.float32).copy()
    G, Q, k = ids.shape
    for g in range(G):
        for q in range(Q):
            o = np.lexsort((ids[g, q], ord_of(keys[g, q], metric), ids[g, q] < 0))
            ids[g, q], keys[g, q] = ids[g, q][o], keys[g, q][o]
    return ids, keys


# ---- synthetic queries --------------------------------------------------------------------------------------------------------------
KEY_MODES = ("distinct", "best_last", "five", "equal", "special")


def draw_values(n, mode, metric, rng):
    """n float32 values (squared distances / inner products) of a key mode:
    distinct    no two alike (as keys);  best_last: distinct, the later the better (no bound from an early record prunes a later one)
    five        five values, so that ids decide almost everywhere;  equal: one value
    special     +inf (L2), both infinities, -0 and +0 (IP) among a few ordinary values"""
    if mode in ("distinct", "best_last"):
        v = np.zeros(0, np.float32)
        while v.shape[0] < n:
            raw = rng.random(2 * n + 16) * 8 if metric == "l2" else rng.standard_normal(2 * n + 16)
            v = np.unique(np.concatenate([v, raw.astype(np.float32)]))
            v = v[v != 0]
        v = rng.permutation(v)[:n]
        if mode == "best_last":
            v = np.sort(v)[::-1] if metric == "l2" else np.sort(v)
        return np.ascontiguousarray(v, np.float32)
    if mode == "five":
        five = np.array([0.25, 0.5, 1.0, 1.5, 4.0], np.float32) if metric == "l2" else np.array([-2.0, -0.5, 0.25, 1.0, 3.0], np.float32)
        return five[rng.integers(0, 5, size=n)]
    if mode == "equal":
        return np.full(n, 1.75 if metric == "l2" else -0.375, np.float32)
    if mode == "special":
        pool = [np.inf, np.inf, 0.0, 0.5, 3.0, 3.4e38] if metric == "l2" else [np.inf, -np.inf, -np.inf, -0.0, 0.0, 0.0, -0.0, 1.0, -1.0]
        return np.array(pool, np.float32)[rng.integers(0, len(pool), size=n)]
    raise ValueError(mode)


def draw_ids(n, rng):
    """n unique ids, about half of them above 2^32"""
    return (rng.permutation(2 * n + 8)[:n].astype(np.int64) + 1) + np.where(rng.random(n) < 0.5, np.int64(1) << 33, np.int64(0))


def make_query(counts, mode, metric, rng, tie=None, flip=False, lost=None):
    """one query's records: counts[p] = the entry counts of pair p's records; keys by `mode`, unique ids.
    tie = (k, "records" | "pairs"): the k-th and (k+1)-th entries of the union get one key and adjacent ids and sit in two records
    of one pair / in two pairs (flip: the later record holds the winner).  lost = (p, i): record i of pair p did not fit."""
    sizes = [n for pr in counts for n in pr]
    N = int(sum(sizes))
    keys = ord_of(draw_values(N, mode, metric, rng), metric)
    ids = draw_ids(N, rng)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if tie is not None:
        k, where = tie
        first = []          # (pair, flat position of the record's first entry)
        r = 0
        for p, pr in enumerate(counts):
            for _ in pr:
                first.append((p, int(start[r])))
                r += 1
        pick = None
        for a in range(len(first)):
            for b in range(a + 1, len(first)):
                if (first[a][0] == first[b][0]) == (where == "records"):
                    pick = (first[a][1], first[b][1])
                    break
            if pick:
                break
        assert pick is not None and N > k, "no place for the tie"
        e1, e2 = pick

        def swap(x, y):
            keys[[x, y]], ids[[x, y]] = keys[[y, x]], ids[[y, x]]
        s = np.lexsort((ids, keys))
        a, b = int(s[k - 1]), int(s[k])
        swap(a, e1)
        b = a if b == e1 else b
        swap(b, e2)
        keys[e2] = keys[e1]
        top = int(ids.max()) + 10
        ids[e1], ids[e2] = (top + 1, top) if flip else (top, top + 1)
    out, r = [], 0
    for p, pr in enumerate(counts):
        recs = []
        for i, n in enumerate(pr):
            lo = int(start[r])
            rec = (keys[lo:lo + n], ids[lo:lo + n])
            if lost is not None and lost == (p, i):
                rec = rec + (True,)
            recs.append(rec)
            r += 1
        out.append(recs)
    return out


# ---- the geometries one launch covers ---------------------------------------------------------------------------------------------
REC_COUNTS = (0, 1, 8, 9, 31, 32, 33)       # records of a pair: none, one, around a fetch group of 8, around the 31 slots
LONG_CHAINS = (31 + 256, 31 + 257)          # ... and chains around one pooling round of 256
POOL_WIDE = 2048                            # entries the widest pool holds: "all keys equal" overflows it several times


def _pair_counts(P, rng, heavy=3):
    """records per pair: every value of REC_COUNTS where P allows; with many pairs only `heavy` of them hold more than 9"""
    c = rng.choice(REC_COUNTS, size=P)
    if P > 9:
        big = np.nonzero(c > 9)[0]
        if big.shape[0] > heavy:
            c[rng.permutation(big)[heavy:]] = rng.choice((0, 1, 1, 8, 9), size=big.shape[0] - heavy)
    if P >= len(REC_COUNTS):
        c[rng.permutation(P)[:len(REC_COUNTS)]] = REC_COUNTS
    return [int(v) for v in c]


def _sizes(nrec, k, fill, rng):
    if fill == "full":
        return [k] * nrec
    return [k if rng.random() < 0.4 else int(rng.integers(1, k + 1)) for _ in range(nrec)]   # mix


def record_cases(k, P, metric, seed):
    """the queries of one launch at (k, P), each with a geometry of its own: (names, queries) for build_records"""
    rng = np.random.default_rng(seed)
    names, qs = [], []

    def add(name, counts, mode, **kw):
        names.append(name)
        qs.append(make_query(counts, mode, metric, rng, **kw))

    def ensure_more_than_k(counts):           # (so that a tie on the k-th key has a (k+1)-th entry, in a second record of pair 0)
        while sum(n for pr in counts for n in pr) <= k + 1 or len(counts[0]) < 2:
            counts[0].append(k)
        if P >= 2 and not counts[1]:
            counts[1].append(max(1, k // 2))
        return counts

    add("empty", [[] for _ in range(P)], "distinct")
    add("mix", [_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)], "distinct")
    add("full", [_sizes(c, k, "full", rng) for c in _pair_counts(P, rng)], "distinct")
    # every record short and the total under k: the answer ends in padding
    total, short = int(rng.integers(0, k)), [[] for _ in range(P)]
    while total > 0:
        n = int(min(total, rng.integers(1, 4)))
        short[int(rng.integers(0, P))].append(n)
        total -= n
    add("short", short, "distinct")
    add("five", [_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)], "five")
    # all keys equal, full records, several times the widest pool (bounded at 320 records for small k)
    nrec = int(min(320, -(-4 * POOL_WIDE // k)))
    per = [nrec // P + (1 if p < nrec % P else 0) for p in range(P)]
    add("equal", [[k] * c for c in per], "equal")
    add("tie_records", ensure_more_than_k([_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)]), "distinct", tie=(k, "records"),
        flip=bool(seed & 1))
    add("tie_pairs", ensure_more_than_k([_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)]), "distinct",
        tie=(k, "pairs" if P >= 2 else "records"), flip=not (seed & 1))
    add("special", [_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)], "special")
    # one pair with a long chain whose records hold the best keys (the k-th result lives in a chained record)
    chain = [_sizes(int(rng.integers(0, 2)), k, "mix", rng) for _ in range(P)]
    nlong = LONG_CHAINS[seed % 2]
    chain[int(rng.integers(0, P))] = [k if i % 37 == 5 else int(rng.integers(1, min(k, 3) + 1)) for i in range(nlong)]
    add("chain", chain, "best_last")
    # a record that did not fit, in the middle of a slot line
    lost = [_sizes(c, k, "mix", rng) for c in _pair_counts(P, rng)]
    if len(lost[0]) < 3:
        lost[0] = _sizes(9, k, "mix", rng)
    add("lost", lost, "distinct", lost=(0, 1))
    return names, qs
