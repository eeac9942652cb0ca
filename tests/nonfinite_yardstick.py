"""The yardstick of search over NaN, Inf and overflowing values (shared by tests/test_nonfinite_oracle.py and
tests/test_nonfinite_search.py; the contract: DESIGN.md 5.8.1, include/quake_hip.h).

One corpus builder plants a handful of special rows of one input class into an ordinary clustered corpus (helpers.make_ivf):
five each at chosen positions of two ordinary lists -- the first tile, the last (partial) tile, inside the 128-row head that seeds a
bound -- and a list made of five special rows only.  The special rows take the lowest ids, in an order that is neither their
stored order nor the bit order of their keys.  A few queries are aimed at those lists, and some of them are special themselves.
brute() is the reference of the rule written from the per-pair values alone: drop NaN, sort by (value, id), take k, pad."""
import numpy as np

import oracle as O
from helpers import make_ivf, make_queries

CLASSES = ("nan", "inf", "overflow", "underflow")
COORD = 3                                  # the coordinate the Inf class works on
ID_ORDER = (1, 3, 0, 4, 2)                 # id of the i-th special row of a set, before the set's base is added
TWO64, TWO65 = np.float32(2.0 ** 64), np.float32(2.0 ** 65)
TINY, ZP = np.float32(2.0 ** -70), np.float32(2.0 ** -100)


def _bits(rows, r, c, word):
    rows.view(np.uint32)[r, c] = word      # (through the integer view: sign and payload of a NaN arrive as written)


def special_rows(cls, base):
    """five special rows of the class, made from five ordinary rows `base` [5, d]"""
    s = np.ascontiguousarray(base[:5], np.float32).copy()
    d = s.shape[1]
    assert s.shape[0] == 5
    if cls == "nan":
        _bits(s, 0, COORD, 0x7FC00000)     # what np.nan, torch and the GPU's default NaN are
        _bits(s, 1, 5 % d, 0xFFC00000)     # negative NaN
        s.view(np.uint32)[2, :] = 0x7FC00000
        _bits(s, 3, 0, 0xFFC12345)         # ... with a payload
        _bits(s, 4, d - 1, 0x7FC00001)
    elif cls == "inf":
        s[0, COORD] = np.inf
        s[1, COORD] = -np.inf
        s[2, COORD] = np.inf               # a second row at the same infinite value: the id decides
        s[3, COORD] = -np.inf
        s[4, COORD], s[4, 7 % d] = np.inf, -np.inf
    elif cls == "overflow":
        s[0] *= TWO64                      # the norm overflows, products with an ordinary query do not
        s[1] *= TWO65
        s[2] *= TWO64
        s[3] *= -TWO64
        s[4] *= TWO65
    elif cls == "underflow":
        s[0] = -ZP                         # against a query of +2^-100 everywhere: every product underflows to -0, the chain ends in -0.0
        s[1] = ZP                          # ... in +0.0
        s[2] = 0.0
        s[3] *= TINY
        s[4] = 0.0
    else:
        raise ValueError(cls)
    return s


def _positions(size):
    p = [1, 2, min(70, size - 3), size // 2, size - 1]
    assert len(set(p)) == 5 and min(p) >= 0, "list too short for five special rows: %d" % size
    return p


def corpus(cls, metric, n, nlist, d, seed, far_tiny=True):
    """ordinary corpus + planted specials.  Returns a dict: centroids, vecs, ids, offsets (CSR), x (the ordinary rows the queries are
    drawn around: not those cut from the tiny list), hosts (the two ordinary lists that hold specials), tiny (the list of five specials), special (CSR rows of all 15)"""
    ivf = make_ivf(n, d, nlist, seed=seed, metric=metric)
    offsets = ivf["offsets"].copy()
    sizes = np.diff(offsets)
    # Which lists hold the specials is chosen so that the special QUERIES reach them in the coarse step, whatever nprobe is: a zero
    # query (IP) and a query whose norm overflowed (L2) tie on every centroid and take the lists of the lowest numbers -- list 0 --;
    # a query of vanishing magnitude ranks the centroids by their norm under L2 and the signed-zero query by the sum of their
    # coordinates under IP -- the other host is the list that wins those (its centroid pulled in to be sure under L2: still by far
    # the nearest one to its own rows).  The list of five specials is a third one.
    cent = ivf["centroids"].copy()
    score = -np.einsum("ij,ij->i", cent, cent) if metric == "l2" else cent.sum(axis=1)
    score[0] = -np.inf
    h0, h1 = int(np.argmax(score)), 0
    if metric == "l2":
        cent[h0] *= np.float32(0.75)
    tiny = int([p for p in np.argsort(-sizes, kind="stable")[nlist // 2:] if p not in (h0, h1)][0])
    assert sizes[tiny] >= 5
    keep = np.ones(offsets[-1], bool)
    keep[offsets[tiny] + 5:offsets[tiny + 1]] = False     # the tiny list keeps five rows
    vecs = np.ascontiguousarray(ivf["vecs"][keep])
    ids = np.ascontiguousarray(ivf["ids"][keep])
    csum = np.zeros(keep.shape[0] + 1, np.int64)
    csum[1:] = np.cumsum(keep)
    offsets = csum[offsets]
    sizes = np.diff(offsets)
    special = []
    for si, lst in enumerate((h0, h1, tiny)):
        pos = list(range(5)) if lst == tiny else _positions(int(sizes[lst]))
        rows = offsets[lst] + np.asarray(pos, np.int64)
        vecs[rows] = special_rows(cls, vecs[rows])
        for r, t in zip(rows, ID_ORDER):                  # lowest ids, the later set first, no order inside a set
            t = t + 5 * (2 - si)
            j = np.nonzero(ids == t)[0]                   # (absent when its row was among those cut from the tiny list)
            if j.shape[0]:
                ids[j[0]] = ids[r]
            ids[r] = t
        special.append(rows)
    if far_tiny:  # out of every ordinary query's reach: only the queries aimed at it probe it (a cold list)
        if metric == "l2":
            cent[tiny] += np.float32(30.0)
        else:
            cent[tiny] *= np.float32(0.4)                 # (a short centroid: its dot product with an ordinary unit query is mid-field)
    assert np.unique(ids).shape[0] == ids.shape[0]
    return dict(centroids=cent, vecs=vecs, ids=ids, offsets=offsets, x=ivf["x"][ivf["assign"] != tiny], hosts=(h0, h1), tiny=tiny,
                special=np.concatenate(special), d=d, nlist=nlist, metric=metric, cls=cls)


def queries(c, nq, seed):
    """(q, special): ordinary queries around the corpus rows; the first ones aimed at the lists that hold specials; `special` names
    the indices of the queries that are special themselves (every pair of theirs may be NaN: checked against all rows)"""
    cls, metric, d = c["cls"], c["metric"], c["d"]
    q = make_queries(nq, d, seed=seed, like=c["x"], metric=metric)
    rng = np.random.default_rng(seed + 1)
    cent = c["centroids"]
    aim = [c["hosts"][i % 2] for i in range(8)] + [c["tiny"]] * 3
    for i, lst in enumerate(aim[:nq]):
        if metric == "ip":
            v = cent[lst] / np.linalg.norm(cent[lst]) + (0.05 * rng.standard_normal(d)).astype(np.float32)
            q[i] = v / np.linalg.norm(v)
        else:
            q[i] = cent[lst] + (0.05 * rng.standard_normal(d)).astype(np.float32)
    sp = []

    def at(i):
        if i < nq:
            sp.append(i)
            return True
        return False
    if cls == "nan":
        if at(1):
            q.view(np.uint32)[1, :] = 0x7FC00000          # the answer is padding only
    elif cls == "inf":
        for i in (1, 9):
            if at(i):
                q[i, COORD] = 0.0                         # inf * 0
    elif cls == "overflow":
        for i in (1, 9):
            if at(i):
                q[i] *= TWO64                             # products overflow, L2 gives inf - inf
    elif cls == "underflow":
        for i in (1, 10):
            if at(i):
                q[i] *= TINY                              # subnormal products
        if at(2):
            q[2] = 0.0
        if at(9):
            q[9] = ZP                                     # the query of the signed-zero pair
    return np.ascontiguousarray(q, np.float32), np.asarray(sp, np.int64)


def probe_counts(c, q, nprobe):
    """(probed [Q, kk] by the oracle's coarse step, number of probing queries per list)"""
    op, _ = O.coarse(q, c["centroids"], None, nprobe, c["metric"], num_threads=8)
    return op, np.bincount(op[op >= 0], minlength=c["nlist"])


def assert_special_queries_meet_specials(c, q, special, nprobe):
    """every special query probes a list that holds planted rows (so that, e.g., the signed-zero pair meets its query in every scan
    form) -- except a query all of whose centroid values are NaN, which probes nothing"""
    op, _ = probe_counts(c, q, nprobe)
    lists = list(c["hosts"]) + [c["tiny"]]
    for i in special:
        if (op[i] < 0).all():
            assert np.isnan(O.pair_values(q[i:i + 1], c["centroids"], c["metric"])).all()
        else:
            assert np.isin(op[i], lists).any(), (int(i), op[i], lists)


def expected(c, q, nprobe, k):
    return O.search(q, c["centroids"], c["vecs"], c["ids"], c["offsets"], nprobe, k, c["metric"], batched_scan=True, num_threads=8)


# ---- the rule from the per-pair values alone -----------------------------------------------------------------------------------
def topk_of_values(val, ids, k, metric):
    """one query: drop NaN, sort by (value, id) -- descending value for IP, -0 == +0 --, take k; returns (ids, values) unpadded"""
    ok = ~np.isnan(val)
    v, i = val[ok], np.asarray(ids, np.int64)[ok]
    order = np.lexsort((i, -v if metric == "ip" else v))[:k]
    return i[order], v[order]


def brute(q, centroids, vecs, ids, offsets, nprobe, k, metric):
    """(ids [Q, k], dist [Q, k]) of search() by the rule: the coarse step over the centroids, then the rows of the probed lists"""
    Q = q.shape[0]
    nlist = centroids.shape[0]
    kk = min(nprobe, nlist)
    cv = O.pair_values(q, centroids, metric)
    out_i = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), -np.inf if metric == "ip" else np.inf, np.float32)
    for i in range(Q):
        pl, _ = topk_of_values(cv[i], np.arange(nlist), kk, metric)
        if pl.shape[0] == 0:
            continue
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pl])
        if rows.shape[0] == 0:
            continue
        val = O.pair_values(q[i:i + 1], vecs[rows], metric)[0]
        bi, bv = topk_of_values(val, ids[rows], k, metric)
        out_i[i, :bi.shape[0]] = bi
        with np.errstate(invalid="ignore"):
            out_d[i, :bv.shape[0]] = np.sqrt(bv) if metric == "l2" else bv
    return out_i, out_d


def assert_same_answer(gi, gd, oi, od):
    """ids exactly; distances as uint32, except that zeros are compared by value (which sign a returned zero carries is not part of
    the contract)"""
    gi, gd, oi, od = np.asarray(gi), np.asarray(gd, np.float32), np.asarray(oi), np.asarray(od, np.float32)
    np.testing.assert_array_equal(gi, oi)
    gz, oz = gd == 0, od == 0
    np.testing.assert_array_equal(gz, oz)
    np.testing.assert_array_equal(gd.view(np.uint32)[~gz], od.view(np.uint32)[~oz])


def assert_no_nan_pair(c, q, special_q, got_ids, allowed=None):
    """directly: no returned id belongs to a (query, row) pair whose canonical value is NaN.  Ordinary queries can only meet a NaN at
    a special row; the special queries are checked against every row."""
    ids, metric = c["ids"], c["metric"]
    got_ids = np.asarray(got_ids)
    sv = O.pair_values(q, c["vecs"][c["special"]], metric)
    sid = ids[c["special"]]
    for i in range(q.shape[0]):
        bad = sid[np.isnan(sv[i])]
        assert not np.isin(got_ids[i], bad).any(), (i, got_ids[i], bad)
    if special_q.shape[0]:
        av = O.pair_values(q[special_q], c["vecs"], metric)
        for j, i in enumerate(special_q):
            bad = ids[np.isnan(av[j])]
            assert not np.isin(got_ids[i], bad).any(), (int(i), got_ids[i])
