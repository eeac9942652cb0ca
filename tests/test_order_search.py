"""Ordered search (qk_order_search / qk_order_scan; Context.order_search / order_scan; QuakeIndex.ordered_search in both mirrors):
per query, the k first hits of the range call with the same arguments by an attribute column, ties to the nearer row, then to the
smaller id.

Every comparison is exact equality of ids, distance bits, values, count, missing and total with tests/order_yardstick.py (pinned on
the CPU by tests/test_order_oracle.py).  The yardstick is evaluated once per situation with k = 1024 and cut to the smaller k's:
"the first k" of a sequence is a prefix of its first 1024.  No assertion reads a clock.  Every test asserts on its own inputs that
the situation it is about occurs.  The corpus, columns and queries are those of tests/test_facet_stats_search.py, rebuilt here."""
import ctypes as C

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import facet_yardstick as FCY
import filter_yardstick as FY
import oracle as O
import order_yardstick as OY
import paging_yardstick as PY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
NAMES = OY.NAMES
SLICE = 1024        # keys per slice of k_order_partial (quake_amd/csrc/qk_facet.h)
KS = (1, 10, 256, 1024)
COLS = ("few", "uniq", "mid", "none", "const")


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    assert len(got) >= 6
    for name, g, w in zip(NAMES, got, want):
        g, w = _np(g), _np(w)
        if name == "dist":
            g, w = g.view(np.uint32), np.ascontiguousarray(w, np.float32).view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, tag))


def _cut(want, k, Q=None):
    return tuple(w[:Q, :k] for w in want[:3]) + tuple(w[:Q] for w in want[3:])


def _attr(s, col):
    from quake_amd.capi import Attr
    a = Attr(s)
    a.set(np.fromiter(col.keys(), np.int64, len(col)), np.fromiter(col.values(), np.int64, len(col)))
    return a


def _stores(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def _uniq_value(i):
    """a distinct signed value per id: multiplication by an odd constant is a bijection of the 64-bit words"""
    return int(np.uint64((int(i) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)).astype(np.int64))


FEW = [I64MIN, -1, 0, 5, I64MAX]


def make_columns(ids, seed):
    """the four columns of tests/test_facet_stats_search.py as dicts id -> value: few (5 values, the extremes and -1, on 95 % of
    the ids), uniq (a value of its own per id), mid (about 300 values, skewed), none (values only for ids that are not stored) --
    plus const (one value on every id) and ramp (the position of the id's row in the store)"""
    rng = np.random.default_rng(seed)
    few_vals = np.array(FEW, np.int64)
    pick = rng.random(ids.shape[0]) < 0.95
    few = {int(i): int(v) for i, v in zip(ids[pick], few_vals[rng.integers(0, 5, size=int(pick.sum()))])}
    uniq = {int(i): _uniq_value(i) for i in ids}
    skew = np.minimum((rng.random(ids.shape[0]) ** 3 * 300).astype(np.int64), 299) * 1000003 - 150000000
    mid = {int(i): int(v) for i, v in zip(ids, skew)}
    none = {int(i): int(i) % 9 for i in range(50000, 50050)}
    const = {int(i): 42 for i in ids}
    ramp = {int(i): r for r, i in enumerate(ids)}
    return dict(few=few, uniq=uniq, mid=mid, none=none, const=const, ramp=ramp)


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    """per metric: the corpus (empty lists, lists of 5 and 7 rows), its stores, the column dicts and their Attr handles, 40 queries"""
    cache = {}

    def get(metric):
        if metric not in cache:
            c = RY.corpus(32, 20, 6000, metric, seed=301 if metric == "l2" else 302)
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and 5 in sizes and 7 in sizes
            s, parent = _stores(ctx, c)
            cols = make_columns(c["ids"], 303)
            assert len(set(cols["uniq"].values())) == c["ids"].shape[0]
            attrs = {k: _attr(s, v) for k, v in cols.items()}
            cache[metric] = dict(c=c, s=s, parent=parent, cols=cols, attrs=attrs, q=RY.queries(c, 40, seed=304), memo={})
        return cache[metric]

    yield get
    for e in cache.values():
        for a in e["attrs"].values():
            a.close()
        e["s"].close()
        e["parent"].close()


def _order(e, nprobe):
    """(paging_yardstick.ordering of the 40 queries, their lists), computed once per nprobe (None: every list)"""
    key = ("order", nprobe)
    if key not in e["memo"]:
        c = e["c"]
        pids = RY.probed(e["q"], None if nprobe is None else c["cent"], c["offsets"], nprobe, c["metric"])
        o = PY.ordering(e["q"], None if nprobe is None else c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe or 1, c["metric"])
        e["memo"][key] = (o, np.broadcast_to(pids, (40, pids.shape[-1])) if pids.ndim == 1 else pids)
    return e["memo"][key]


def _radii(e, nprobe):
    """(tag, radius): one no row passes, one that IS a distance of the first query and keeps about half of its probed rows (the
    boundary row is a hit), everything"""
    metric = e["c"]["metric"]
    mine = np.sort(_order(e, nprobe)[0].dist[0])
    r = mine[mine.shape[0] // 2] if metric == "l2" else mine[-(mine.shape[0] // 2) - 1]
    assert (mine == r).sum() >= 1
    return [("none", -1.0 if metric == "l2" else 1e30), ("half", float(r)), ("all", float("inf") if metric == "l2" else float("-inf"))]


def _want(e, nprobe, radius, col, desc, ml):
    key = ("want", nprobe, radius, col, desc, ml)
    if key not in e["memo"]:
        e["memo"][key] = OY.expected(_order(e, nprobe)[0], radius, e["cols"][col], 1024, desc, ml)
    return e["memo"][key]


# ---- 1. the grid: metric, column, search and scan, nprobe, radius, k, direction, missing policy ------------------------------------
@pytest.mark.parametrize("col", COLS)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_grid(ctx, corpora, metric, col):
    e = corpora(metric)
    s, q, a = e["s"], e["q"], e["attrs"][col]
    seen = set()
    for nprobe in (3, None):
        parent = e["parent"] if nprobe is not None else None
        pids = _order(e, nprobe)[1]
        for tag, radius in _radii(e, nprobe):
            for desc in (False, True):
                for ml in (False, True):
                    want = _want(e, nprobe, radius, col, desc, ml)
                    ids, dist, values, count, missing, total = want
                    assert (count + missing == total).all()
                    for k in KS:
                        t = (metric, col, nprobe, tag, desc, ml, k)
                        _eq(ctx.order_search(parent, s, q, nprobe or 1, radius, metric, a, k, desc, ml), _cut(want, k), t)
                        assert ctx.last_scan_kernel() == "k_scan (order)"
                        Q = 1 if k == 10 else 40
                        _eq(ctx.order_scan(s, q[:Q], pids[:Q], radius, metric, a, k, desc, ml), _cut(want, k, Q), t + ("scan",))
                    shown = np.minimum(total if ml else count, 1024)
                    assert ((ids >= 0).sum(1) == shown).all()
                    if tag == "none":
                        assert total.sum() == 0 and (ids == -1).all()                      # a query with no hit at all
                    if tag != "none" and col == "none":
                        assert (count == 0).all() and (total > 0).any() and (values == 0).all()   # count = 0 < total
                        assert (ids >= 0).any() == ml
                    if tag != "none" and ((count < 1024) & (count > 0)).any():
                        seen.add("fewer than k")
                    if tag == "all" and col == "few" and not ml:
                        # thousands of hits per value: at k = 10 the cut falls between two entries of one value, (key, id) decides
                        w11 = want[2][:, :11]
                        tied = (w11[:, 9] == w11[:, 10]) & (want[0][:, 10] >= 0)
                        assert tied.all() if nprobe is None else tied.any()
                        assert (values[:, 0] == (I64MAX if desc else I64MIN)).any()
                        seen.add("tie at the cut")
                    if tag == "all" and col == "few" and ml and nprobe is None:
                        assert (missing > 0).all() and (count + missing == 6000).all() and (count > 1024).all()
    if col != "none":
        assert "fewer than k" in seen
    if col == "few":
        assert "tie at the cut" in seen


# ---- 2. ties at the cut: three rows with one vector and one value; a row that is a hit twice -----------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_planted_ties(ctx, metric):
    c = RY.corpus(32, 20, 6000, metric, seed=311)
    sizes = np.diff(c["offsets"])
    big = int(np.argmax(sizes))
    rows = c["offsets"][big] + np.array([3, 40, 41])
    c["vecs"][rows] = c["vecs"][rows[0]]
    tid = np.sort(c["ids"][rows])
    s, parent = _stores(ctx, c)
    col = {int(i): 5 for i in c["ids"]}
    for i in tid:
        col[int(i)] = 1
    a = _attr(s, col)
    q = np.ascontiguousarray(np.repeat(c["vecs"][rows[:1]], 3, axis=0))
    q[1:] = RY.queries(c, 2, seed=312)
    inf = float("inf") if metric == "l2" else float("-inf")
    o = PY.ordering(q, None, c["vecs"], c["ids"], c["offsets"], 1, metric)
    at = [int(np.nonzero(o.ids[0] == i)[0][0]) for i in tid]
    assert len({int(o.keys[0][j]) for j in at}) == 1                      # one key: the id decides among the three
    w3 = OY.expected(o, inf, col, 3)
    assert w3[0][0].tolist() == tid.tolist() and (w3[2][0] == 1).all() and len(set(w3[1][0].view(np.uint32).tolist())) == 1
    for k in (1, 2, 3, 4):                                                # k = 1, 2: the cut lies inside the triple
        for desc in (False, True):
            want = OY.expected(o, inf, col, k, desc)
            _eq(ctx.order_search(None, s, q, 1, inf, metric, a, k, desc), want, ("triple", metric, k, desc))
    # descending: the 5997 rows of value 5 come first, the triple is the tail of the order
    wd = OY.expected(o, inf, col, 1024, True)
    assert (wd[2] == 5).all()
    # a row that is a hit twice (its list named twice): two equal entries.  The yardstick sees a store with that list twice
    vecs2 = np.concatenate([c["vecs"], c["vecs"][c["offsets"][big]:c["offsets"][big + 1]]])
    ids2 = np.concatenate([c["ids"], c["ids"][c["offsets"][big]:c["offsets"][big + 1]]])
    offs2 = np.concatenate([c["offsets"], [c["offsets"][-1] + sizes[big]]])
    small = int(np.nonzero(sizes == 7)[0][0])
    pairs = RY.all_pairs(q, vecs2, ids2, offs2, np.array([big, small, 20], np.int64), metric)
    uniq = {int(i): _uniq_value(i) for i in c["ids"]}
    au = _attr(s, uniq)
    twice = np.array([[big, small, big]] * 3, np.int64)
    for k in (1, 2, 9, 256):
        for desc in (False, True):
            want = OY.expected_pairs(q, vecs2, ids2, pairs, inf, metric, uniq, k, desc)
            if k > 1:
                assert (want[0][:, 0] == want[0][:, 1]).all() and (want[2][:, 0] == want[2][:, 1]).all()
            assert (want[5] == 2 * sizes[big] + 7).all()
            _eq(ctx.order_scan(s, q, twice, inf, metric, au, k, desc), want, ("twice", metric, k, desc))
    for x in (a, au, s, parent):
        x.close()


# ---- 3. the partial lists and their merge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_partial_and_merge(ctx, corpora, metric):
    e = corpora(metric)
    c, s, q = e["c"], e["s"], e["q"]
    o, pids = _order(e, None)
    sizes = np.diff(c["offsets"])
    # every query's segment is the whole store in list order: position of a row = its row number; the library's decomposition
    S = -(-20 * int(sizes.max()) // SLICE)
    Sg = min(S, 16384 // 40)
    assert Sg >= 6 and 6000 > 5 * SLICE          # slice j of a query is workgroup j's (j < 6 <= Sg): six workgroups per query
    lims, rows, dist = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    assert (np.diff(lims) == 6000).all() and (rows[:6000] == np.arange(6000)).all()
    # a radius per situation from one query's own distances
    r_one = r_many = None
    for qi in range(40):
        dq = dist[lims[qi]:lims[qi + 1]]
        near = np.argsort(dq if metric == "l2" else -dq, kind="stable")
        for n_near, several in ((20, False), (3000, True)):
            r = float(dq[near[n_near]])
            slices = set((np.nonzero(RY.passes(dq, r, metric))[0] // SLICE).tolist())
            if not several and r_one is None and len(slices) == 1:
                r_one = r                          # query qi: at least 21 hits, all in one slice
            if several and r_many is None and len(slices) >= 4:
                r_many = r                         # query qi: hits in several slices, that is in several workgroups
    assert r_one is not None and r_many is not None
    inf = float("inf") if metric == "l2" else float("-inf")
    for radius in (r_one, r_many, inf):
        for col in ("uniq", "ramp", "few"):
            for desc in (False, True):
                want = OY.expected(o, radius, e["cols"][col], 1024, desc, True)
                for k in (1, 100, 256, 1024):
                    _eq(ctx.order_search(None, s, q, 1, radius, metric, e["attrs"][col], k, desc, True), _cut(want, k),
                        ("partial", metric, radius, col, desc, k))
    # ramp, descending, every row a hit: inside a slice every hit beats all before it, so each of the 1024 hits of a workgroup is
    # a candidate -- more than 2 * kp for kp = 1, 128, 256: the buffer of 512 records is cut back at least twice per workgroup
    assert all(e["cols"]["ramp"][int(i)] == r for r, i in enumerate(c["ids"][:2000])) and SLICE > 2 * 256 + 256


# ---- 4. filters; order_scan with -1, absent and empty lists ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filters(ctx, corpora, metric):
    from quake_amd.capi import Filter
    e = corpora(metric)
    c, s, parent, q, cols, attrs = e["c"], e["s"], e["parent"], e["q"][:17], e["cols"], e["attrs"]
    ids = c["ids"]
    radius = _radii(e, 3)[1][1]
    S = FY.draw_set(ids, 0.3, np.random.default_rng(321))
    where = [("mid", "between", -150000000, -150000000 + 40 * 1000003), ("few", "!=", 0)]
    cases = [
        ("allow", Filter(s, S, "allow"), FCY.allowed_ids(ids, FY.allowed_rows(ids, S, "allow"))),
        ("deny", Filter(s, S, "deny"), FCY.allowed_ids(ids, FY.allowed_rows(ids, S, "deny"))),
        ("where", Filter.where(s, [(attrs["mid"], "range", where[0][2], where[0][3]), (attrs["few"], "not_range", 0, 0)]),
         FCY.allowed_ids(ids, AY.eval_where(where, ids, cols))),
        ("nothing", Filter(s, np.array([10 ** 8], np.int64), "allow"), np.zeros(0, np.int64)),
    ]
    pids = RY.probed(q, c["cent"], c["offsets"], 4, metric)
    plain = OY.expected(PY.ordering(q, c["cent"], c["vecs"], ids, c["offsets"], 4, metric), radius, cols["few"], 1024, False, True)
    for tag, f, allowed in cases:
        if tag == "nothing":   # (a CSR without rows: the answer is all padding)
            o = PY.Order([np.zeros(0, np.int64)] * 17, [np.zeros(0, np.float32)] * 17, [np.zeros(0, np.uint32)] * 17, metric)
        else:
            o = PY.ordering(q, c["cent"], c["vecs"], ids, c["offsets"], 4, metric, S=allowed, mode="allow")
        for col in ("few", "uniq"):
            for desc, ml in ((False, True), (True, False)):
                want = OY.expected(o, radius, cols[col], 1024, desc, ml)
                if col == "few" and ml:
                    assert want[5].sum() == 0 if tag == "nothing" else 0 < want[5].sum() < plain[5].sum()
                for k in (10, 1024):
                    _eq(ctx.order_search(parent, s, q, 4, radius, metric, attrs[col], k, desc, ml, filter=f), _cut(want, k),
                        (metric, tag, col, k))
                    _eq(ctx.order_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(pids).cuda(), radius, metric, attrs[col], k, desc, ml,
                                       filter=f), _cut(want, k), (metric, tag, col, k, "scan, device"))
        f.close()
    sizes = np.diff(c["offsets"])
    empty = int(np.nonzero(sizes == 0)[0][0])
    edge = np.array([[5, -1, 9], [-1, -1, -1], [10 ** 6, 7, empty], [-1, 6, -1], [20, 21, 10 ** 12]], np.int64)
    inf = float("inf") if metric == "l2" else float("-inf")
    o = PY.ordering(q[:5], None, c["vecs"], ids, c["offsets"], None, metric, pids=np.where(edge >= 20, -1, edge))
    want = OY.expected(o, inf, cols["mid"], 1024, False, True)
    assert [t > 0 for t in want[5]] == [True, False, True, True, False]
    for k in (7, 1024):
        _eq(ctx.order_scan(s, q[:5], edge, inf, metric, attrs["mid"], k, False, True), _cut(want, k), "edge pids")
        _eq(ctx.order_scan(s, torch.from_numpy(q[:5]).cuda(), torch.from_numpy(edge).cuda(), inf, metric, attrs["mid"], k, False, True),
            _cut(want, k), "edge pids, device")


# ---- 5. squared L2; the counters are those of facet statistics -----------------------------------------------------------------------------
def test_squared_l2_and_counters(ctx, corpora):
    e = corpora("l2")
    s, parent, q = e["s"], e["parent"], e["q"]
    o = _order(e, 3)[0]
    d64 = np.sort(o.dist[0].astype(np.float64)) ** 2
    gaps = np.nonzero(np.diff(d64) > 1e-4 * d64[1:])[0]
    j = int(gaps[gaps.shape[0] // 2])
    r2 = np.float32((d64[j] + d64[j + 1]) / 2)      # no squared distance within 1e-5 of it: sqrt(v) <= sqrt(r2) <=> v <= r2
    r = np.float32(np.sqrt(np.float64(r2)))
    want = OY.expected(o, r, e["cols"]["uniq"], 10)
    assert want[5].sum() > 0
    _eq(ctx.order_search(parent, s, q, 3, r, "l2", e["attrs"]["uniq"], 10), want, "sqrt")
    ctx.set_squared_l2(True)
    try:
        got = ctx.order_search(parent, s, q, 3, r2, "l2", e["attrs"]["uniq"], 10)
        # the squared distance is reported; its correctly rounded root is what the call reports otherwise
        _eq((got[0], np.sqrt(got[1]), *got[2:]), want, "squared")
    finally:
        ctx.set_squared_l2(False)
    for metric in ("l2", "ip"):
        e = corpora(metric)
        for _, radius in _radii(e, 3):
            for col in ("few", "none"):
                got = ctx.order_search(e["parent"], e["s"], e["q"], 3, radius, metric, e["attrs"][col], 5)
                st = ctx.facet_stats_search(e["parent"], e["s"], e["q"], 3, radius, metric, e["attrs"][col])
                np.testing.assert_array_equal(got[3], st[0][0])
                np.testing.assert_array_equal(got[4], st[1][0])
                np.testing.assert_array_equal(got[5], st[7])


# ---- 6. liveness ---------------------------------------------------------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = RY.corpus(32, 20, 6000, "l2", seed=331)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(332)
    q = RY.queries(c, 17, seed=333)
    pids = RY.probed(q, c["cent"], c["offsets"], 6, "l2")
    col = {int(i): int(i) % 12 - 6 for i in c["ids"][::2]}
    a = _attr(s, col)
    radius = 5.5

    def check(tag):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(20)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        o = PY.ordering(q, None, vecs, ids, offs, None, "l2", pids=pids)
        out = []
        for desc, ml in ((False, False), (True, True)):
            want = OY.expected(o, radius, col, 1024, desc, ml)
            assert want[5].sum() > 0
            for k in (3, 1024):
                _eq(ctx.order_scan(s, q, pids, radius, "l2", a, k, desc, ml), _cut(want, k), (tag, desc, ml, k))
            out.append(want)
        return out

    w0 = check("as built")
    assert w0[0][2][:, 0].min() == -6 and w0[1][2][:, 0].max() == 5
    some = c["ids"][1::2][:800]
    for i in some:
        col[int(i)] = 1000 + int(i) % 3
    a.set(some, np.array([col[int(i)] for i in some]))
    w1 = check("set_attribute")
    assert w1[0][4].sum() < w0[0][4].sum() and w1[1][2][:, 0].max() == 1002
    gone = some[:400]
    for i in gone:
        del col[int(i)]
    a.unset(gone)
    w2 = check("unset")
    assert w2[0][4].sum() > w1[0][4].sum()
    s.remove_ids(c["ids"][::5])
    w3 = check("remove")
    assert w3[0][5].sum() < w2[0][5].sum()
    na = 400
    new_ids = np.arange(10 ** 6, 10 ** 6 + na, dtype=np.int64)
    lists = rng.integers(4, 20, size=na).astype(np.int64)
    new_vecs = (c["cent"][lists] + 0.3 * rng.standard_normal((na, 32))).astype(np.float32)
    lists[:17] = pids[:, 0]
    new_vecs[:17] = q + np.float32(1e-3)
    for i in new_ids[::2]:
        col[int(i)] = -777
    a.set(new_ids[::2], np.full(na // 2, -777, np.int64))
    s.add_batch(new_ids, new_vecs, lists)
    w4 = check("add, with and without values")
    assert (w4[0][2][:, 0] == -777).any() and w4[0][5].sum() > w3[0][5].sum() and w4[0][4].sum() > w3[0][4].sum()
    a.close()
    s.close()
    parent.close()


# ---- 7. wide rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    c = RY.corpus(2600, 3, 300, metric, seed=341, empty=0)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 7, seed=342)
    cols = make_columns(c["ids"], 343)
    o = PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 2, metric)
    d0 = np.sort(o.dist[0])
    for name in ("few", "uniq"):
        a = _attr(s, cols[name])
        for radius in (float(d0[d0.shape[0] // 2]), float("inf") if metric == "l2" else float("-inf")):
            for desc in (False, True):
                want = OY.expected(o, radius, cols[name], 1024, desc, True)
                assert want[5].sum() > 0
                for k in (1, 10, 1024):
                    _eq(ctx.order_search(parent, s, q, 2, radius, metric, a, k, desc, True), _cut(want, k), ("wide", metric, name, k))
                    assert ctx.last_scan_kernel() == "k_scan_wide (order)"
        a.close()
    s.close()
    parent.close()


# ---- 8. several passes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1024, 7])
def test_passes(ctx, k):
    """k = 1024 is also the one place where the 2048-record buffer of the large instantiation is cut INSIDE the sweep: the partial
    lists of 932 queries of 1024 records each are held to 128 MiB, which leaves 5 workgroups per query, each with about 26 slices of
    1024 hits (every row is a hit) -- more than the 1792 records the buffer takes before its first cut.  With a larger budget for
    the lists a workgroup would see fewer slices and this test would lose that situation."""
    from quake_amd.capi import Attr, Store
    d, nlist, n, Q = 16, 64, 1 << 17, 1040
    rng = np.random.default_rng(351)
    sizes = np.full(nlist, (n - 9000) // (nlist - 1), np.int64)
    sizes[0] = 9000
    sizes[-1] += n - sizes.sum()
    assert sizes.sum() == n and sizes.max() >= 8192 and nlist * sizes.max() >= 1 << 19
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    vals = rng.integers(I64MIN // 4, I64MAX // 4, size=n).astype(np.int64)
    vals[:3] = [I64MIN, I64MAX, -1]
    assert np.unique(vals).shape[0] == n
    q = rng.standard_normal((Q, d)).astype(np.float32)
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    a = Attr(s)
    a.set(ids, vals)
    asc = np.argsort(vals, kind="stable")
    ctx.set_timing(1)
    try:
        for desc in (False, True):
            first = (asc[::-1] if desc else asc)[:k]
            oi, od, ov, cnt, mis, tot, tm = ctx.order_search(None, s, q, 1, float("inf"), "l2", a, k, desc, timing=True)
            assert tm["n_items"] >= 2
            # radius +inf and no NaN: every stored row is a hit of every query, so every query's answer is the column's own first k
            assert (cnt == n).all() and (mis == 0).all() and (tot == n).all()
            np.testing.assert_array_equal(oi, np.broadcast_to(ids[first], (Q, k)))
            np.testing.assert_array_equal(ov, np.broadcast_to(vals[first], (Q, k)))
            per_pass = (1 << 29) // (nlist * 9000)                       # queries of a pass: 2^29 keys over 64 lists of up to 9000
            # ... which the call itself confirms: with another pass size the number of passes it reports would differ, and the
            # queries checked below would no longer be the first and the last of a pass
            assert per_pass < Q <= 2 * per_pass and tm["n_items"] == -(-Q // per_pass) == 2
            for qi in (0, per_pass - 1, per_pass, Q - 1):                # the first and the last query of each pass
                want = np.sqrt(O.pair_values(q[qi:qi + 1], vecs[first], "l2")[0])
                np.testing.assert_array_equal(od[qi].view(np.uint32), want.astype(np.float32).view(np.uint32))
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 9. device and host memory, NULL outputs, determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_memory_null_outputs_and_determinism(ctx, corpora, metric):
    from quake_amd.capi import metric_code
    e = corpora(metric)
    s, parent, q, a = e["s"], e["parent"], e["q"], e["attrs"]["few"]
    radius = _radii(e, 3)[1][1]
    k = 100
    host = ctx.order_search(parent, s, q, 3, radius, metric, a, k, True, True)
    _eq(host, _cut(_want(e, 3, radius, "few", True, True), k), "host")
    assert host[5].sum() > 0
    dev = ctx.order_search(parent, s, torch.from_numpy(q).cuda(), 3, radius, metric, a, k, True, True)
    assert all(t.is_cuda for t in dev)
    _eq(dev, host, "device")
    again = ctx.order_search(parent, s, q, 3, radius, metric, a, k, True, True)
    for x, y in zip(host, again):
        assert x.tobytes() == y.tobytes()
    again = ctx.order_search(parent, s, torch.from_numpy(q).cuda(), 3, radius, metric, a, k, True, True)
    torch.cuda.synchronize()   # (the context's stream is its own: torch reads the results behind a device-wide wait)
    for x, y in zip(dev, again):
        assert torch.equal(x, y)
    # every output but ids may be NULL, each on its own -- in host and in device memory
    P = lambda b: C.c_void_p(b.ctypes.data) if isinstance(b, np.ndarray) else C.c_void_p(b.data_ptr())  # noqa: E731
    for mem, xq in ((0, q), (1, torch.from_numpy(q).cuda())):
        for skip in range(6):
            if mem == 0:
                bufs = [np.full(h.shape, -7, h.dtype) for h in host]
            else:
                bufs = [torch.full(tuple(h.shape), -7, dtype=torch.float32 if h.dtype == np.float32 else torch.int64, device="cuda")
                        for h in host]
            ptrs = [None if (j == skip and j != 0) else P(b) for j, b in enumerate(bufs)]
            st = ctx.lib.qk_order_search(ctx.h, parent.h, s.h, P(xq), 40, 3, metric_code(metric), C.c_float(radius), None, a.h, 3, k,
                                         *ptrs, mem, None)
            assert st == 0
            for j in range(6):
                if j == skip and j != 0:
                    assert (_np(bufs[j]) == -7).all()
                else:
                    assert _np(bufs[j]).tobytes() == host[j].tobytes(), "%s with output %d NULL, mem %d" % (NAMES[j], skip, mem)


# ---- 10. limits and errors at the C level ---------------------------------------------------------------------------------------------------------
def test_limits(ctx, corpora):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter, Store
    e, e2 = corpora("l2"), corpora("ip")
    s, parent, q, attrs = e["s"], e["parent"], e["q"][:5], e["attrs"]
    mid = attrs["mid"]
    pids = RY.probed(q, e["c"]["cent"], e["c"]["offsets"], 4, "l2")
    plain = ctx.order_search(parent, s, q, 4, 6.0, "l2", mid, 1024)
    assert plain[5].sum() > 0
    for k, match in ((0, "QK_ERR_INVALID.*k=0"), (-3, "QK_ERR_INVALID.*k=-3"), (1025, "QK_ERR_UNSUPPORTED.*k=1025")):
        with pytest.raises(QuakeHipError, match=match):
            ctx.order_search(parent, s, q, 4, 6.0, "l2", mid, k)
        with pytest.raises(QuakeHipError, match=match):
            ctx.order_scan(s, q, pids, 6.0, "l2", mid, k)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.order_search(parent, s, q, 4, 6.0, "l2", e2["attrs"]["mid"], 5)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.order_search(parent, s, q, 4, 6.0, "l2", None, 5)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*NaN"):
        ctx.order_search(parent, s, q, 4, float("nan"), "l2", mid, 5)
    f2 = Filter(e2["s"], e2["c"]["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.order_search(parent, s, q, 4, 6.0, "l2", mid, 5, filter=f2)
    f2.close()
    # Q == 0 is served
    empty = ctx.order_search(parent, s, q[:0], 4, 6.0, "l2", mid, 5)
    assert empty[0].shape == (0, 5) and empty[3].shape == (0,)
    # no lists probed: a store without lists -- all padding and zeros
    bare = Store(ctx, 32)
    ab = _attr(bare, {1: 1})
    got = ctx.order_search(None, bare, q, 1, 6.0, "l2", ab, 4, False, True)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and all((got[j] == 0).all() for j in (2, 3, 4, 5))
    ab.close()
    bare.close()
    # the context still answers, and answers the same
    _eq(ctx.order_search(parent, s, q, 4, 6.0, "l2", mid, 1024), plain, "after the refusals")
    _eq(ctx.order_scan(s, q, pids, 6.0, "l2", mid, 1024), plain, "scan")


# ---- 11. the mirrors -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def _build(mod, x, ids, nlist, metric="l2", workers=0):
    idx = mod.QuakeIndex()
    bp = mod.IndexBuildParams()
    bp.nlist, bp.metric, bp.num_workers = nlist, metric, workers
    idx.build(x, ids, bp)
    return idx


def _res(r):
    return (r.ids, r.distances, r.values, r.counts, r.missing, r.totals)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(qb, metric, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(361)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(17, d, generator=g)
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(362)))
    idx = _build(quake, x, ids, 20, metric)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    for m in (idx, loaded):
        m.set_attribute("cat", ids[::2], ids[::2] % 7 - 3)
        m.set_attribute("big", ids, (ids * 3 + 1000) * (1 << 48))
    radius = 7.5 if metric == "l2" else 0.5
    inf = float("inf") if metric == "l2" else float("-inf")
    seen_missing = False
    for k in (3, 300):
        sp, spc = quake.SearchParams(), qb.SearchParams()
        for p in (sp, spc):
            p.nprobe, p.k = 5, k
        for exclude in (None, True):
            sp.filter = None if exclude is None else idx.make_filter(S, exclude)
            spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
            for rad in (None, radius):
                for name in ("cat", "big"):
                    for desc, missing in ((False, "exclude"), (True, "last")):
                        # the C ABI call on the index's own store (the index's own k-means decides the lists)
                        want = idx._ctx.order_search(idx.parent._store if idx.parent is not None else None, idx._store, q.numpy(), 5,
                                                     inf if rad is None else rad, metric, idx._attributes()[name], k, desc,
                                                     missing == "last", filter=sp.filter._h if sp.filter is not None else None)
                        assert want[5].sum() > 0
                        seen_missing = seen_missing or (missing == "last" and (want[2][want[0] >= 0] == 0).any() and want[4].sum() > 0)
                        t = (metric, k, exclude, rad, name, desc, missing)
                        r = idx.ordered_search(q, name, sp, radius=rad, descending=desc, missing=missing)
                        _eq(_res(r), want, ("python",) + t)
                        assert r.column == name and r.timing_info.n_queries == 17 and tuple(r.ids.shape) == (17, k)
                        rd = idx.ordered_search(q.cuda(), name, sp, radius=rad, descending=desc, missing=missing)
                        assert all(o.is_cuda for o in _res(rd))
                        _eq(_res(rd), want, ("python, device",) + t)
                        for xq in (q, q.cuda()):
                            rc = loaded.ordered_search(xq, name, spc, radius=rad, descending=desc, missing=missing)
                            assert rc.ids.is_cuda == xq.is_cuda and rc.totals.is_cuda == xq.is_cuda and rc.column == name
                            _eq(_res(rc), want, ("compiled", xq.is_cuda) + t)
        sp.filter = spc.filter = None
    assert seen_missing
    for m, p in ((idx, sp), (loaded, spc)):
        empty = m.ordered_search(q[:0], "cat", p)
        assert tuple(empty.ids.shape) == (0, 300) and tuple(empty.values.shape) == (0, 300) and tuple(empty.totals.shape) == (0,)


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(371)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        idx.set_attribute("doc", ids, ids % 50)

        def params(**kw):
            sp = mod.SearchParams()
            sp.k, sp.nprobe = 5, 4
            for k, v in kw.items():
                setattr(sp, k, v)
            return sp

        plain = idx.ordered_search(qq, "doc", params(), radius=5.0)
        assert plain.totals.sum() > 0
        for kw, match in ((dict(recall_target=0.9), "recall_target"),
                          (dict(filters=[idx.make_filter(ids[:1000])], query_filter=torch.zeros(10, dtype=torch.int32)), "query_filter"),
                          (dict(max_nprobe=8), "max_nprobe"),
                          (dict(filter_exact_rows=100, filter=idx.make_filter(ids[:50])), "filter_exact_rows"),
                          (dict(filters_exact_rows=100), "filters_exact_rows"),
                          (dict(filter=other.make_filter(ids[:1000])), "another index"),
                          (dict(k=0), "k=0 must be between 1 and 1024"),
                          (dict(k=1025), "k=1025 must be between 1 and 1024")):
            with pytest.raises(RuntimeError, match=match):
                idx.ordered_search(qq, "doc", params(**kw), radius=5.0)
        with pytest.raises(RuntimeError, match="unknown attribute column 'nope'"):
            idx.ordered_search(qq, "nope", params(), radius=5.0)
        with pytest.raises(RuntimeError, match="NaN"):
            idx.ordered_search(qq, "doc", params(), radius=float("nan"))
        with pytest.raises(RuntimeError, match="missing must be 'exclude' or 'last', got 'first'"):
            idx.ordered_search(qq, "doc", params(), radius=5.0, missing="first")
        # a call with two faults raises the same error in both mirrors: refusals, column, k, missing, filter, radius
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.ordered_search(qq, "nope", params(recall_target=0.9), radius=5.0)
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.ordered_search(qq, "nope", params(k=0), radius=5.0, missing="first")
        with pytest.raises(RuntimeError, match="k=0"):
            idx.ordered_search(qq, "doc", params(k=0), radius=float("nan"), missing="first")
        with pytest.raises(RuntimeError, match="missing must be"):
            idx.ordered_search(qq, "doc", params(filter=other.make_filter(ids[:1000])), radius=float("nan"), missing="first")
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.ordered_search(qq, "doc", params(), radius=5.0)
        again = idx.ordered_search(qq, "doc", params(), radius=5.0)
        for a, b in zip(_res(again), _res(plain)):
            assert torch.equal(a, b)
