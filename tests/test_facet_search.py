"""Facet counts (qk_facet_search / qk_facet_scan; Context.facet_search / facet_scan; QuakeIndex.facet_counts in both mirrors): per
query, the value counts of attribute columns over the hits of the range call with the same arguments.

Every comparison is exact equality of all five outputs -- values, counts, distinct, missing, total -- with
tests/facet_yardstick.py (pinned on the CPU by tests/test_facet_oracle.py), whose hits are tests/range_yardstick.py's.  No
assertion reads a clock.  Every test asserts on its own inputs that the situation it is about occurs."""
import ctypes as C

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import expr_yardstick as EY
import facet_yardstick as FCY
import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAMES = ("values", "counts", "distinct", "missing", "total")


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(_np(g), w, err_msg="%s %s" % (name, tag))


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


def make_columns(ids, seed):
    """the four columns of these tests as dicts id -> value: few (5 values, the extremes and -1, on 95 % of the ids), uniq (a value
    of its own per id), mid (about 300 values, skewed), none (values only for ids that are not stored)"""
    rng = np.random.default_rng(seed)
    few_vals = np.array([I64MIN, -1, 0, 5, I64MAX], np.int64)
    pick = rng.random(ids.shape[0]) < 0.95
    few = {int(i): int(v) for i, v in zip(ids[pick], few_vals[rng.integers(0, 5, size=int(pick.sum()))])}
    uniq = {int(i): _uniq_value(i) for i in ids}
    skew = np.minimum((rng.random(ids.shape[0]) ** 3 * 300).astype(np.int64), 299) * 1000003 - 150000000   # ~300 values, skewed
    mid = {int(i): int(v) for i, v in zip(ids, skew)}
    none = {int(i): int(i) % 9 for i in range(50000, 50050)}                                               # no stored id
    return dict(few=few, uniq=uniq, mid=mid, none=none)


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
            assert len(set(cols["uniq"].values())) == c["ids"].shape[0] and 250 <= len(set(cols["mid"].values())) <= 300
            attrs = {k: _attr(s, v) for k, v in cols.items()}
            cache[metric] = dict(c=c, s=s, parent=parent, cols=cols, attrs=attrs, q=RY.queries(c, 40, seed=304), hits={})
        return cache[metric]

    yield get
    for e in cache.values():
        for a in e["attrs"].values():
            a.close()
        e["s"].close()
        e["parent"].close()


def _pairs(e, nprobe):
    """range_yardstick.all_pairs of the 40 queries, computed once per nprobe (None: every list)"""
    key = ("pairs", nprobe)
    if key not in e["hits"]:
        c = e["c"]
        pids = RY.probed(e["q"], None if nprobe is None else c["cent"], c["offsets"], nprobe, c["metric"])
        e["hits"][key] = RY.all_pairs(e["q"], c["vecs"], c["ids"], c["offsets"], pids, c["metric"])
    return e["hits"][key]


def _hits(e, nprobe, radius, Q=40):
    lims, hid, _ = RY.select(_pairs(e, nprobe), e["c"]["ids"], radius, e["c"]["metric"])
    return FCY.split(lims, hid)[:Q]


def _want(e, hits, names, n):
    return FCY.expected_cols(hits, [e["cols"][k] for k in names], n)


def _cut(want, Q, n):
    """the expectation of the first Q queries and n_values = n from one computed for more of both: the order (-count, value) of a
    query does not depend on the other queries, and its first n entries are the n best"""
    v, c, d, m, t = want
    return v[:, :Q, :n], c[:, :Q, :n], d[:, :Q], m[:, :Q], t[:Q]


def _radii(e, nprobe):
    """(tag, radius): one no row passes, one that IS a distance of the range result (the boundary row is a hit), everything"""
    metric = e["c"]["metric"]
    lims, _, dist = _pairs(e, nprobe)
    mine = dist[lims[0]:lims[1]]
    mine = np.sort(mine[~np.isnan(mine)])
    r = mine[mine.shape[0] // 3] if metric == "l2" else mine[-(mine.shape[0] // 3) - 1]
    assert (mine == r).sum() >= 1
    return [("none", -1.0 if metric == "l2" else 2.0), ("boundary", float(r)), ("all", float("inf") if metric == "l2" else float("-inf"))]


ALL4 = ["few", "uniq", "mid", "none"]


# ---- 1-3, 9. Q, nprobe, radii, n_values ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 4, 20, None])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_grid(ctx, corpora, metric, nprobe):
    e = corpora(metric)
    s, parent = e["s"], e["parent"] if nprobe is not None else None
    attrs = [e["attrs"][k] for k in ALL4]
    seen_hit = seen_boundary = False
    for tag, radius in _radii(e, nprobe):
        hits = _hits(e, nprobe, radius)
        want256 = _want(e, hits, ALL4, 256)
        for Q in (1, 7, 40):
            for n in ((10,) if Q != 40 else (1, 10, 256)):
                want = _cut(want256, Q, n)
                got = ctx.facet_search(parent, s, e["q"][:Q], nprobe or 1, radius, metric, attrs, n_values=n)
                _eq(got, want, (metric, nprobe, tag, Q, n))
                if tag == "none":
                    assert want[4].sum() == 0 and want[1].sum() == 0
                if tag == "all" and Q == 40:
                    assert (want[2][1] > 256).any() or nprobe == 1     # uniq: more distinct values than any n_values
                    assert (want[3][3] == want[4]).all()              # none: every hit is missing
                    assert (want[1][0][:, 0] > 64).any()                # few: many hits on one counter
                    seen_hit = True
                if tag == "boundary":
                    below = _hits(e, nprobe, np.nextafter(np.float32(radius), np.float32(-np.inf if metric == "l2" else np.inf)), 1)
                    assert len(below[0]) < len(hits[0])                 # the boundary row itself is a hit
                    seen_boundary = True
    assert seen_hit and seen_boundary
    assert ctx.last_scan_kernel() == "k_scan (facet)"


# ---- 4, 5. squared L2; total equals the lims of the range call ----------------------------------------------------------------------
def test_squared_l2_and_totals(ctx, corpora):
    e = corpora("l2")
    c, s, parent, q = e["c"], e["s"], e["parent"], e["q"]
    lims, _, dist = _pairs(e, 4)
    d64 = np.sort(dist[lims[0]:lims[1]].astype(np.float64)) ** 2
    gaps = np.nonzero(np.diff(d64) > 1e-4 * d64[1:])[0]
    j = int(gaps[gaps.shape[0] // 2])
    r2 = np.float32((d64[j] + d64[j + 1]) / 2)      # no squared distance within 1e-5 of it: sqrt(v) <= sqrt(r2) <=> v <= r2
    r = np.float32(np.sqrt(np.float64(r2)))
    attrs = [e["attrs"][k] for k in ALL4]
    want = _want(e, _hits(e, 4, r), ALL4, 10)
    assert want[4].sum() > 0
    _eq(ctx.facet_search(parent, s, q, 4, r, "l2", attrs), want, "sqrt")
    ctx.set_squared_l2(True)
    try:
        _eq(ctx.facet_search(parent, s, q, 4, r2, "l2", attrs), want, "squared")
        # a squared distance of the range result as the radius: inclusive; and total == the lims differences of the range call
        rl, _, rd = ctx.range_search(parent, s, q, 4, float("inf"), "l2")
        rb = float(np.sort(rd[rl[0]:rl[1]])[5])
        got = ctx.facet_search(parent, s, q, 4, rb, "l2", attrs)
        lims_sq = ctx.range_search(parent, s, q, 4, rb, "l2", cap=0)[0]
        np.testing.assert_array_equal(_np(got[4]), np.diff(lims_sq))
        assert got[4][0] >= 6
    finally:
        ctx.set_squared_l2(False)
    for metric in ("l2", "ip"):
        e = corpora(metric)
        for _, radius in _radii(e, 4):
            got = ctx.facet_search(e["parent"], e["s"], e["q"], 4, radius, metric, e["attrs"]["mid"])
            lims = ctx.range_search(e["parent"], e["s"], e["q"], 4, radius, metric, cap=0)[0]
            np.testing.assert_array_equal(_np(got[4]), np.diff(lims))


# ---- 6. filters -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filters(ctx, corpora, metric):
    from quake_amd.capi import Filter
    e = corpora(metric)
    c, s, parent, q, cols, attrs = e["c"], e["s"], e["parent"], e["q"][:17], e["cols"], e["attrs"]
    ids = c["ids"]
    radius = _radii(e, 4)[1][1]
    S = FY.draw_set(ids, 0.3, np.random.default_rng(311))
    where = [("mid", "between", -150000000, -150000000 + 40 * 1000003), ("few", "!=", 0)]
    any_of = [[("few", "in", [-1, int(I64MAX)])], [("mid", ">=", -150000000 + 200 * 1000003), ("few", "==", int(I64MIN))]]
    cases = [
        ("allow", Filter(s, S, "allow"), FCY.allowed_ids(ids, FY.allowed_rows(ids, S, "allow"))),
        ("deny", Filter(s, S, "deny"), FCY.allowed_ids(ids, FY.allowed_rows(ids, S, "deny"))),
        ("where", Filter.where(s, [(attrs["mid"], "range", where[0][2], where[0][3]), (attrs["few"], "not_range", 0, 0)]),
         FCY.allowed_ids(ids, AY.eval_where(where, ids, cols))),
        ("any_of", Filter.expr(s, [[(attrs["few"], "in", [-1, int(I64MAX)])],
                                   [(attrs["mid"], "range", any_of[1][0][2], int(I64MAX)), (attrs["few"], "range", int(I64MIN), int(I64MIN))]]),
         FCY.allowed_ids(ids, EY.eval_any_of(any_of, ids, cols))),
        ("nothing", Filter(s, np.array([10 ** 8], np.int64), "allow"), np.zeros(0, np.int64)),
    ]
    pids = RY.probed(q, c["cent"], c["offsets"], 4, metric)
    for tag, f, allowed in cases:
        hits = FCY.hits_search(q, c["cent"], c["vecs"], ids, c["offsets"], 4, radius, metric, allowed)
        want = _want(e, hits, ALL4, 10)
        if tag == "nothing":
            assert all(w.sum() == 0 for w in want)
        else:
            assert 0 < want[4].sum() < sum(len(h) for h in _hits(e, 4, radius, 17))
        _eq(ctx.facet_search(parent, s, q, 4, radius, metric, [attrs[k] for k in ALL4], filter=f), want, (metric, tag))
        _eq(ctx.facet_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(pids).cuda(), radius, metric, [attrs[k] for k in ALL4], filter=f),
            want, (metric, tag, "scan, device"))
        f.close()


# ---- 7. facet_scan: -1, absent and empty lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_scan_edge_pids(ctx, corpora, metric):
    e = corpora(metric)
    c, s, q, attrs = e["c"], e["s"], e["q"][:5], e["attrs"]
    sizes = np.diff(c["offsets"])
    empty = int(np.nonzero(sizes == 0)[0][0])
    edge = np.array([[5, -1, 9], [-1, -1, -1], [10 ** 6, 7, empty], [-1, 6, -1], [20, 21, 10 ** 12]], np.int64)
    radius = float("inf") if metric == "l2" else float("-inf")
    hits = FCY.hits_scan(q, c["vecs"], c["ids"], c["offsets"], np.where(edge >= 20, -1, edge), radius, metric)
    assert [len(h) > 0 for h in hits] == [True, False, True, True, False]
    want = _want(e, hits, ["few", "mid"], 10)
    _eq(ctx.facet_scan(s, q, edge, radius, metric, [attrs["few"], attrs["mid"]]), want, "edge pids")
    _eq(ctx.facet_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(edge).cuda(), radius, metric, [attrs["few"], attrs["mid"]]), want,
        "edge pids, device")


# ---- 8, 10. several columns in one call; host and device tensors ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_columns_and_memory(ctx, corpora, metric):
    e = corpora(metric)
    s, parent, q, attrs = e["s"], e["parent"], e["q"], e["attrs"]
    radius = _radii(e, 4)[1][1]
    names = ["few", "uniq", "mid", "few"]
    both = ctx.facet_search(parent, s, q, 4, radius, metric, [attrs[k] for k in names], n_values=16)
    _eq(both, _want(e, _hits(e, 4, radius), names, 16), "four columns")
    for ci, k in enumerate(names):
        one = ctx.facet_search(parent, s, q, 4, radius, metric, attrs[k], n_values=16)     # an Attr alone: C = 1
        assert one[0].shape == (1, 40, 16) and one[2].shape == (1, 40) and one[4].shape == (40,)
        for name, a, b in zip(NAMES[:4], both, one):
            np.testing.assert_array_equal(a[ci], b[0], err_msg="%s of column %d" % (name, ci))
        np.testing.assert_array_equal(both[4], one[4])
    dev = ctx.facet_search(parent, s, torch.from_numpy(q).cuda(), 4, radius, metric, [attrs[k] for k in names], n_values=16)
    assert all(t.is_cuda for t in dev)
    _eq(dev, both, "device")
    again = ctx.facet_search(parent, s, q, 4, radius, metric, [attrs[k] for k in names], n_values=16)
    for a, b in zip(both, again):
        assert a.tobytes() == b.tobytes()
    # distinct / missing / total may be NULL
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    from quake_amd.capi import metric_code
    ov, oc = np.full((1, 40, 16), -7, np.int64), np.full((1, 40, 16), -7, np.int64)
    h = (C.c_void_p * 1)(attrs["mid"].h)
    st = ctx.lib.qk_facet_search(ctx.h, parent.h, s.h, P(q), 40, 4, metric_code(metric), C.c_float(radius), None, h, 1, 16, P(ov), P(oc),
                                 None, None, None, 0, None)
    assert st == 0
    np.testing.assert_array_equal(ov[0], both[0][2])
    np.testing.assert_array_equal(oc[0], both[1][2])


# ---- 11. liveness -----------------------------------------------------------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = RY.corpus(32, 20, 6000, "l2", seed=321)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(322)
    q = RY.queries(c, 17, seed=323)
    pids = RY.probed(q, c["cent"], c["offsets"], 6, "l2")
    col = {int(i): int(i) % 12 - 6 for i in c["ids"][::2]}
    a = _attr(s, col)
    radius = 5.5

    def check(tag):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(20)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        want = FCY.expected_cols(FCY.hits_scan(q, vecs, ids, offs, pids, radius, "l2"), [col], 16)
        assert want[4].sum() > 0
        _eq(ctx.facet_scan(s, q, pids, radius, "l2", a, n_values=16), want, tag)
        return want

    w0 = check("as built")
    some = c["ids"][1::2][:800]
    for i in some:
        col[int(i)] = 1000 + int(i) % 3
    a.set(some, np.array([col[int(i)] for i in some]))
    w1 = check("set_attribute")
    assert w1[3].sum() < w0[3].sum() and (w1[0] >= 1000).any()
    s.remove_ids(c["ids"][::5])
    w2 = check("remove")
    assert w2[4].sum() < w1[4].sum()
    na = 400
    new_ids = np.arange(10 ** 6, 10 ** 6 + na, dtype=np.int64)
    lists = rng.integers(4, 20, size=na).astype(np.int64)
    new_vecs = (c["cent"][lists] + 0.3 * rng.standard_normal((na, 32))).astype(np.float32)
    lists[:17] = pids[:, 0]
    new_vecs[:17] = q + np.float32(1e-3)
    for i in new_ids[::2]:
        col[int(i)] = 777
    a.set(new_ids[::2], np.full(na // 2, 777, np.int64))
    s.add_batch(new_ids, new_vecs, lists)
    w3 = check("add, with and without values")
    assert (w3[0] == 777).any() and w3[4].sum() > w2[4].sum() and w3[3].sum() > w2[3].sum()
    a.close()
    s.close()
    parent.close()


# ---- 12. wide rows --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    c = RY.corpus(2600, 3, 300, metric, seed=331, empty=0)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 7, seed=332)
    cols = make_columns(c["ids"], 333)
    attrs = [_attr(s, cols[k]) for k in ("few", "uniq")]
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], RY.probed(q, c["cent"], c["offsets"], 2, metric), metric)
    d0 = np.sort(pairs[2][pairs[0][0]:pairs[0][1]])
    for radius in (float(d0[d0.shape[0] // 2]), float("inf") if metric == "l2" else float("-inf")):
        lims, hid, _ = RY.select(pairs, c["ids"], radius, metric)
        want = FCY.expected_cols(FCY.split(lims, hid), [cols["few"], cols["uniq"]], 10)
        assert want[4].sum() > 0
        _eq(ctx.facet_search(parent, s, q, 2, radius, metric, attrs), want, ("wide", metric, radius))
        assert ctx.last_scan_kernel() == "k_scan_wide (facet)"
    for a in attrs:
        a.close()
    s.close()
    parent.close()


# ---- 13. several passes ------------------------------------------------------------------------------------------------------------------------------
def test_passes(ctx):
    from quake_amd.capi import Store
    d, nlist, n, Q = 16, 64, 1 << 17, 1040
    rng = np.random.default_rng(341)
    sizes = np.full(nlist, (n - 9000) // (nlist - 1), np.int64)
    sizes[0] = 9000
    sizes[-1] += n - sizes.sum()
    assert sizes.sum() == n and sizes.max() >= 8192 and nlist * sizes.max() >= 1 << 19
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    vals = (rng.random(n) ** 2 * 1000).astype(np.int64) - 500            # 1000 values, skewed
    assert np.unique(vals).shape[0] == 1000
    q = rng.standard_normal((Q, d)).astype(np.float32)
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    from quake_amd.capi import Attr
    a = Attr(s)
    a.set(ids, vals)
    uv, uc = np.unique(vals, return_counts=True)
    order = np.lexsort((uv, -uc))[:10]
    ctx.set_timing(1)
    try:
        gv, gc, gd, gm, gt, tm = ctx.facet_search(None, s, q, 1, float("inf"), "l2", a, n_values=10, timing=True)
        assert tm["n_items"] >= 2
        # radius +inf and no NaN: every stored row is a hit of every query, so every query's answer is the column's histogram
        np.testing.assert_array_equal(gv[0], np.broadcast_to(uv[order], (Q, 10)))
        np.testing.assert_array_equal(gc[0], np.broadcast_to(uc[order], (Q, 10)))
        assert (gd == 1000).all() and (gm == 0).all() and (gt == n).all()
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 15. limits at the C level ------------------------------------------------------------------------------------------------------------------------
def test_limits(ctx, corpora):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter
    e, e2 = corpora("l2"), corpora("ip")
    s, parent, q, attrs = e["s"], e["parent"], e["q"][:5], e["attrs"]
    mid = attrs["mid"]
    plain = ctx.facet_search(parent, s, q, 4, 6.0, "l2", mid)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*n_cols=0"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", [])
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*n_cols=5"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", [mid] * 5)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*n_values=0"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", mid, n_values=0)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*n_values=257"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", mid, n_values=257)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", [mid, e2["attrs"]["mid"]])
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", [mid, None])
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*NaN"):
        ctx.facet_search(parent, s, q, 4, float("nan"), "l2", mid)
    f2 = Filter(e2["s"], e2["c"]["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.facet_search(parent, s, q, 4, 6.0, "l2", mid, filter=f2)
    f2.close()
    pids = RY.probed(q, e["c"]["cent"], e["c"]["offsets"], 4, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*n_values=257"):
        ctx.facet_scan(s, q, pids, 6.0, "l2", mid, n_values=257)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*n_cols=0"):
        ctx.facet_scan(s, q, pids, 6.0, "l2", [])
    # Q == 0 is served
    empty = ctx.facet_search(parent, s, q[:0], 4, 6.0, "l2", mid)
    assert empty[0].shape == (1, 0, 10) and empty[4].shape == (0,)
    # the context still answers, and answers the same
    _eq(ctx.facet_search(parent, s, q, 4, 6.0, "l2", mid), plain, "after the refusals")
    _eq(ctx.facet_scan(s, q, pids, 6.0, "l2", mid), plain, "scan")


# ---- 14, 16. the mirrors ------------------------------------------------------------------------------------------------------------------------------
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
    return (r.values, r.counts, r.distinct, r.missing, r.totals)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(qb, metric, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(351)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(17, d, generator=g)
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(352)))
    idx = _build(quake, x, ids, 20, metric)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    before = repr(quake.SearchParams())
    for m in (idx, loaded):
        m.set_attribute("cat", ids[::2], ids[::2] % 7 - 3)
        m.set_attribute("doc", ids, ids * 3 - 9000)
    sp, spc = quake.SearchParams(), qb.SearchParams()
    for p in (sp, spc):
        p.nprobe, p.k = 5, 3
    store_of = lambda: (idx.parent._store if idx.parent is not None else None, idx._store)  # noqa: E731
    radius = 7.5 if metric == "l2" else 0.5

    def compare(tag):
        for exclude in (None, True):
            sp.filter = None if exclude is None else idx.make_filter(S, exclude)
            spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
            for rad, n_values in ((None, 10), (radius, 4)):
                r = idx.facet_counts(q, ["cat", "doc"], sp, radius=rad, n_values=n_values)
                inf = float("inf") if metric == "l2" else float("-inf")
                base = idx._ctx.facet_search(*store_of(), q.numpy(), 5, inf if rad is None else rad, metric,
                                             [idx._attributes()["cat"], idx._attributes()["doc"]], n_values=n_values,
                                             filter=sp.filter._h if sp.filter is not None else None)
                _eq(_res(r), base, ("python", tag, exclude, rad))
                assert r.columns == ["cat", "doc"] and r.values.shape == (2, 17, n_values) and r.timing_info.n_queries == 17
                tot = r.totals.numpy()
                assert tot.sum() > 0 and (rad is None or tot.sum() < _np(idx.facet_counts(q, "cat", sp).totals).sum())
                np.testing.assert_array_equal(r.distinct[1].numpy() + r.missing[1].numpy(), tot)  # doc: a value of its own per vector
                if n_values >= 8:
                    np.testing.assert_array_equal(r.counts[0].numpy().sum(1) + r.missing[0].numpy(), tot)
                rd = idx.facet_counts(q.cuda(), ["cat", "doc"], sp, radius=rad, n_values=n_values)
                assert all(t.is_cuda for t in _res(rd))
                _eq(_res(rd), base, ("python, device", tag, exclude, rad))
                for xq in (q, q.cuda()):
                    rc = loaded.facet_counts(xq, ["cat", "doc"], spc, radius=rad, n_values=n_values)
                    assert rc.values.is_cuda == xq.is_cuda and rc.totals.is_cuda == xq.is_cuda and list(rc.columns) == ["cat", "doc"]
                    _eq(_res(rc), base, ("compiled", tag, exclude, rad, xq.is_cuda))
            one, onec = idx.facet_counts(q, "cat", sp), loaded.facet_counts(q, "cat", spc)           # a name alone: C = 1
            assert tuple(one.values.shape) == (1, 17, 10) and one.columns == ["cat"]
            _eq(_res(onec), [t.numpy() for t in _res(one)], ("one column", tag, exclude))
        sp.filter = spc.filter = None

    compare("as built")
    xa = torch.randn(300, d, generator=g)
    ia = torch.arange(300) + 10 ** 6
    for m in (idx, loaded):
        m.add(xa, ia)
        m.set_attribute("cat", ia[:150], torch.full((150,), 99))
    compare("add")
    for m in (idx, loaded):
        m.remove(ids[:1500])
    compare("remove")
    assert "facet" not in before and repr(quake.SearchParams()) == before
    for m, p in ((idx, sp), (loaded, spc)):
        empty = m.facet_counts(q[:0], ["cat", "doc"], p, n_values=4)
        assert tuple(empty.values.shape) == (2, 0, 4) and tuple(empty.distinct.shape) == (2, 0) and tuple(empty.totals.shape) == (0,)


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(361)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        idx.set_attribute("doc", ids, ids % 50)
        fresh = lambda: mod.SearchParams()  # noqa: E731

        def params(**kw):
            sp = fresh()
            sp.k, sp.nprobe = 5, 4
            for k, v in kw.items():
                setattr(sp, k, v)
            return sp

        plain = idx.facet_counts(qq, "doc", params(), radius=5.0)
        assert plain.totals.sum() > 0
        for kw, match in ((dict(recall_target=0.9), "recall_target"),
                          (dict(filters=[idx.make_filter(ids[:1000])], query_filter=torch.zeros(10, dtype=torch.int32)), "query_filter"),
                          (dict(max_nprobe=8), "max_nprobe"),
                          (dict(filter_exact_rows=100, filter=idx.make_filter(ids[:50])), "filter_exact_rows"),
                          (dict(filters_exact_rows=100), "filters_exact_rows"),
                          (dict(filter=other.make_filter(ids[:1000])), "another index")):
            with pytest.raises(RuntimeError, match=match):
                idx.facet_counts(qq, "doc", params(**kw), radius=5.0)
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.facet_counts(qq, ["doc", "nope"], params(), radius=5.0)
        with pytest.raises(RuntimeError, match="NaN"):
            idx.facet_counts(qq, "doc", params(), radius=float("nan"))
        for n_values in (0, 257):
            with pytest.raises(RuntimeError, match="n_values"):
                idx.facet_counts(qq, "doc", params(), radius=5.0, n_values=n_values)
        for names in ([], ["doc"] * 5):
            with pytest.raises(RuntimeError, match="between 1 and 4 columns"):
                idx.facet_counts(qq, names, params(), radius=5.0)
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.facet_counts(qq, "doc", params(), radius=5.0)
        again = idx.facet_counts(qq, "doc", params(), radius=5.0)
        for a, b in zip(_res(again), _res(plain)):
            assert torch.equal(a, b)
