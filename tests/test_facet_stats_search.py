"""Facet statistics (qk_facet_stats_search / qk_facet_stats_scan; Context.facet_stats_search / facet_stats_scan;
QuakeIndex.facet_stats in both mirrors): per query, count / missing / min / max / exact sum / histogram of attribute columns over
the hits of the range call with the same arguments.

Every comparison is exact integer equality of all eight outputs -- count, missing, min, max, sum_lo, sum_hi, hist, total -- with
tests/facet_stats_yardstick.py (pinned on the CPU by tests/test_facet_stats_oracle.py), whose hits are tests/range_yardstick.py's.
No assertion reads a clock.  Every test asserts on its own inputs that the situation it is about occurs.  The corpus, columns and
queries are those of tests/test_facet_search.py, rebuilt here."""
import ctypes as C

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import expr_yardstick as EY
import facet_stats_yardstick as FSY
import facet_yardstick as FCY
import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
NAMES = FSY.NAMES
FC_SLICE = 1024      # keys per workgroup step of k_facet_stats (quake_amd/csrc/qk_facet.hip)


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    assert len(got) >= 8
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(_np(g), _np(w), err_msg="%s %s" % (name, tag))


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
    """the four columns of tests/test_facet_search.py as dicts id -> value: few (5 values, the extremes and -1, on 95 % of the
    ids), uniq (a value of its own per id), mid (about 300 values, skewed), none (values only for ids that are not stored)"""
    rng = np.random.default_rng(seed)
    few_vals = np.array(FEW, np.int64)
    pick = rng.random(ids.shape[0]) < 0.95
    few = {int(i): int(v) for i, v in zip(ids[pick], few_vals[rng.integers(0, 5, size=int(pick.sum()))])}
    uniq = {int(i): _uniq_value(i) for i in ids}
    skew = np.minimum((rng.random(ids.shape[0]) ** 3 * 300).astype(np.int64), 299) * 1000003 - 150000000
    mid = {int(i): int(v) for i, v in zip(ids, skew)}
    none = {int(i): int(i) % 9 for i in range(50000, 50050)}
    return dict(few=few, uniq=uniq, mid=mid, none=none)


def _edges255(seed):
    rng = np.random.default_rng(seed)
    e = sorted({int(x) for x in rng.integers(I64MIN, I64MAX, size=400, endpoint=True)})[:255]
    assert len(e) == 255
    return e


MID_EDGES = [-150000000 + k * 1000003 for k in (0, 1, 2, 5, 40, 41, 150, 299)]   # every one of them a value of `mid`
ALL4 = ["few", "uniq", "mid", "none"]
EDGES4 = [FEW, _edges255(7)[::16], None, [0]]      # 5, 16, 0 and 1 edges: hist_stride 17, three columns padded


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
            assert all(v in set(cols["mid"].values()) for v in MID_EDGES[:3])
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
        e["hits"][key] = (RY.all_pairs(e["q"], c["vecs"], c["ids"], c["offsets"], pids, c["metric"]), pids)
    return e["hits"][key]


def _hits(e, nprobe, radius, Q=40):
    lims, hid, _ = RY.select(_pairs(e, nprobe)[0], e["c"]["ids"], radius, e["c"]["metric"])
    return FCY.split(lims, hid)[:Q]


def _norm(edges, n):
    """per-column edge lists of a call's `edges` argument for n columns"""
    if edges is None:
        return [[] for _ in range(n)]
    if len(edges) and all(x is None or isinstance(x, (list, tuple)) for x in edges):
        return [list(x) if x is not None else [] for x in edges]
    return [list(edges) for _ in range(n)]


def _want(e, hits, names, edges):
    return FSY.expected_cols(hits, [e["cols"][k] for k in names], _norm(edges, len(names)))


def _radii(e, nprobe):
    """(tag, radius): one no row passes, one that IS a distance of the first query and keeps about half of its probed rows (the
    boundary row is a hit), everything"""
    metric = e["c"]["metric"]
    lims, _, dist = _pairs(e, nprobe)[0]
    mine = dist[lims[0]:lims[1]]
    mine = np.sort(mine[~np.isnan(mine)])
    r = mine[mine.shape[0] // 2] if metric == "l2" else mine[-(mine.shape[0] // 2) - 1]
    assert (mine == r).sum() >= 1
    return [("none", -1.0 if metric == "l2" else 1e30), ("half", float(r)), ("all", float("inf") if metric == "l2" else float("-inf"))]


# ---- 1, 3. the grid: metric, search and scan, nprobe, radius; the `none` column ----------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 3, None])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_grid(ctx, corpora, metric, nprobe):
    e = corpora(metric)
    c, s, q = e["c"], e["s"], e["q"]
    parent = e["parent"] if nprobe is not None else None
    attrs = [e["attrs"][k] for k in ALL4]
    pids = _pairs(e, nprobe)[1]
    pids = np.broadcast_to(pids, (40, pids.shape[-1])) if pids.ndim == 1 else pids
    seen_big = False
    for tag, radius in _radii(e, nprobe):
        hits = _hits(e, nprobe, radius)
        want = _want(e, hits, ALL4, EDGES4)
        for Q in (1, 40):
            wq = [w[:, :Q] for w in want[:7]] + [want[7][:Q]]
            _eq(ctx.facet_stats_search(parent, s, q[:Q], nprobe or 1, radius, metric, attrs, edges=EDGES4), wq, (metric, nprobe, tag, Q))
            assert ctx.last_scan_kernel() == "k_scan (facet stats)"
            _eq(ctx.facet_stats_scan(s, q[:Q], pids[:Q], radius, metric, attrs, edges=EDGES4), wq, (metric, nprobe, tag, Q, "scan"))
        count, missing, vmin, vmax, lo, hi, hist, total, sums = want
        assert hist.shape == (4, 40, 17) and (hist.sum(2) == count).all() and (count + missing == total[None, :]).all()
        # the `none` column: no hit has a value
        assert (count[3] == 0).all() and (missing[3] == total).all() and (vmin[3] == I64MAX).all() and (vmax[3] == I64MIN).all()
        assert (lo[3] == 0).all() and (hi[3] == 0).all() and (hist[3] == 0).all()
        if tag == "none":
            assert total.sum() == 0
        if tag == "half":
            assert 0 < total[0] < len(_hits(e, nprobe, _radii(e, nprobe)[2][1], 1)[0])
            below = _hits(e, nprobe, np.nextafter(np.float32(radius), np.float32(-np.inf if metric == "l2" else np.inf)), 1)
            assert len(below[0]) < len(hits[0])                             # the boundary row itself is a hit
        if tag == "all":
            assert (missing[0] > 0).any()                                     # few: ids without a value
            if nprobe is None:
                assert (hist[0, :, 1:6] > 0).all()                            # every value of few occurs, each in its own bucket
                # every query's segment is the whole store: several slices, handed to several workgroups
                assert (total == 6000).all() and 6000 > 2 * FC_SLICE
                assert any(not I64MIN <= x <= I64MAX for x in sums[0])        # few: an exact sum outside int64
                assert (hi[0] != 0).any() and (hi[0] != -1).any()
                seen_big = True
    assert seen_big or nprobe is not None


# ---- 2. edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_edges(ctx, corpora, metric):
    e = corpora(metric)
    s, parent, q, attrs = e["s"], e["parent"], e["q"], e["attrs"]
    radius = _radii(e, 4)[1][1]
    hits = _hits(e, 4, radius)
    assert sum(len(h) for h in hits) > 1000
    e255 = _edges255(11)
    cases = [
        (["uniq"], None), (["uniq"], [0]), (["uniq"], e255), (["mid"], MID_EDGES), (["few"], FEW),
        (["few"], [I64MIN]), (["few"], [I64MAX]), (["few"], [I64MIN, I64MAX]), (["uniq"], [I64MIN, I64MAX]),
        (["few", "uniq", "mid", "uniq"], [FEW, None, e255, [1]]),            # 5 / 0 / 255 / 1 edges: hist_stride 256, padding
        (["mid", "mid"], [MID_EDGES, [MID_EDGES[3] + 1]]),                   # the same column twice with different edges
        (["uniq", "mid"], [[], e255[:64]]),
        (ALL4, e255[:100:3]),                                                # four columns, one sequence for all
    ]
    for names, edges in cases:
        want = _want(e, hits, names, edges)
        got = ctx.facet_stats_search(parent, s, q, 4, radius, metric, [attrs[k] for k in names], edges=edges)
        _eq(got, want, (metric, names, "edges", None if edges is None else len(edges)))
        assert got[6].shape == want[6].shape and (want[6].sum(2) == want[0]).all()
    w = _want(e, hits, ["few"], [I64MIN])
    assert (w[6][0, :, 0] == 0).all() and w[6][0, :, 1].sum() > 0             # nothing lies below INT64_MIN
    w = _want(e, hits, ["few"], [I64MAX])
    assert (w[6][0, :, 1] > 0).any() and (w[6][0, :, 0] > 0).any()            # INT64_MAX itself lies right of the edge INT64_MAX
    w = _want(e, hits, ["mid"], MID_EDGES)
    assert (w[6][0, :, 1] > 0).any() and (w[6][0, :, 0] == 0).all()           # a value equal to the first edge: bucket 1, not 0


# ---- 4. filters ---------------------------------------------------------------------------------------------------------------------
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
    unfiltered = sum(len(h) for h in _hits(e, 4, radius, 17))
    for tag, f, allowed in cases:
        hits = FCY.hits_search(q, c["cent"], c["vecs"], ids, c["offsets"], 4, radius, metric, allowed)
        want = _want(e, hits, ALL4, EDGES4)
        if tag == "nothing":
            assert want[7].sum() == 0
        else:
            assert 0 < want[7].sum() < unfiltered
        _eq(ctx.facet_stats_search(parent, s, q, 4, radius, metric, [attrs[k] for k in ALL4], edges=EDGES4, filter=f), want, (metric, tag))
        _eq(ctx.facet_stats_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(pids).cuda(), radius, metric, [attrs[k] for k in ALL4],
                                 edges=EDGES4, filter=f), want, (metric, tag, "scan, device"))
        f.close()


# ---- 5. the histogram over a column's own values is its facet counts -------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_agrees_with_facet_counts_on_the_device(ctx, corpora, metric):
    e = corpora(metric)
    s, parent, q, few = e["s"], e["parent"], e["q"], e["attrs"]["few"]
    radius = _radii(e, 4)[1][1]
    st = ctx.facet_stats_search(parent, s, q, 4, radius, metric, few, edges=FEW)
    fv, fc, fd, fm, ft = ctx.facet_search(parent, s, q, 4, radius, metric, few, n_values=8)
    assert ft.sum() > 0 and (fd[0] >= 4).any()
    for qi in range(40):
        counts = dict(zip(fv[0, qi, :fd[0, qi]].tolist(), fc[0, qi, :fd[0, qi]].tolist()))
        assert st[6][0, qi, 1:].tolist() == [counts.get(v, 0) for v in FEW] and st[6][0, qi, 0] == 0
    np.testing.assert_array_equal(st[1], fm)
    np.testing.assert_array_equal(st[7], ft)


# ---- 6. squared L2; total equals the lims of the range call -----------------------------------------------------------------------------
def test_squared_l2_and_totals(ctx, corpora):
    e = corpora("l2")
    s, parent, q = e["s"], e["parent"], e["q"]
    lims, _, dist = _pairs(e, 4)[0]
    d64 = np.sort(dist[lims[0]:lims[1]].astype(np.float64)) ** 2
    gaps = np.nonzero(np.diff(d64) > 1e-4 * d64[1:])[0]
    j = int(gaps[gaps.shape[0] // 2])
    r2 = np.float32((d64[j] + d64[j + 1]) / 2)      # no squared distance within 1e-5 of it: sqrt(v) <= sqrt(r2) <=> v <= r2
    r = np.float32(np.sqrt(np.float64(r2)))
    attrs = [e["attrs"][k] for k in ALL4]
    want = _want(e, _hits(e, 4, r), ALL4, EDGES4)
    assert want[7].sum() > 0
    _eq(ctx.facet_stats_search(parent, s, q, 4, r, "l2", attrs, edges=EDGES4), want, "sqrt")
    ctx.set_squared_l2(True)
    try:
        _eq(ctx.facet_stats_search(parent, s, q, 4, r2, "l2", attrs, edges=EDGES4), want, "squared")
        rl, _, rd = ctx.range_search(parent, s, q, 4, float("inf"), "l2")
        rb = float(np.sort(rd[rl[0]:rl[1]])[5])    # a squared distance of the range result as the radius: inclusive
        got = ctx.facet_stats_search(parent, s, q, 4, rb, "l2", attrs)
        np.testing.assert_array_equal(_np(got[7]), np.diff(ctx.range_search(parent, s, q, 4, rb, "l2", cap=0)[0]))
        assert got[7][0] >= 6
    finally:
        ctx.set_squared_l2(False)
    for metric in ("l2", "ip"):
        e = corpora(metric)
        for _, radius in _radii(e, 4):
            got = ctx.facet_stats_search(e["parent"], e["s"], e["q"], 4, radius, metric, e["attrs"]["mid"])
            lims = ctx.range_search(e["parent"], e["s"], e["q"], 4, radius, metric, cap=0)[0]
            np.testing.assert_array_equal(_np(got[7]), np.diff(lims))


# ---- 7. facet_stats_scan: -1, absent and empty lists, a list named twice -------------------------------------------------------------------
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
    want = _want(e, hits, ["few", "mid"], [FEW, MID_EDGES])
    _eq(ctx.facet_stats_scan(s, q, edge, radius, metric, [attrs["few"], attrs["mid"]], edges=[FEW, MID_EDGES]), want, "edge pids")
    _eq(ctx.facet_stats_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(edge).cuda(), radius, metric, [attrs["few"], attrs["mid"]],
                             edges=[FEW, MID_EDGES]), want, "edge pids, device")
    # a list named twice: the hits are BY DEFINITION those of range_scan for the same pids
    big = int(np.argmax(sizes))
    twice = np.array([[big, 5, big]] * 5, np.int64)
    rl, rids, _ = ctx.range_scan(s, q, twice, radius, metric)
    want = _want(e, FCY.split(rl, rids), ["few", "mid"], [FEW, MID_EDGES])
    got = ctx.facet_stats_scan(s, q, twice, radius, metric, [attrs["few"], attrs["mid"]], edges=[FEW, MID_EDGES])
    _eq(got, want, "a list named twice")
    np.testing.assert_array_equal(got[7], np.diff(rl))
    assert (np.diff(rl) >= sizes[big]).all()


# ---- 8. liveness ---------------------------------------------------------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = RY.corpus(32, 20, 6000, "l2", seed=321)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(322)
    q = RY.queries(c, 17, seed=323)
    pids = RY.probed(q, c["cent"], c["offsets"], 6, "l2")
    col = {int(i): int(i) % 12 - 6 for i in c["ids"][::2]}
    a = _attr(s, col)
    radius = 5.5
    edges = [-3, 0, 3, 500, 1001]

    def check(tag):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(20)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        want = FSY.expected_cols(FCY.hits_scan(q, vecs, ids, offs, pids, radius, "l2"), [col], [edges])
        assert want[7].sum() > 0
        _eq(ctx.facet_stats_scan(s, q, pids, radius, "l2", a, edges=edges), want, tag)
        return want

    w0 = check("as built")
    assert w0[3].max() == 5 and w0[2].min() == -6 and w0[6][0, :, 4:].sum() == 0
    some = c["ids"][1::2][:800]
    for i in some:
        col[int(i)] = 1000 + int(i) % 3
    a.set(some, np.array([col[int(i)] for i in some]))
    w1 = check("set_attribute")
    assert w1[1].sum() < w0[1].sum() and w1[3].max() == 1002 and w1[6][0, :, 4].sum() > 0 and w1[6][0, :, 5].sum() > 0
    assert sum(w1[8][0]) > sum(w0[8][0])
    gone = some[:400]
    for i in gone:
        del col[int(i)]
    a.unset(gone)
    w2 = check("unset")
    assert w2[1].sum() > w1[1].sum() and sum(w2[8][0]) < sum(w1[8][0]) and w2[6][0].sum() < w1[6][0].sum()
    s.remove_ids(c["ids"][::5])
    w3 = check("remove")
    assert w3[7].sum() < w2[7].sum()
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
    assert (w4[2] == -777).any() and w4[7].sum() > w3[7].sum() and w4[1].sum() > w3[1].sum()
    a.close()
    s.close()
    parent.close()


# ---- 9. wide rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    c = RY.corpus(2600, 3, 300, metric, seed=331, empty=0)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 7, seed=332)
    cols = make_columns(c["ids"], 333)
    attrs = [_attr(s, cols[k]) for k in ("few", "uniq")]
    edges = [FEW, _edges255(13)[::5]]
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], RY.probed(q, c["cent"], c["offsets"], 2, metric), metric)
    d0 = np.sort(pairs[2][pairs[0][0]:pairs[0][1]])
    for radius in (float(d0[d0.shape[0] // 2]), float("inf") if metric == "l2" else float("-inf")):
        lims, hid, _ = RY.select(pairs, c["ids"], radius, metric)
        want = FSY.expected_cols(FCY.split(lims, hid), [cols["few"], cols["uniq"]], edges)
        assert want[7].sum() > 0
        _eq(ctx.facet_stats_search(parent, s, q, 2, radius, metric, attrs, edges=edges), want, ("wide", metric, radius))
        assert ctx.last_scan_kernel() == "k_scan_wide (facet stats)"
    for a in attrs:
        a.close()
    s.close()
    parent.close()


# ---- 10. several passes -------------------------------------------------------------------------------------------------------------------------
def test_passes(ctx):
    from quake_amd.capi import Attr, Store
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
    vals = rng.integers(I64MIN // 4, I64MAX // 4, size=n).astype(np.int64)     # 2^17 values of about 2^61: the sum leaves int64
    vals[:3] = [I64MIN, I64MAX, -1]
    edges = sorted({int(x) for x in rng.integers(I64MIN // 4, I64MAX // 4, size=40)})
    q = rng.standard_normal((Q, d)).astype(np.float32)
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    a = Attr(s)
    a.set(ids, vals)
    total = sum(int(v) for v in vals)
    assert not I64MIN <= total <= I64MAX
    hi, lo = FSY.split128(total)
    hist = np.bincount(np.searchsorted(np.array(edges, np.int64), vals, side="right"), minlength=len(edges) + 1)
    ctx.set_timing(1)
    try:
        cnt, mis, vmin, vmax, slo, shi, gh, tot, tm = ctx.facet_stats_search(None, s, q, 1, float("inf"), "l2", a, edges=edges, timing=True)
        assert tm["n_items"] >= 2
        # radius +inf and no NaN: every stored row is a hit of every query, so every query's answer is the column's own statistics
        assert (cnt == n).all() and (mis == 0).all() and (tot == n).all() and (vmin == I64MIN).all() and (vmax == I64MAX).all()
        assert (slo == lo).all() and (shi == hi).all()
        np.testing.assert_array_equal(gh[0], np.broadcast_to(hist, (Q, len(edges) + 1)))
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 11, 14. device and host memory, NULL outputs, determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_memory_null_outputs_and_determinism(ctx, corpora, metric):
    from quake_amd.capi import metric_code
    e = corpora(metric)
    s, parent, q, attrs = e["s"], e["parent"], e["q"], e["attrs"]
    radius = _radii(e, 4)[1][1]
    names = ["few", "uniq", "mid", "few"]
    edges = [FEW, _edges255(17)[:40], MID_EDGES, [0]]
    cols = [attrs[k] for k in names]
    host = ctx.facet_stats_search(parent, s, q, 4, radius, metric, cols, edges=edges)
    _eq(host, _want(e, _hits(e, 4, radius), names, edges), "host")
    assert host[7].sum() > 0
    dev = ctx.facet_stats_search(parent, s, torch.from_numpy(q).cuda(), 4, radius, metric, cols, edges=edges)
    assert all(t.is_cuda for t in dev)
    _eq(dev, host, "device")
    again = ctx.facet_stats_search(parent, s, q, 4, radius, metric, cols, edges=edges)
    for a, b in zip(host, again):
        assert a.tobytes() == b.tobytes()
    again = ctx.facet_stats_search(parent, s, torch.from_numpy(q).cuda(), 4, radius, metric, cols, edges=edges)
    torch.cuda.synchronize()   # (the context's stream is its own: torch reads the results behind a device-wide wait)
    for a, b in zip(dev, again):
        assert torch.equal(a, b)
    one = ctx.facet_stats_search(parent, s, q, 4, radius, metric, attrs["mid"], edges=MID_EDGES)      # an Attr alone: C = 1
    assert one[0].shape == (1, 40) and one[6].shape == (1, 40, len(MID_EDGES) + 1) and one[7].shape == (40,)
    for k in range(6):
        np.testing.assert_array_equal(one[k][0], host[k][2])
    np.testing.assert_array_equal(one[6][0], host[6][2][:, :len(MID_EDGES) + 1])
    # every output but total may be NULL, each on its own -- in host and in device memory
    P = lambda a: C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())  # noqa: E731
    harr = (C.c_void_p * 4)(*[a.h for a in cols])
    flat = [x for l in edges for x in l]
    earr, narr = (C.c_int64 * len(flat))(*flat), (C.c_int * 4)(*[len(l) for l in edges])
    for mem, xq in ((0, q), (1, torch.from_numpy(q).cuda())):
        for skip in range(8):
            if mem == 0:
                bufs = [np.full(h.shape, -7, np.int64) for h in host]
            else:
                bufs = [torch.full(tuple(h.shape), -7, dtype=torch.int64, device="cuda") for h in host]
            ptrs = [None if (k == skip and k != 7) else P(b) for k, b in enumerate(bufs)]
            st = ctx.lib.qk_facet_stats_search(ctx.h, parent.h, s.h, P(xq), 40, 4, metric_code(metric), C.c_float(radius), None, harr, 4,
                                               earr, narr, *ptrs, mem, None)
            assert st == 0
            for k in range(8):
                if k == skip and k != 7:
                    assert (_np(bufs[k]) == -7).all()
                else:
                    np.testing.assert_array_equal(_np(bufs[k]), host[k], err_msg="%s with output %d NULL, mem %d" % (NAMES[k], skip, mem))
    # edges and n_edges both NULL: no histogram, or the single bucket
    bufs = [np.full(h.shape, -7, np.int64) for h in host[:6]] + [np.full((4, 40, 1), -7, np.int64), np.full(40, -7, np.int64)]
    st = ctx.lib.qk_facet_stats_search(ctx.h, parent.h, s.h, P(q), 40, 4, metric_code(metric), C.c_float(radius), None, harr, 4, None, None,
                                       *[P(b) for b in bufs], 0, None)
    assert st == 0
    np.testing.assert_array_equal(bufs[6][:, :, 0], host[0])
    np.testing.assert_array_equal(bufs[2], host[2])


# ---- 12. limits and errors at the C level ---------------------------------------------------------------------------------------------------------
def test_limits(ctx, corpora):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter, Store, metric_code
    e, e2 = corpora("l2"), corpora("ip")
    s, parent, q, attrs = e["s"], e["parent"], e["q"][:5], e["attrs"]
    mid = attrs["mid"]
    plain = ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", mid, edges=MID_EDGES)
    assert plain[7].sum() > 0
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*n_cols=0"):
        ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", [])
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*n_cols=5"):
        ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", [mid] * 5)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", [mid, e2["attrs"]["mid"]])
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", [mid, None])
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*NaN"):
        ctx.facet_stats_search(parent, s, q, 4, float("nan"), "l2", mid)
    f2 = Filter(e2["s"], e2["c"]["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", mid, filter=f2)
    f2.close()
    pids = RY.probed(q, e["c"]["cent"], e["c"]["offsets"], 4, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*n_cols=0"):
        ctx.facet_stats_scan(s, q, pids, 6.0, "l2", [])
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*n_cols=5"):
        ctx.facet_stats_scan(s, q, pids, 6.0, "l2", [mid] * 5)
    # the edge errors of the C ABI itself (the wrapper's lower_edges would refuse them first)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    out = [np.zeros((1, 5), np.int64) for _ in range(6)] + [np.zeros((1, 5, 300), np.int64), np.zeros(5, np.int64)]
    harr = (C.c_void_p * 1)(mid.h)

    def raw(edges, n_edges, search=True, total=True):
        earr = (C.c_int64 * max(len(edges), 1))(*edges) if edges is not None else None
        narr = (C.c_int * 1)(n_edges) if n_edges is not None else None
        ptrs = [P(b) for b in out[:7]] + [P(out[7]) if total else None]
        if search:
            st = ctx.lib.qk_facet_stats_search(ctx.h, parent.h, s.h, P(q), 5, 4, metric_code("l2"), C.c_float(6.0), None, harr, 1, earr, narr,
                                               *ptrs, 0, None)
        else:
            st = ctx.lib.qk_facet_stats_scan(ctx.h, s.h, P(q), 5, P(pids), 4, metric_code("l2"), C.c_float(6.0), None, harr, 1, earr, narr,
                                             *ptrs, 0, None)
        return st, ctx.lib.qk_last_error().decode()

    QK_ERR_INVALID, QK_ERR_UNSUPPORTED = 1, 4      # (include/quake_hip.h)
    for search in (True, False):
        assert raw([1, 2, 3], 3, search)[0] == 0
        st, msg = raw([1], -1, search)
        assert st == QK_ERR_INVALID and "negative" in msg
        st, msg = raw(list(range(256)), 256, search)
        assert st == QK_ERR_UNSUPPORTED and "QK_MAX_FACET_EDGES" in msg
        assert raw(list(range(255)), 255, search)[0] == 0
        for bad in ([1, 1], [2, 1], [0, 5, 5], [I64MAX, I64MIN]):
            st, msg = raw(bad, len(bad), search)
            assert st == QK_ERR_INVALID and "strictly ascending" in msg
        assert raw(None, 2, search)[0] == QK_ERR_INVALID and raw([1, 2], None, search)[0] == QK_ERR_INVALID
        assert raw(None, 0, search)[0] == 0 and raw(None, None, search)[0] == 0
        assert raw(None, None, search, total=False)[0] == QK_ERR_INVALID
    # Q == 0 is served
    empty = ctx.facet_stats_search(parent, s, q[:0], 4, 6.0, "l2", mid, edges=MID_EDGES)
    assert empty[0].shape == (1, 0) and empty[6].shape == (1, 0, len(MID_EDGES) + 1) and empty[7].shape == (0,)
    # no lists probed: a store without lists -- every count zero, min / max at their identities
    bare = Store(ctx, 32)
    ab = _attr(bare, {1: 1})
    got = ctx.facet_stats_search(None, bare, q, 1, 6.0, "l2", ab, edges=[0])
    assert all((got[k] == 0).all() for k in (0, 1, 4, 5, 6, 7)) and (got[2] == I64MAX).all() and (got[3] == I64MIN).all()
    ab.close()
    bare.close()
    # the context still answers, and answers the same
    _eq(ctx.facet_stats_search(parent, s, q, 4, 6.0, "l2", mid, edges=MID_EDGES), plain, "after the refusals")
    _eq(ctx.facet_stats_scan(s, q, pids, 6.0, "l2", mid, edges=MID_EDGES), plain, "scan")


# ---- 13. the mirrors -------------------------------------------------------------------------------------------------------------------------------
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
    return (r.count, r.missing, r.min, r.max, r.sum_lo, r.sum_hi, r.histogram, r.totals)


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
    cat = {int(i): int(i) % 7 - 3 for i in ids[::2]}
    big = {int(i): (int(i) * 3 + 1000) * (1 << 48) for i in ids}        # positive values up to 2^62.3: a few hits leave int64
    assert max(big.values()) <= I64MAX

    def set_attributes(m):
        m.set_attribute("cat", ids[::2], ids[::2] % 7 - 3)
        m.set_attribute("big", ids, (ids * 3 + 1000) * (1 << 48))

    set_attributes(idx)
    set_attributes(loaded)
    sp, spc = quake.SearchParams(), qb.SearchParams()
    for p in (sp, spc):
        p.nprobe, p.k = 5, 3
    radius = 7.5 if metric == "l2" else 0.5
    edges = {"cat": [-3, 0, 1, 3], "big": [1 << 60, 1 << 61, 1 << 62]}
    per = [edges["cat"], edges["big"]]
    stored = {"ids": ids.numpy().copy(), "x": x.numpy().copy()}

    def compare(tag):
        for exclude in (None, True):
            sp.filter = None if exclude is None else idx.make_filter(S, exclude)
            spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
            for rad in (None, radius):
                r = idx.facet_stats(q, ["cat", "big"], sp, radius=rad, edges=edges)
                inf = float("inf") if metric == "l2" else float("-inf")
                rl, rids, _ = idx._ctx.range_search(idx.parent._store if idx.parent is not None else None, idx._store, q.numpy(), 5,
                                                    inf if rad is None else rad, metric, filter=sp.filter._h if sp.filter is not None else None)
                # the yardstick over the hit ids of the range call (the index's own k-means decides the lists)
                want = FSY.expected_cols(FCY.split(rl, rids), [cat, big], per)
                _eq(_res(r), want, ("python", tag, exclude, rad))
                assert r.columns == ["cat", "big"] and r.edges == per and r.timing_info.n_queries == 17
                assert tuple(r.histogram.shape) == (2, 17, 5) and r.totals.sum() > 0
                assert r.sums() == want[8]
                if rad is None and exclude is None:
                    assert any(not I64MIN <= v <= I64MAX for v in want[8][1])
                means = r.means()
                cnt = want[0]
                assert means.shape == (2, 17) and means.dtype == np.float64
                for c in range(2):
                    for qi in range(17):
                        assert (np.isnan(means[c, qi]) if cnt[c, qi] == 0 else means[c, qi] == want[8][c][qi] / int(cnt[c, qi]))
                rd = idx.facet_stats(q.cuda(), ["cat", "big"], sp, radius=rad, edges=edges)
                assert all(t.is_cuda for t in _res(rd))
                _eq(_res(rd), want, ("python, device", tag, exclude, rad))
                for xq in (q, q.cuda()):
                    rc = loaded.facet_stats(xq, ["cat", "big"], spc, radius=rad, edges=edges)
                    assert rc.count.is_cuda == xq.is_cuda and rc.totals.is_cuda == xq.is_cuda and list(rc.columns) == ["cat", "big"]
                    assert [list(l) for l in rc.edges] == per
                    _eq(_res(rc), want, ("compiled", tag, exclude, rad, xq.is_cuda))
                    assert rc.sums() == want[8] and np.array_equal(rc.means(), means, equal_nan=True)
            one, onec = idx.facet_stats(q, "cat", sp, edges=[0]), loaded.facet_stats(q, "cat", spc, edges=[0])     # a name alone: C = 1
            assert tuple(one.count.shape) == (1, 17) and tuple(one.histogram.shape) == (1, 17, 2) and one.columns == ["cat"]
            _eq(_res(onec), [t.numpy() for t in _res(one)], ("one column", tag, exclude))
            nohist, nohistc = idx.facet_stats(q, ["cat", "big"], sp), loaded.facet_stats(q, ["cat", "big"], spc)
            assert tuple(nohist.histogram.shape) == (2, 17, 1) and torch.equal(nohist.histogram[:, :, 0], nohist.count)
            _eq(_res(nohistc), [t.numpy() for t in _res(nohist)], ("no edges", tag, exclude))
        sp.filter = spc.filter = None

    compare("as built")
    before = [t.clone() for t in _res(idx.facet_stats(q, ["cat", "big"], sp, radius=radius, edges=edges))]
    # save -> load, the attributes set again: the answer is unchanged
    path2 = str(tmp_path / "index2")
    idx.save(path2)
    for mod in (quake, qb):
        again = mod.QuakeIndex()
        again.load(path2)
        set_attributes(again)
        p = mod.SearchParams()
        p.nprobe, p.k = 5, 3
        for a, b in zip(_res(again.facet_stats(q, ["cat", "big"], p, radius=radius, edges=edges)), before):
            assert torch.equal(a, b)
    xa = torch.randn(300, d, generator=g)
    ia = torch.arange(300) + 10 ** 6
    for m in (idx, loaded):
        m.add(xa, ia)
        m.set_attribute("cat", ia[:150], torch.full((150,), 99))
    for i in ia[:150]:
        cat[int(i)] = 99
    compare("add")
    for m in (idx, loaded):
        m.remove(ids[:1500])
    compare("remove")
    for m, p in ((idx, sp), (loaded, spc)):
        empty = m.facet_stats(q[:0], ["cat", "big"], p, edges=edges)
        assert tuple(empty.count.shape) == (2, 0) and tuple(empty.histogram.shape) == (2, 0, 5) and tuple(empty.totals.shape) == (0,)


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

        plain = idx.facet_stats(qq, "doc", params(), radius=5.0, edges=[10, 20])
        assert plain.totals.sum() > 0
        for kw, match in ((dict(recall_target=0.9), "recall_target"),
                          (dict(filters=[idx.make_filter(ids[:1000])], query_filter=torch.zeros(10, dtype=torch.int32)), "query_filter"),
                          (dict(max_nprobe=8), "max_nprobe"),
                          (dict(filter_exact_rows=100, filter=idx.make_filter(ids[:50])), "filter_exact_rows"),
                          (dict(filters_exact_rows=100), "filters_exact_rows"),
                          (dict(filter=other.make_filter(ids[:1000])), "another index")):
            with pytest.raises(RuntimeError, match=match):
                idx.facet_stats(qq, "doc", params(**kw), radius=5.0)
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.facet_stats(qq, ["doc", "nope"], params(), radius=5.0)
        with pytest.raises(RuntimeError, match="NaN"):
            idx.facet_stats(qq, "doc", params(), radius=float("nan"))
        for names in ([], ["doc"] * 5):
            with pytest.raises(RuntimeError, match="between 1 and 4 columns"):
                idx.facet_stats(qq, names, params(), radius=5.0)
        for bad, match in (([3, 3], "strictly ascending"), ([5, 1], "strictly ascending"), (list(range(256)), "at most 255"),
                           ([1.5], "integers"), ([1 << 63], "int64"), ({"nope": [1]}, "not one of"), ({"doc": [2, 2]}, "strictly ascending")):
            with pytest.raises(RuntimeError, match=match):
                idx.facet_stats(qq, "doc", params(), radius=5.0, edges=bad)
        # a call with two faults raises the same error in both mirrors: the edges are looked at behind the refusals and the column
        # lookup, in front of the filter and the radius
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.facet_stats(qq, "doc", params(recall_target=0.9), radius=5.0, edges=[3, 3])
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.facet_stats(qq, ["doc", "nope"], params(), radius=5.0, edges=[1.5])
        with pytest.raises(RuntimeError, match="between 1 and 4 columns"):
            idx.facet_stats(qq, ["doc"] * 5, params(), radius=5.0, edges=[[1]])
        with pytest.raises(RuntimeError, match="strictly ascending"):
            idx.facet_stats(qq, "doc", params(), radius=float("nan"), edges=[3, 3])
        with pytest.raises(RuntimeError, match="strictly ascending"):
            idx.facet_stats(qq, "doc", params(filter=other.make_filter(ids[:1000])), radius=5.0, edges=[3, 3])
        # tensors in every position of edges
        for e in (torch.tensor([10, 20]), [torch.tensor([10, 20])], {"doc": torch.tensor([10, 20])}, [np.array([10, 20])]):
            for a, b in zip(_res(idx.facet_stats(qq, "doc", params(), radius=5.0, edges=e)), _res(plain)):
                assert torch.equal(a, b)
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.facet_stats(qq, "doc", params(), radius=5.0)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.facet_stats(qq, "doc", params(), radius=5.0, edges=[3, 3])
        again = idx.facet_stats(qq, "doc", params(), radius=5.0, edges=[10, 20])
        for a, b in zip(_res(again), _res(plain)):
            assert torch.equal(a, b)
