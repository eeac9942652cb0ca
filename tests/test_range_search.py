"""Range search (qk_range_search / qk_range_scan; Context.range_search / range_scan; QuakeIndex.range_search in both mirrors):
every row of the probed lists within a radius of each query, in scan order, behind a capacity protocol that never loses the counts.

Every comparison is bit for bit -- lims, ids, and the uint32 view of the distances -- against tests/range_yardstick.py: the
oracle's canonical distance of every probed row, walked in scan order and cut at the radius in float32 (pinned on the CPU by
tests/test_range_oracle.py).  Radii are taken from the yardstick's own distances, so every case has rows exactly on the radius."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu


def _stores(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _eq(got, want, tag):
    np.testing.assert_array_equal(_np(got[0]), want[0], err_msg="lims " + str(tag))
    np.testing.assert_array_equal(_np(got[1]), want[1], err_msg="ids " + str(tag))
    np.testing.assert_array_equal(_np(got[2]).view(np.uint32), np.asarray(want[2]).view(np.uint32), err_msg="dist " + str(tag))


def _radius(pairs, Q, level, metric):
    """a radius from the yardstick's own distances: 'few' -- about Q / 4 hits in all, no hit for most queries; 'ten' -- about 10
    per query; 'inf' -- every probed row"""
    if level == "inf":
        return np.float32(np.inf if metric == "l2" else -np.inf)
    d = np.sort(pairs[2])
    if metric == "ip":
        d = d[::-1]
    want = max(1, Q // 4) if level == "few" else 10 * Q
    return d[min(want, d.shape[0]) - 1]


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c = RY.corpus(d, 64, 20000, metric, seed=300 + d + (1 if metric == "ip" else 0))
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and ((sizes > 0) & (sizes < 16)).sum() >= 1 and (sizes % 16 != 0).any()
            cache[(d, metric)] = (c,) + _stores(ctx, c)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


@pytest.fixture(scope="module")
def small(ctx, corpora):
    """one shared case for the protocol tests: d = 64, L2, 33 queries, nprobe 4, its probed lists and the yardstick's pairs"""
    c, s, parent = corpora(64, "l2")
    q = RY.queries(c, 33, seed=11)
    pids = RY.probed(q, c["cent"], c["offsets"], 4, "l2")
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, "l2")
    return dict(c=c, s=s, parent=parent, q=q, pids=pids, pairs=pairs)


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[64, 128, 768], nprobe=[1, 8, 32], Q=[1, 17, 1024], level=["few", "ten", "inf"],
            mem=["host", "device"], entry=["range_search", "coarse+range_scan"])


def _grid():
    """2 x 3 x 3 x 3 x 3 x 2 x 2 = 648 points, pruned with a fixed seed: case i takes, on every axis, element i of a seeded shuffle of
    that axis repeated -- every value of every axis appears, in combinations the seed decides.  Q = 1024 with d = 768 is capped at
    nprobe 8 (the CPU yardstick of such a case takes tens of seconds); the cap moves the case, it drops no axis value."""
    rng = np.random.default_rng(20250310)
    n = 24
    cols = {}
    for name, vals in AXES.items():
        seq = []
        while len(seq) < n:
            seq += [vals[i] for i in rng.permutation(len(vals))]
        cols[name] = seq[:n]
    cases = []
    for i in range(n):
        c = {name: cols[name][i] for name in AXES}
        if c["Q"] == 1024 and c["d"] == 768 and c["nprobe"] == 32:
            c["nprobe"] = 8
        cases.append(c)
    for name, vals in AXES.items():
        assert {c[name] for c in cases} == set(vals), name
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, case):
    c, s, parent = corpora(case["d"], case["metric"])
    metric, nprobe, Q = case["metric"], case["nprobe"], case["Q"]
    q = RY.queries(c, Q, seed=zlib.crc32(repr(sorted(case.items())).encode()) % (1 << 30))
    pids = RY.probed(q, c["cent"], c["offsets"], nprobe, metric)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    radius = _radius(pairs, Q, case["level"], metric)
    want = RY.select(pairs, c["ids"], radius, metric)
    if case["level"] == "few" and Q > 1:
        assert (np.diff(want[0]) == 0).sum() > Q // 2
    if case["level"] == "inf":
        assert want[1].shape[0] == pairs[1].shape[0]
    dev = case["mem"] == "device"
    xq = torch.from_numpy(q).cuda() if dev else q
    if case["entry"] == "range_search":
        got = ctx.range_search(parent, s, xq, nprobe, radius, metric)
    else:
        gp, _ = ctx.coarse(parent, xq, nprobe, metric)
        got = ctx.range_scan(s, xq, gp, radius, metric)
    ctx.synchronize()
    assert ctx.last_scan_kernel() == "k_scan (range)"
    assert ctx.last_range_calls <= 2
    _eq(got, want, case)


# ---- 2. wide rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    c = RY.corpus(3072, 8, 3000, metric, seed=351)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 17, seed=352)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], RY.probed(q, c["cent"], c["offsets"], 3, metric), metric)
    for level in ("few", "ten", "inf"):
        radius = _radius(pairs, 17, level, metric)
        got = ctx.range_search(parent, s, q, 3, radius, metric)
        assert ctx.last_scan_kernel() == "k_scan_wide (range)"
        _eq(got, RY.select(pairs, c["ids"], radius, metric), (metric, level))
    s.close()
    parent.close()


# ---- 3. the boundary: inclusive, exact, on the value the caller sees ---------------------------------------------------------------
def _better(r, metric):
    return np.nextafter(np.float32(r), np.float32(-np.inf if metric == "l2" else np.inf))


@pytest.mark.parametrize("mode", ["l2", "l2-squared", "ip"])
def test_boundary(ctx, corpora, mode):
    metric = "ip" if mode == "ip" else "l2"
    c, s, parent = corpora(128, metric)
    q = RY.queries(c, 6, seed=21)
    q[0] = c["vecs"][c["offsets"][10] + 3]  # a stored row: distance 0 under L2
    pids = RY.probed(q, c["cent"], c["offsets"], 4, metric)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    inf = np.float32(np.inf if metric == "l2" else -np.inf)
    ctx.set_squared_l2(mode == "l2-squared")
    try:
        lims, ids, dist = ctx.range_search(parent, s, q, 4, inf, metric)  # every probed row with the distance the caller sees
        np.testing.assert_array_equal(lims, pairs[0])
        np.testing.assert_array_equal(ids, c["ids"][pairs[1]])
        seen = np.sqrt(dist) if mode == "l2-squared" else dist  # (float32 sqrt is correctly rounded: the same bits as the library's)
        np.testing.assert_array_equal(seen.view(np.uint32), pairs[2].view(np.uint32))
        rng = np.random.default_rng(22)
        for qi in range(q.shape[0]):
            mine = slice(lims[qi], lims[qi + 1])
            dq, iq = dist[mine], ids[mine]
            for j in rng.integers(0, dq.shape[0], size=3):
                for r, inside in [(dq[j], True), (_better(dq[j], metric), False)]:
                    gl, gi, gd = ctx.range_search(parent, s, q[qi:qi + 1], 4, r, metric)
                    keep = RY.passes(dq, r, metric)
                    np.testing.assert_array_equal(gi, iq[keep])
                    np.testing.assert_array_equal(gd.view(np.uint32), dq[keep].view(np.uint32))
                    assert gl[1] == keep.sum() and (iq[j] in gi) == inside, (mode, qi, j, r)
        if metric == "l2":  # a row at distance 0 with radius 0 is a hit
            zero = c["ids"][c["offsets"][10] + 3]
            assert dist[:lims[1]][ids[:lims[1]] == zero] == np.float32(0)
            for r in (0.0, -0.0):
                gl, gi, gd = ctx.range_search(parent, s, q[:1], 4, r, metric)
                assert zero in gi and (gd == 0).all() and gl[1] == (dist[:lims[1]] == 0).sum()
            gl, gi, gd = ctx.range_search(parent, s, q[:1], 4, -1e-30, metric)
            assert gl[1] == 0 and gi.shape[0] == 0
    finally:
        ctx.set_squared_l2(False)


# ---- 4. the capacity protocol ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_capacity(ctx, small, mem):
    c, s, parent, q = small["c"], small["s"], small["parent"], small["q"]
    radius = _radius(small["pairs"], q.shape[0], "ten", "l2")
    want = RY.select(small["pairs"], c["ids"], radius, "l2")
    total = int(want[0][-1])
    assert total >= 100
    dev = mem == "device"
    xq = torch.from_numpy(q).cuda() if dev else q
    SI, SD = -777, np.float32(-5.5)

    def buffers(n):
        if dev:
            return torch.full((n,), SI, dtype=torch.int64, device="cuda"), torch.full((n,), float(SD), dtype=torch.float32, device="cuda")
        return np.full(n, SI, np.int64), np.full(n, SD, np.float32)

    for cap in (total // 2, total + 100, 1):
        bi, bd = buffers(total + 200)
        lims, gi, gd = ctx.range_search(parent, s, xq, 4, radius, "l2", cap=cap, out=(bi, bd))
        ctx.synchronize()
        n = min(cap, total)
        np.testing.assert_array_equal(_np(lims), want[0])  # exact whatever cap is
        assert gi.shape[0] == n
        np.testing.assert_array_equal(_np(bi)[:n], want[1][:n])
        np.testing.assert_array_equal(_np(bd)[:n].view(np.uint32), want[2][:n].view(np.uint32))
        assert (_np(bi)[n:] == SI).all() and (_np(bd)[n:] == SD).all()  # nothing behind the prefix is touched
    # count only: no buffers at all
    lims, gi, gd = ctx.range_search(parent, s, xq, 4, radius, "l2", cap=0)
    ctx.synchronize()
    np.testing.assert_array_equal(_np(lims), want[0])
    assert gi.shape[0] == 0 and gd.shape[0] == 0 and ctx.last_range_calls == 1
    # ids without distances
    bi, _ = buffers(total)
    lims, gi, gd = ctx.range_search(parent, s, xq, 4, radius, "l2", out=(bi, None))
    ctx.synchronize()
    np.testing.assert_array_equal(_np(bi), want[1])
    # cap=None: a short first guess is repeated once, and only once
    inf = ctx.range_search(parent, s, xq, 4, np.inf, "l2")
    assert ctx.last_range_calls == 2 and small["pairs"][1].shape[0] > max(4096, 64 * q.shape[0])
    _eq(inf, RY.select(small["pairs"], c["ids"], np.inf, "l2"), "cap=None, two calls")
    _eq(ctx.range_search(parent, s, xq, 4, radius, "l2"), want, "cap=None, one call")
    assert ctx.last_range_calls == 1
    # Q == 0
    lims, gi, gd = ctx.range_search(parent, s, xq[:0], 4, radius, "l2")
    assert _np(lims).tolist() == [0] and gi.shape[0] == 0


# ---- 5. passes: lims and results are continuous across every pass boundary ---------------------------------------------------------
def test_passes(ctx):
    """The pass size depends on the store's LARGEST list: one unprobed list of 300 000 rows makes a call with P = 32 run in
    ceil(1024 / floor(2^29 / (32 * 300000))) = 19 passes while the probed work and the yardstick stay tiny."""
    from quake_amd.capi import Store
    d, nsmall, big = 16, 48, 300000
    rng = np.random.default_rng(41)
    sizes = rng.integers(0, 60, size=nsmall)
    sizes[[3, 17]] = 0
    sizes = np.concatenate([sizes, [big]]).astype(np.int64)
    offsets = np.zeros(nsmall + 2, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    Q, P = 1024, 32
    q = rng.standard_normal((Q, d)).astype(np.float32)
    pids = np.stack([rng.permutation(nsmall)[:P] for _ in range(Q)]).astype(np.int64)
    pids[rng.random((Q, P)) < 0.05] = -1
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    pairs = RY.all_pairs(q, vecs, ids, offsets, pids, "l2")
    ctx.set_timing(1)
    try:
        for level in ("ten", "inf"):
            radius = _radius(pairs, Q, level, "l2")
            want = RY.select(pairs, ids, radius, "l2")
            lims, gi, gd, tm = ctx.range_scan(s, q, pids, radius, "l2", timing=True)
            assert tm["n_items"] == -(-Q // ((1 << 29) // (P * big))) == 19
            _eq((lims, gi, gd), want, level)
            assert tm["partitions_scanned"] == int(((pids >= 0) & (sizes[np.maximum(pids, 0)] > 0)).sum())
            assert tm["scan_bytes"] == int(sizes[np.unique(pids[pids >= 0])].sum()) * d * 4
        # a capacity that ends inside a later pass
        cap = int(want[0][700]) + 3
        bi, bd = np.full(want[1].shape[0], -9, np.int64), np.full(want[1].shape[0], -9, np.float32)
        lims, gi, gd = ctx.range_scan(s, q, pids, radius, "l2", cap=cap, out=(bi, bd))
        np.testing.assert_array_equal(lims, want[0])
        np.testing.assert_array_equal(bi[:cap], want[1][:cap])
        assert (bi[cap:] == -9).all() and (bd[cap:] == -9).all()
    finally:
        ctx.set_timing(0)
        s.close()


# ---- 6. pids edge cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_pids_edge_cases(ctx, small, mem):
    from quake_amd.capi import Store
    c, s = small["c"], small["s"]
    q = small["q"][:5]
    sizes = np.diff(c["offsets"])
    empty = int(np.nonzero(sizes == 0)[0][0])
    pids = np.array([[5, -1, 9], [-1, -1, -1], [10 ** 6, 7, empty], [-1, 6, -1], [64, 65, 10 ** 12]], np.int64)  # 64+: never created
    want = RY.scan(q, c["vecs"], c["ids"], c["offsets"], np.where(pids >= 64, -1, pids), np.inf, "l2")
    np.testing.assert_array_equal(np.diff(want[0]), [sizes[5] + sizes[9], 0, sizes[7], sizes[6], 0])
    dev = mem == "device"
    got = ctx.range_scan(s, torch.from_numpy(q).cuda() if dev else q, torch.from_numpy(pids).cuda() if dev else pids, np.inf, "l2")
    ctx.synchronize()
    _eq(got, want, "edge pids")
    # a list that was removed is absent too
    s2 = Store(ctx, c["d"])
    s2.build_csr(c["offsets"], c["ids"], c["vecs"])
    s2.remove_list(7)
    got = ctx.range_scan(s2, q, pids, np.inf, "l2")
    np.testing.assert_array_equal(np.diff(got[0]), [sizes[5] + sizes[9], 0, 0, sizes[6], 0])
    # parent == None: every list, in list order
    got = ctx.range_search(None, s, q[:2], 1, np.inf, "l2")
    _eq(got, RY.search(q[:2], None, c["vecs"], c["ids"], c["offsets"], 1, np.inf, "l2"), "all lists")
    s2.close()


# ---- 7. filter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filter(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent = corpora(64, metric)
    q = RY.queries(c, 40, seed=61)
    rng = np.random.default_rng(62)
    pids = RY.probed(q, c["cent"], c["offsets"], 8, metric)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    for sel in (0.5, 0.01, 0):
        allow = FY.draw_set(c["ids"], sel, rng)
        for mode in ("allow", "deny"):
            S = allow if mode == "allow" else np.setdiff1d(c["ids"], allow)
            f = Filter(s, S, mode)
            for level in ("ten", "inf"):
                radius = _radius(pairs, 40, level, metric)
                want = RY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 8, radius, metric, S, mode)
                got = ctx.range_search(parent, s, q, 8, radius, metric, filter=f)
                _eq(got, want, (sel, mode, level))
                assert np.isin(got[1], allow).all()  # directly: nothing outside the filter
                _eq(ctx.range_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(pids).cuda(), radius, metric, filter=f), want,
                    (sel, mode, level, "scan, device"))
                if sel == 0:
                    assert got[1].shape[0] == 0 and (_np(got[0]) == 0).all()
            assert f.info()["rebuilds"] == 0
            f.close()


def test_filter_follows_store_changes(ctx):
    from quake_amd.capi import Filter, Store
    c = RY.corpus(32, 24, 6000, "l2", seed=71)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(72)
    q = RY.queries(c, 50, seed=73)
    pids = RY.probed(q, c["cent"], c["offsets"], 6, "l2")
    S = np.concatenate([FY.draw_set(c["ids"], 0.3, rng), np.arange(10 ** 6, 10 ** 6 + 2000, 2)]).astype(np.int64)
    filters = {"allow": Filter(s, S, "allow"), "deny": Filter(s, S, "deny")}

    def check(tag, rebuilds):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(24)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        pairs = RY.all_pairs(q, vecs, ids, offs, pids, "l2")
        radius = _radius(pairs, 50, "ten", "l2")
        _eq(ctx.range_scan(s, q, pids, radius, "l2"), RY.select(pairs, ids, radius, "l2"), (tag, "unfiltered"))
        for mode, f in filters.items():
            got = ctx.range_scan(s, q, pids, radius, "l2", filter=f)
            _eq(got, RY.scan(q, vecs, ids, offs, pids, radius, "l2", S, mode), (tag, mode))
            assert np.isin(got[1], S).all() if mode == "allow" else not np.isin(got[1], S).any()
            assert f.info()["rebuilds"] == rebuilds, (tag, mode)

    check("as built", 0)
    na = 800
    s.add_batch(np.arange(10 ** 6, 10 ** 6 + na, dtype=np.int64), (c["cent"][rng.integers(4, 24, size=na)]
                + 0.4 * rng.standard_normal((na, 32))).astype(np.float32), rng.integers(4, 24, size=na).astype(np.int64))
    check("add_batch", 1)
    s.remove_ids(np.concatenate([S[:500], np.setdiff1d(c["ids"], S)[:500]]))
    check("remove_ids", 2)
    nos = np.array([5, 6, 7, 8], np.int64)
    s.refine_lists(nos, np.ascontiguousarray(c["cent"][nos]), "l2", 2)
    check("refine_lists", 3)
    check("nothing changed", 3)
    for f in filters.values():
        f.close()
    s.close()
    parent.close()


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------------
def test_determinism(small):
    from quake_amd.capi import Context
    c, s, parent, q = small["c"], small["s"], small["parent"], small["q"]
    radius = _radius(small["pairs"], q.shape[0], "ten", "l2")
    ctxs = [Context(0), Context(0)]
    runs = [ctxs[i].range_search(parent, s, q, 4, radius, "l2") for i in (0, 0, 1)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()
    _eq(runs[2], RY.select(small["pairs"], c["ids"], radius, "l2"), "second context")
    for x in ctxs:
        x.close()


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, corpora, small):
    from quake_amd._lib import QK_MEM_HOST, QuakeHipError
    from quake_amd.capi import Filter
    c, s, parent, q = small["c"], small["s"], small["parent"], small["q"]
    c2, s2, parent2 = corpora(128, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*NaN"):
        ctx.range_search(parent, s, q, 4, float("nan"), "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*NaN"):
        ctx.range_scan(s, q, small["pids"], float("nan"), "ip")
    lims = np.zeros(q.shape[0] + 1, np.int64)
    ids, dist = np.zeros(8, np.int64), np.zeros(8, np.float32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def raw(cap, lims_p):
        return ctx.lib.qk_range_search(ctx.h, parent.h, s.h, P(q), q.shape[0], 4, 1, 1.0, None, cap, lims_p, P(ids), P(dist), QK_MEM_HOST, None)

    assert raw(-1, P(lims)) == 1 and raw(8, None) == 1 and raw(8, P(lims)) == 0  # QK_ERR_INVALID twice, then QK_OK
    pp = np.ascontiguousarray(small["pids"])
    assert ctx.lib.qk_range_scan(ctx.h, s.h, P(q), q.shape[0], P(pp), 4, 1, 1.0, None, -5, P(lims), P(ids), P(dist), QK_MEM_HOST, None) == 1
    assert ctx.lib.qk_range_scan(ctx.h, s.h, P(q), q.shape[0], P(pp), 4, 1, 1.0, None, 8, None, P(ids), P(dist), QK_MEM_HOST, None) == 1
    f2 = Filter(s2, c2["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.range_search(parent, s, q, 4, 1.0, "l2", filter=f2)
    f2.close()
    gi, gd = ctx.search(parent, s, q, 4, 10, "l2")  # the context still answers
    oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", batched_scan=True)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))


# ---- 10. both mirrors ------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("nlist", [0, 20])
def test_mirrors(qb, nlist, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(81)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(50, d, generator=g)
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.2, np.random.default_rng(82)))
    idx = _build(quake, x, ids, nlist)
    sp = quake.SearchParams()
    before = repr(sp)
    sp.k, sp.nprobe = 10, 5
    radius = float(idx.search(q, sp).distances[:, -1].median())  # about 10 hits per query
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    spc = qb.SearchParams()
    spc.k, spc.nprobe = 10, 5
    for exclude in (None, False, True):
        sp.filter = None if exclude is None else idx.make_filter(S, exclude)
        spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
        r = idx.range_search(q, radius, sp)
        # the Python mirror is Context.range_search on the index's own stores
        lims, gi, gd = idx._ctx.range_search(idx.parent._store if idx.parent is not None else None, idx._store, q.numpy(), 5, radius, "l2",
                                             filter=sp.filter._h if sp.filter is not None else None)
        _eq((r.lims, r.ids, r.distances), (lims, gi, gd), ("python", exclude))
        assert r.lims[-1] == r.ids.shape[0] == r.distances.shape[0] and r.ids.shape[0] > 0 and r.timing_info.n_queries == 50
        if exclude is not None:
            assert np.isin(r.ids.numpy(), S.numpy()).all() != exclude and (exclude or r.ids.shape[0] > 0)
        rd = idx.range_search(q.cuda(), radius, sp)  # device tensors in, device tensors out
        assert rd.ids.is_cuda and rd.lims.is_cuda and rd.distances.is_cuda
        _eq((rd.lims, rd.ids, rd.distances), (lims, gi, gd), ("python, device", exclude))
        # the compiled mirror over the same saved partitions
        for xq in (q, q.cuda()):
            rc = loaded.range_search(xq, radius, spc)
            assert rc.ids.is_cuda == xq.is_cuda
            _eq((rc.lims, rc.ids, rc.distances), (lims, gi, gd), ("compiled", exclude, xq.is_cuda))
        # the infinite radius goes through the second call of the capacity protocol
        big = idx.range_search(q, float("inf"), sp)
        bigc = loaded.range_search(q, float("inf"), spc)
        _eq((bigc.lims, bigc.ids, bigc.distances), (big.lims.numpy(), big.ids.numpy(), big.distances.numpy()), ("inf", exclude))
        if exclude is None:
            assert big.ids.shape[0] > max(4096, 64 * 50) and (nlist != 0 or big.ids.shape[0] == 50 * n)
    sp.filter = None
    assert "filter" not in before and repr(quake.SearchParams()) == before
    empty = idx.range_search(q[:0], radius, sp)
    assert empty.lims.tolist() == [0] and empty.ids.shape[0] == 0


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(91)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        plain = idx.range_search(qq, 3.0, sp)
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.range_search(qq, 3.0, sp)
        sp.recall_target = -1.0
        sp.filters = [idx.make_filter(ids[:1000])]
        sp.query_filter = torch.zeros(10, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="query_filter"):
            idx.range_search(qq, 3.0, sp)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        sp.filter = other.make_filter(ids[:1000])
        with pytest.raises(RuntimeError, match="another index"):
            idx.range_search(qq, 3.0, sp)
        sp.filter = None
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.range_search(qq, 3.0, sp)
        with pytest.raises((RuntimeError, ValueError), match="NaN"):
            idx.range_search(qq, float("nan"), sp)
        again = idx.range_search(qq, 3.0, sp)
        assert torch.equal(again.lims, plain.lims) and torch.equal(again.ids, plain.ids) and torch.equal(again.distances, plain.distances)
