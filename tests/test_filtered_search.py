"""Filtered search (qk_filter_*, qk_search_filtered, qk_scan_filtered; Filter / SearchParams.filter in both mirrors): a search
restricted to a set of ids, decided inside the scan kernel (k_scan_filt / k_scan_wide_filt read a row mask derived from the ids).

Every comparison is bit for bit -- ids, and the uint32 view of the distances -- against the yardstick of tests/filter_yardstick.py:
the oracle's search over the CSR with the disallowed rows deleted (pinned on the CPU by tests/test_filtered_oracle.py).  On top of
that every answer is checked directly: it never contains a disallowed id."""
import zlib

import numpy as np
import pytest
import torch

import filter_yardstick as Y
import oracle as O

pytestmark = pytest.mark.gpu

QK_MAX_K = 448


def _corpus(d, nlist, n, metric, seed, empty=2, id_base=7, id_step=1):
    """clustered rows in skewed lists: `empty` empty lists, two lists of a handful of rows (shorter than a tile), the rest of
    whatever length the draw gives (almost never a multiple of 16)"""
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
    ids = rng.permutation(n).astype(np.int64) * id_step + id_base
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return dict(cent=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets, x=x, d=d,
                metric=metric)


def _queries(c, Q, seed):
    rng = np.random.default_rng(seed)
    q = (c["x"][rng.integers(0, c["x"].shape[0], size=Q)] + 0.05 * rng.standard_normal((Q, c["d"]))).astype(np.float32)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q)


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


def _eq(gi, gd, oi, od, tag):
    np.testing.assert_array_equal(_np(gi), oi, err_msg=str(tag))
    np.testing.assert_array_equal(_np(gd).view(np.uint32), np.asarray(od).view(np.uint32), err_msg=str(tag))


def _only_allowed(gi, all_ids, S, mode, tag):
    """directly: no id of the answer is outside the filter (independent of the yardstick)"""
    gi = _np(gi)
    got = gi[gi >= 0]
    assert np.isin(got, all_ids).all(), tag
    inS = np.isin(got, S)
    assert inS.all() if mode == "allow" else not inS.any(), tag


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
            c = _corpus(d, 64, 20000, metric, seed=100 + d + (1 if metric == "ip" else 0))
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and ((sizes > 0) & (sizes < 16)).sum() >= 1 and (sizes % 16 != 0).any()
            cache[(d, metric)] = (c,) + _stores(ctx, c)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[64, 128, 768], nprobe=[1, 8, 32], k=[1, 10, 100, 448], sel=[1, 0.5, 0.1, 0.01, 0],
            mode=["allow", "deny"], Q=[1, 17, 1024], mem=["host", "device"], entry=["search", "coarse+scan"])


def _grid():
    """The full grid has 2 x 3 x 3 x 4 x 5 x 2 x 3 x 2 x 2 = 8640 points.  Pruned with a fixed seed: case i takes, on every axis, the
    element i of a seeded shuffle of that axis repeated -- so every value of every axis appears (the longest axis has 5 values and
    there are 30 cases), in combinations the seed decides, not the author.  Q = 1024 with d = 768 is capped at nprobe 8 (the CPU
    yardstick of such a case takes tens of seconds); the cap moves the case to another point of the grid, it drops no axis value."""
    rng = np.random.default_rng(20240917)
    n = 30
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
    from quake_amd.capi import Filter
    c, s, parent = corpora(case["d"], case["metric"])
    metric, nprobe, k, Q = case["metric"], case["nprobe"], case["k"], case["Q"]
    rng = np.random.default_rng(zlib.crc32(repr(sorted(case.items())).encode()))
    q = _queries(c, Q, seed=int(rng.integers(1 << 30)))
    allow = Y.draw_set(c["ids"], case["sel"], rng)
    # deny: the complement of the allow-set (plus ids the store does not hold, which are ignored) -- the same filter
    S = allow if case["mode"] == "allow" else np.concatenate([np.setdiff1d(c["ids"], allow), np.array([-5, 10 ** 12], np.int64)])
    if case["mode"] == "allow":
        S = np.concatenate([S, S[:3], np.array([10 ** 12 + 1], np.int64)])  # duplicates and an absent id change nothing
    oi, od = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, S, case["mode"])
    dev = case["mem"] == "device"
    xq = torch.from_numpy(q).cuda() if dev else q
    f = Filter(s, torch.from_numpy(S).cuda() if dev else S, case["mode"])
    try:
        if case["entry"] == "search":
            gi, gd = ctx.search(parent, s, xq, nprobe, k, metric, filter=f)
        else:
            pids, _ = ctx.coarse(parent, xq, nprobe, metric)
            gi, gd = ctx.scan(s, xq, pids, k, metric, filter=f)
        ctx.synchronize()  # (device buffers are complete behind the context's stream)
        assert "(filtered)" in ctx.last_scan_kernel()
        _eq(gi, gd, oi, od, case)
        _only_allowed(gi, c["ids"], S, case["mode"], case)
        info = f.info()
        assert info["rebuilds"] == 0 and info["n_ids"] == np.unique(S).shape[0]
        assert info["rows_allowed"] == int(Y.allowed_rows(c["ids"], S, case["mode"]).sum())
    finally:
        f.close()


# ---- 2. padding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_padding(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent = corpora(64, metric)
    q = _queries(c, 33, seed=5)
    rng = np.random.default_rng(6)
    for S, tag in [(Y.draw_set(c["ids"], 0.002, rng), "fewer than k left"), (np.zeros(0, np.int64), "empty allow-set"),
                   (np.array([-3, 10 ** 13], np.int64), "nothing of the set is stored")]:
        f = Filter(s, S, "allow")
        for nprobe, k in [(1, 10), (4, 100)]:
            gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filter=f)
            oi, od = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, S, "allow")
            _eq(gi, gd, oi, od, (tag, nprobe, k))
            assert (gi < 0).any(), tag
            _only_allowed(gi, c["ids"], S, "allow", tag)
        if S.shape[0] == 0 or tag.startswith("nothing"):
            pad = np.float32(np.inf) if metric == "l2" else np.float32(-np.inf)
            assert (gi == -1).all() and (gd == pad).all()
        f.close()
    # a deny-set of everything: padding only as well
    f = Filter(s, c["ids"], "deny")
    gi, gd = ctx.search(parent, s, q, 8, 10, metric, filter=f)
    assert (gi == -1).all() and f.info()["rows_allowed"] == 0
    f.close()


# ---- 3. the seeding rule ---------------------------------------------------------------------------------------------------------
def test_disallowed_near_rows_do_not_seed_a_bound(ctx):
    """The nearest list's first 128 rows are disallowed and far closer to the queries than any allowed row, k <= 64, nprobe 8: the
    shape where the unfiltered path learns a bound from a sample of the nearest list's head.  A filtered search that kept that
    bound would return padding; the yardstick returns k rows."""
    from quake_amd.capi import Filter, Store
    d, nlist, per = 64, 16, 600
    rng = np.random.default_rng(31)
    cent = (4.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    vecs = (cent[:, None, :] + 1.0 * rng.standard_normal((nlist, per, d))).astype(np.float32)
    vecs[:, :128, :] = cent[:, None, :] + 0.001 * rng.standard_normal((nlist, 128, d)).astype(np.float32)  # every list: a tight head
    vecs = np.ascontiguousarray(vecs.reshape(-1, d))
    ids = np.arange(nlist * per, dtype=np.int64)
    offsets = np.arange(nlist + 1, dtype=np.int64) * per
    head = (ids % per) < 128
    q = (cent[rng.integers(0, nlist, size=256)] + 0.001 * rng.standard_normal((256, d))).astype(np.float32)
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
    f = Filter(s, ids[head], "deny")
    for k in (10, 64):
        gi, gd = ctx.search(parent, s, q, 8, k, "l2", filter=f)
        oi, od = Y.search(q, cent, vecs, ids, offsets, 8, k, "l2", ids[head], "deny")
        assert (oi >= 0).all()
        _eq(gi, gd, oi, od, k)
        _only_allowed(gi, ids, ids[head], "deny", k)
        ui, _ = ctx.search(parent, s, q, 8, k, "l2")
        assert np.isin(ui, ids[head]).all()  # the unfiltered answer is made of the disallowed heads only
    f.close()
    s.close()
    parent.close()


# ---- 4. everything allowed = the unfiltered search, from another kernel ----------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_all_allowed_equals_unfiltered(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent = corpora(128, metric)
    q = _queries(c, 300, seed=9)
    fa = Filter(s, c["ids"], "allow")
    fd = Filter(s, np.zeros(0, np.int64), "deny")
    for nprobe, k in [(1, 10), (8, 10), (32, 100)]:
        ui, ud = ctx.search(parent, s, q, nprobe, k, metric)
        unf = ctx.last_scan_kernel()
        for f in (fa, fd):
            gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filter=f)
            filt = ctx.last_scan_kernel()
            _eq(gi, gd, ui, ud, (nprobe, k))
            assert filt == "k_scan (filtered)" and filt != unf
    fa.close()
    fd.close()


# ---- 5. tile skipping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 768])
def test_tile_skipping(ctx, d):
    """long lists whose masks are mostly zero words: one allowed row in one tile, a row in the last (partial) tile only, whole tiles
    alternating, whole runs of 64+ zero words (the walk refills its 64-tile window)"""
    from quake_amd.capi import Filter, Store
    rng = np.random.default_rng(41)
    sizes = np.array([5003, 16 * 200, 7, 0, 2999], np.int64)
    nlist = sizes.shape[0]
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), sizes)
    vecs = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) + 1000
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    q = (vecs[rng.integers(0, n, size=40)] + 0.05 * rng.standard_normal((40, d))).astype(np.float32)
    pids = np.broadcast_to(np.arange(nlist, dtype=np.int64), (40, nlist)).copy()
    row = np.arange(n) - offsets[assign]  # row of its list
    sets = {
        "one row in one tile of the long list": ids[(assign == 0) & (row == 16 * 137 + 5)],
        "a row of the last, partial tile only": ids[(assign == 0) & (row == 5002)],
        "alternating whole tiles": ids[((row // 16) % 2 == 1)],
        "one tile in 70": ids[((row // 16) % 70 == 69)],
        "first and last tile of every list": ids[(row < 16) | (row >= (sizes[assign] - 1) // 16 * 16)],
    }
    for tag, S in sets.items():
        assert S.shape[0] > 0
        f = Filter(s, S, "allow")
        for k in (1, 10, 100):
            gi, gd = ctx.scan(s, q, pids, k, "l2", filter=f)
            oi, od = Y.scan(q, vecs, ids, offsets, pids, k, "l2", S, "allow")
            _eq(gi, gd, oi, od, (tag, k))
            _only_allowed(gi, ids, S, "allow", tag)
        assert f.info()["rows_allowed"] == S.shape[0]
        f.close()
    s.close()


# ---- 6. staleness: the filter follows the ids through everything that moves rows --------------------------------------------------
def _index_csr(idx):
    """the index's current partitions as a CSR in the order of the parent's rows (list i of the CSR = the partition of centroid
    i, so the oracle needs no list numbers: after maintenance they are no longer 0 .. nlist-1)"""
    s = idx._store
    cent, cids = idx.parent._store.get_list(0)
    assert sorted(int(p) for p in cids) == sorted(int(p) for p in s.list_ids())
    pv, pi = zip(*[s.get_list(int(p)) for p in cids])
    vecs, aids, offs = O.csr_from_partitions(pv, pi, idx._d)
    return cent, None, vecs, aids, offs


def test_filter_follows_ids_through_index_changes():
    import quake_amd as quake
    from quake_amd.maintenance import ListScanLatencyEstimator, MaintenanceCostEstimator
    g = torch.Generator().manual_seed(5)
    d, NB = 16, 60000
    x_bg = torch.randn(NB, d, generator=g)
    idx = quake.QuakeIndex()
    bp = quake.IndexBuildParams()
    bp.nlist = 40
    idx.build(x_bg, torch.arange(NB), bp)
    # as tests/test_maintenance_gpu.py: two hot partitions that will split, six tiny cold ones that will be deleted
    hot_c = torch.stack([torch.full((d,), 8.0), torch.full((d,), -8.0)])
    cold_c = torch.stack([torch.cat([torch.full((1,), 60.0 + 10 * i), torch.zeros(d - 1)]) for i in range(6)])
    vecs, vids, nxt = [], [], NB
    for c, n in [(hot_c[0], 1200), (hot_c[1], 1200)] + [(c, 10) for c in cold_c]:
        vecs.append((c + 0.3 * torch.randn(n, d, generator=g)).numpy())
        vids.append(np.arange(nxt, nxt + n, dtype=np.int64))
        nxt += n
    cents = np.stack([v.mean(0) for v in vecs]).astype(np.float32)
    idx._add_partitions({"centroids": cents, "vectors": vecs, "vector_ids": vids})
    idx._resident.update(range(NB, nxt))
    lat = ListScanLatencyEstimator(d, [1, 2, 4, 16, 64, 256, 1024, 4096, 16384, 65536], [1, 4, 16, 64, 256], 1,
                                   profile_fn=lambda n, k: 100.0 + 1.0 * n)
    mp = quake.MaintenancePolicyParams()
    mp.window_size = 200
    mp.refinement_radius = 4
    mp.refinement_iterations = 2
    mp.min_partition_size = 32
    mp.delete_threshold_ns = 0.1
    mp.split_threshold_ns = 0.1
    idx.initialize_maintenance_policy(mp, cost_estimator=MaintenanceCostEstimator(d, 0.9, 10, latency_estimator=lat))

    rng = np.random.default_rng(77)
    # S: a third of what is stored now, and ids that are not stored yet (some of them arrive later)
    S = np.concatenate([rng.permutation(nxt)[: nxt // 3], np.arange(nxt + 0, nxt + 200000, 2)]).astype(np.int64)
    q = torch.cat([hot_c[0] + 0.3 * torch.randn(150, d, generator=g), hot_c[1] + 0.3 * torch.randn(100, d, generator=g),
                   torch.randn(100, d, generator=g)])
    filters = {"allow": idx.make_filter(torch.from_numpy(S)), "deny": idx.make_filter(torch.from_numpy(S), exclude=True)}
    sp = quake.SearchParams()
    sp.k, sp.nprobe = 10, 4
    rebuilds = {m: 0 for m in filters}

    def check(tag, changed):
        cent, cids, cv, ci, co = _index_csr(idx)
        sp.filter = None
        r = idx.search(q, sp)  # the unfiltered search against the same partitions: the yardstick's inputs are the index's state
        oi, od = O.search(q.numpy(), cent, cv, ci, co, sp.nprobe, sp.k, "l2", batched_scan=True, num_threads=8, centroid_ids=cids)
        _eq(r.ids, r.distances, oi, od, (tag, "unfiltered"))
        for mode, f in filters.items():
            sp.filter = f
            for again in (False, True):  # two searches in a row: the second never rebuilds
                r = idx.search(q, sp)
                oi, od = Y.search(q.numpy(), cent, cv, ci, co, sp.nprobe, sp.k, "l2", S, mode, centroid_ids=cids)
                _eq(r.ids, r.distances, oi, od, (tag, mode, again))
                _only_allowed(r.ids, ci, S, mode, (tag, mode))
                info = f.info()
                want = rebuilds[mode] + (1 if changed and not again else 0)
                assert info["rebuilds"] == want, (tag, mode, again, info)
                rebuilds[mode] = want
                assert info["rows_allowed"] == int(Y.allowed_rows(ci, S, mode).sum())
        sp.filter = None

    check("as built", changed=False)
    # add: ids inside and outside S
    na = 3000
    idx.add(torch.randn(na, d, generator=g), torch.arange(nxt, nxt + na))
    nxt += na
    check("add", changed=True)
    # remove (swap with last inside the lists): allowed and disallowed ids
    idx.remove(torch.from_numpy(np.concatenate([S[:2000], np.setdiff1d(np.arange(NB), S)[:2000]])))
    check("remove", changed=True)
    # modify: the rows of some ids are replaced (and move to other lists)
    mid = torch.from_numpy(np.intersect1d(S, idx.get_ids().numpy())[:500])
    idx.modify(mid, torch.randn(mid.shape[0], d, generator=g))
    check("modify", changed=True)
    idx.refine_partitions(torch.tensor([0, 1, 2, 3, 4, 5]), 2)
    check("refine_partitions", changed=True)
    # maintenance with a recorded latency grid: splits the two hot partitions, deletes the six cold ones
    idx.track_hits = True
    sp1 = quake.SearchParams()
    sp1.k, sp1.nprobe = 10, 1
    idx.search(q[:250], sp1)
    idx.track_hits = False
    t = idx.maintenance()
    assert t.n_splits >= 1 and t.n_deletes >= 1, (t.n_splits, t.n_deletes)
    check("maintenance", changed=True)
    # an add that outgrows the arena
    grown = idx._store.counters()["arena_reallocations"]
    nb = 90000
    idx.add(torch.randn(nb, d, generator=g), torch.arange(nxt, nxt + nb))
    nxt += nb
    assert idx._store.counters()["arena_reallocations"] > grown
    check("arena growth", changed=True)
    check("nothing changed", changed=False)


# ---- 7. wide rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    from quake_amd.capi import Filter
    d = 3072
    c = _corpus(d, 24, 3000, metric, seed=51)
    s, parent = _stores(ctx, c)
    q = _queries(c, 19, seed=52)
    rng = np.random.default_rng(53)
    S = Y.draw_set(c["ids"], 0.1, rng)
    # ... and the rows of one list as a contiguous range: whole tiles without a candidate elsewhere
    o = c["offsets"]
    big = int(np.argmax(np.diff(o)))
    S2 = c["ids"][o[big] + 40: o[big] + 90]
    for S_, mode in [(S, "allow"), (S2, "allow"), (S, "deny")]:
        f = Filter(s, S_, mode)
        for k, nprobe in [(10, 3), (448, 24)]:
            gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filter=f)
            assert ctx.last_scan_kernel() == "k_scan_wide (filtered)"
            oi, od = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, S_, mode)
            _eq(gi, gd, oi, od, (mode, k, nprobe))
            _only_allowed(gi, c["ids"], S_, mode, (mode, k))
        f.close()
    s.close()
    parent.close()


# ---- 8. both mirrors, flat index, hit tracking --------------------------------------------------------------------------------------
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
def test_both_mirrors(qb, nlist):
    import quake_amd as quake
    g = torch.Generator().manual_seed(61)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(50, d, generator=g)
    rng = np.random.default_rng(62)
    S = torch.from_numpy(Y.draw_set(ids.numpy(), 0.2, rng))
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, nlist)
        sp = mod.SearchParams()
        assert sp.filter is None
        before = repr(sp)
        sp.k, sp.nprobe = 10, 5
        plain = idx.search(q, sp)
        for exclude in (False, True):
            sp.filter = idx.make_filter(S, exclude)
            r = idx.search(q, sp)
            rd = idx.search(q.cuda(), sp)  # device tensors
            assert torch.equal(rd.ids.cpu(), r.ids) and torch.equal(rd.distances.cpu(), r.distances)
            out[(name, exclude)] = (r.ids.numpy(), r.distances.numpy())
            _only_allowed(r.ids, ids.numpy(), S.numpy(), "deny" if exclude else "allow", (name, exclude))
            assert sp.filter.info()["rows_allowed"] == (n - S.shape[0] if exclude else S.shape[0])
        sp.filter = None
        assert "filter" not in before and repr(mod.SearchParams()) == before  # the summary does not know the extension
        again = idx.search(q, sp)
        assert torch.equal(again.ids, plain.ids)
        if name == "python":
            # yardstick over the index's own partitions
            if nlist == 0:
                pv, pi = idx._store.get_list(0)
                offs = np.array([0, n], np.int64)
                for exclude in (False, True):
                    oi, od = Y.search(q.numpy(), None, pv, pi, offs, 1, 10, "l2", S.numpy(), "deny" if exclude else "allow")
                    _eq(*out[(name, exclude)], oi, od, ("flat", exclude))
            else:
                cent, cids, cv, ci, co = _index_csr(idx)
                for exclude in (False, True):
                    oi, od = Y.search(q.numpy(), cent, cv, ci, co, 5, 10, "l2", S.numpy(), "deny" if exclude else "allow", centroid_ids=cids)
                    _eq(*out[(name, exclude)], oi, od, ("ivf", exclude))
                # hit tracking: the probed lists are the unfiltered search's
                idx.track_hits = True
                sp.filter = idx.make_filter(S)
                idx.search(q, sp)
                hits_f = idx._pending_hits[-1].clone()
                sp.filter = None
                idx.search(q, sp)
                hits_u = idx._pending_hits[-1]
                assert torch.equal(hits_f.cpu(), hits_u.cpu())
    for exclude in (False, True):  # (both mirrors ran the same k-means: the same partitions, the same tensors)
        np.testing.assert_array_equal(out[("python", exclude)][0], out[("compiled", exclude)][0])
        np.testing.assert_array_equal(out[("python", exclude)][1].view(np.uint32), out[("compiled", exclude)][1].view(np.uint32))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, corpora, qb):
    import quake_amd as quake
    from quake_amd.capi import Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(64, "l2")
    c2, s2, parent2 = corpora(128, "l2")
    q = _queries(c, 8, seed=3)
    f = Filter(s, c["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.search(parent, s, q, 4, QK_MAX_K + 1, "l2", filter=f)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.scan(s, q, np.zeros((8, 1), np.int64), QK_MAX_K + 1, "l2", filter=f)
    f2 = Filter(s2, c2["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search(parent, s, q, 4, 10, "l2", filter=f2)
    with pytest.raises(ValueError):
        Filter(s, c["ids"][:5], "maybe")
    gi, gd = ctx.search(parent, s, q, 4, 10, "l2")  # the context still answers
    oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", batched_scan=True)
    _eq(gi, gd, oi, od, "after refusals")
    f.close()
    f2.close()

    g = torch.Generator().manual_seed(71)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        plain = idx.search(qq, sp)
        sp.filter = idx.make_filter(ids[:1000])
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.search(qq, sp)
        sp.recall_target = -1.0
        sp.k = QK_MAX_K + 1
        with pytest.raises(RuntimeError, match="QK_MAX_K"):
            idx.search(qq, sp)
        sp.k = 5
        sp.filter = other.make_filter(ids[:1000])
        with pytest.raises((RuntimeError, ValueError), match="another"):
            idx.search(qq, sp)
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.make_filter(ids[:1000])
        sp.filter = idx.make_filter(ids[:1000])
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.search(qq, sp)
        sp.filter = None
        again = idx.search(qq, sp)
        assert torch.equal(again.ids, plain.ids) and torch.equal(again.distances, plain.distances)
        assert tuple(grp.search(qq, sp).ids.shape) == (10, 5)


# ---- 10. 64-bit ids ----------------------------------------------------------------------------------------------------------------
def test_64_bit_ids(ctx):
    from quake_amd.capi import Filter
    c = _corpus(128, 32, 12000, "l2", seed=81, id_base=1 << 33, id_step=16)  # 2^33 + 16 x permutation
    assert c["ids"].min() >= (1 << 33)
    s, parent = _stores(ctx, c)
    q = _queries(c, 100, seed=82)
    rng = np.random.default_rng(83)
    S = Y.draw_set(c["ids"], 0.1, rng)
    near = S + 1  # ids that differ from allowed ones in the low bits only, and are not stored
    for S_, mode in [(S, "allow"), (S, "deny"), (near, "allow"), (S - (1 << 33), "allow")]:
        f = Filter(s, S_, mode)
        gi, gd = ctx.search(parent, s, q, 8, 10, "l2", filter=f)
        oi, od = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 8, 10, "l2", S_, mode)
        _eq(gi, gd, oi, od, mode)
        _only_allowed(gi, c["ids"], S_, mode, mode)
        f.close()
    s.close()
    parent.close()


def test_filter_outlives_its_store(ctx):
    from quake_amd.capi import Filter
    c = _corpus(64, 8, 2000, "l2", seed=91)
    s, parent = _stores(ctx, c)
    f = Filter(s, c["ids"][:50], "allow")
    assert f.info()["device_bytes"] > 0 and s.device_bytes() > 0
    f.store = None
    s.close()
    assert f.info()["n_ids"] == 50
    f.close()
    parent.close()
