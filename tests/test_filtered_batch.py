"""Per-query filters (qk_search_filtered_batch, qk_search_filtered_batch_tracked, qk_scan_filtered_batch; filters= / query_filter=
of capi.Context; SearchParams.filters / query_filter in both mirrors): one batch, a different id filter for each query, decided
inside the scan kernel (k_scan_filtq / k_scan_wide_filtq test a row against the mask word of its lane's own query).

The definition is the equation the tests use: row i of the answer equals the single-filter answer of query i alone under
filters[qfilter[i]].  Expected values come from tests/filter_yardstick.py, per distinct filter over the queries that name it, the
rows scattered back into place; every comparison is bit for bit (ids, uint32 view of the distances), and every answer is checked
directly: no id of a row lies outside that row's own filter.  No test reads a clock."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_yardstick as Y
import oracle as O
from test_filtered_search import _build, _corpus, _eq, _index_csr, _np, _queries, _stores

pytestmark = pytest.mark.gpu

QK_MAX_K = 448
PER_QUERY = "k_scan (filtered, per query)"
PER_QUERY_WIDE = "k_scan_wide (filtered, per query)"


def _pad(metric):
    return np.float32(np.inf) if metric == "l2" else np.float32(-np.inf)


def _scatter(Q, k, metric, qf, sets, fn):
    """the per-query yardstick: fn(rows, S, mode) -> (ids, dist) of the queries `rows` under one filter, for every distinct filter
    number of qf; a number outside [0, F) leaves its rows padded"""
    oi = np.full((Q, k), -1, np.int64)
    od = np.full((Q, k), _pad(metric), np.float32)
    for f in np.unique(qf):
        if not 0 <= f < len(sets):
            continue
        rows = np.nonzero(qf == f)[0]
        oi[rows], od[rows] = fn(rows, *sets[f])
    return oi, od


def _yard_search(q, c, nprobe, k, metric, qf, sets):
    return _scatter(q.shape[0], k, metric, qf, sets, lambda rows, S, mode: Y.search(
        np.ascontiguousarray(q[rows]), c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, S, mode))


def _own_filter_only(gi, all_ids, qf, sets, tag):
    """directly: no id of row i is outside filters[qf[i]] (independent of the yardstick)"""
    gi = _np(gi)
    for i in range(gi.shape[0]):
        got = gi[i][gi[i] >= 0]
        if not 0 <= qf[i] < len(sets):
            assert got.shape[0] == 0, (tag, i)
            continue
        S, mode = sets[qf[i]]
        assert np.isin(got, all_ids).all(), (tag, i)
        inS = np.isin(got, S)
        assert inS.all() if mode == "allow" else not inS.any(), (tag, i)


def _filters(s, sets, dev=False):
    from quake_amd.capi import Filter
    return [Filter(s, torch.from_numpy(S).cuda() if dev else S, mode) for S, mode in sets]


def _close(fs):
    for f in fs:
        f.close()


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    """the corpus of tests/test_filtered_search.py: 20 000 rows in 64 skewed lists (empty ones, ones shorter than a tile)"""
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c = _corpus(d, 64, 20000, metric, seed=100 + d + (1 if metric == "ip" else 0))
            cache[(d, metric)] = (c,) + _stores(ctx, c)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


def _five_sets(ids, rng):
    """allow 0.5, allow 0.01, deny 0.1, allow-empty, deny-empty"""
    return [(Y.draw_set(ids, 0.5, rng), "allow"), (Y.draw_set(ids, 0.01, rng), "allow"), (Y.draw_set(ids, 0.1, rng), "deny"),
            (np.zeros(0, np.int64), "allow"), (np.zeros(0, np.int64), "deny")]


def _one_list_queries(c, Q, seed):
    """queries around the centroid of the longest list: with nprobe 1 they all probe that list and share its 16-query tiles"""
    rng = np.random.default_rng(seed)
    big = int(np.argmax(np.diff(c["offsets"])))
    q = (c["cent"][big] + 0.05 * rng.standard_normal((Q, c["d"]))).astype(np.float32)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        near = np.argmax(q @ c["cent"].T, axis=1)
    else:
        near = np.argmin(((q[:, None, :] - c["cent"][None, :, :]) ** 2).sum(-1), axis=1)
    assert (near == big).all()
    return np.ascontiguousarray(q)


# ---- 1. mixed tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mixed_tiles(ctx, corpora, metric):
    c, s, parent = corpora(128, metric)
    rng = np.random.default_rng(1201)
    Q = 53
    q = _one_list_queries(c, Q, seed=1202)
    sets = _five_sets(c["ids"], rng)
    qf = (np.arange(Q) % 5).astype(np.int32)
    fs = _filters(s, sets)
    for nprobe in (1, 8):  # 8: the queries of a tile exchange bounds through gtau, each under its own filter
        for k in (1, 10, 100):
            gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filters=fs, query_filter=qf)
            assert ctx.last_scan_kernel() == PER_QUERY
            oi, od = _yard_search(q, c, nprobe, k, metric, qf, sets)
            _eq(gi, gd, oi, od, (nprobe, k))
            _own_filter_only(gi, c["ids"], qf, sets, (nprobe, k))
            assert (gi[qf == 3] == -1).all() and (gd[qf == 3] == _pad(metric)).all()  # allow-empty: all padding
            assert (gi[qf == 4] >= 0).all()
    _close(fs)
    # one filter per query, selectivities drawn by a seeded rng
    Q = 48
    q = np.ascontiguousarray(q[:Q])
    sel = rng.choice([0.9, 0.5, 0.1, 0.02, 0.003], size=Q)
    sets = [(Y.draw_set(c["ids"], float(sel[i]), rng), "allow" if rng.random() < 0.7 else "deny") for i in range(Q)]
    qf = rng.permutation(Q).astype(np.int32)
    fs = _filters(s, sets)
    for nprobe, k in [(1, 10), (8, 100)]:
        gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filters=fs, query_filter=qf)
        oi, od = _yard_search(q, c, nprobe, k, metric, qf, sets)
        _eq(gi, gd, oi, od, ("F = Q", nprobe, k))
        _own_filter_only(gi, c["ids"], qf, sets, ("F = Q", nprobe, k))
    _close(fs)


# ---- 2. a neighbour's rows are not mine ----------------------------------------------------------------------------------------------
def test_a_neighbours_rows_are_not_mine(ctx):
    """The layout of test_disallowed_near_rows_do_not_seed_a_bound: every list has a tight head of 128 rows far closer to the
    queries than anything else.  Filter A denies every head, filter B allows only the heads, and the queries alternate A, B, A,
    B ...: every tile of 16 lanes holds both, and the OR of the two masks is all ones -- the set of tiles that are read and the set
    of rows that are candidates are different things.  A kernel that tests a row against the union, or against another lane's
    word, fails here."""
    from quake_amd.capi import Store
    d, nlist, per = 64, 16, 600
    rng = np.random.default_rng(31)
    cent = (4.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    vecs = (cent[:, None, :] + 1.0 * rng.standard_normal((nlist, per, d))).astype(np.float32)
    vecs[:, :128, :] = cent[:, None, :] + 0.001 * rng.standard_normal((nlist, 128, d)).astype(np.float32)
    vecs = np.ascontiguousarray(vecs.reshape(-1, d))
    ids = np.arange(nlist * per, dtype=np.int64)
    offsets = np.arange(nlist + 1, dtype=np.int64) * per
    head = ids[(ids % per) < 128]
    Q = 64
    q = (cent[rng.integers(0, nlist, size=Q)] + 0.001 * rng.standard_normal((Q, d))).astype(np.float32)
    c = dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets)
    sets = [(head, "deny"), (head, "allow")]
    qf = (np.arange(Q) % 2).astype(np.int32)
    oi, od = _yard_search(q, c, 8, 10, "l2", qf, sets)
    assert (oi[qf == 0] >= 0).all() and not np.isin(oi[qf == 0], head).any()  # A: k rows, none of them a head
    assert np.isin(oi[qf == 1], head).all()                                      # B: heads only
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
    fs = _filters(s, sets)
    gi, gd = ctx.search(parent, s, q, 8, 10, "l2", filters=fs, query_filter=qf)
    _eq(gi, gd, oi, od, "A / B alternating")
    _own_filter_only(gi, ids, qf, sets, "A / B alternating")
    _close(fs)
    s.close()
    parent.close()


# ---- 3. disjoint tiles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 768])
def test_disjoint_tiles(ctx, d):
    """the 5-list store of test_tile_skipping; E allows the rows of even tiles, O those of odd tiles, S a single row of the last,
    partial tile of list 0: every tile is read for some query and holds nothing for the others"""
    from quake_amd.capi import Store
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
    Q = 40
    q = (vecs[rng.integers(0, n, size=Q)] + 0.05 * rng.standard_normal((Q, d))).astype(np.float32)
    pids = np.broadcast_to(np.arange(nlist, dtype=np.int64), (Q, nlist)).copy()
    row = np.arange(n) - offsets[assign]
    sets = [(ids[(row // 16) % 2 == 0], "allow"), (ids[(row // 16) % 2 == 1], "allow"),
            (ids[(assign == 0) & (row == 5002)], "allow")]
    assert sets[2][0].shape[0] == 1
    qf = (np.arange(Q) % 3).astype(np.int32)
    fs = _filters(s, sets)
    for k in (1, 10, 100):
        gi, gd = ctx.scan(s, q, pids, k, "l2", filters=fs, query_filter=qf)
        assert ctx.last_scan_kernel() == PER_QUERY
        oi, od = _scatter(Q, k, "l2", qf, sets, lambda rows, S, mode: Y.scan(
            np.ascontiguousarray(q[rows]), vecs, ids, offsets, pids[rows], k, "l2", S, mode))
        _eq(gi, gd, oi, od, k)
        _own_filter_only(gi, ids, qf, sets, k)
        assert (gi[qf == 2][:, 0] == sets[2][0][0]).all() and (gi[qf == 2][:, 1:] == -1).all()
    _close(fs)
    s.close()


# ---- 4. nothing in the union -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_nothing_in_the_union(ctx, corpora, metric):
    c, s, parent = corpora(128, metric)
    q = _queries(c, 37, seed=1401)
    sets = [(np.zeros(0, np.int64), "allow"), (np.array([-3, 10 ** 13, 10 ** 13 + 5], np.int64), "allow")]
    qf = (np.arange(37) % 2).astype(np.int32)
    fs = _filters(s, sets)
    for nprobe, k in [(1, 10), (8, 100)]:
        gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filters=fs, query_filter=qf)  # (raises unless QK_OK)
        assert (gi == -1).all() and (gd == _pad(metric)).all()
    _close(fs)


# ---- 5. F = 1 is the single-filter call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_one_filter_is_the_single_filter_call(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent = corpora(128, metric)
    q = _queries(c, 300, seed=9)
    f = Filter(s, Y.draw_set(c["ids"], 0.3, np.random.default_rng(1501)), "allow")
    qf = np.zeros(300, np.int32)
    for nprobe, k in [(1, 10), (8, 10), (32, 100)]:
        si, sd = ctx.search(parent, s, q, nprobe, k, metric, filter=f)
        assert ctx.last_scan_kernel() == "k_scan (filtered)"
        gi, gd = ctx.search(parent, s, q, nprobe, k, metric, filters=[f], query_filter=qf)
        assert ctx.last_scan_kernel() == PER_QUERY
        _eq(gi, gd, si, sd, (nprobe, k))
    f.close()


# ---- 6. stale masks and stale union --------------------------------------------------------------------------------------------------
def test_stale_masks_and_stale_union():
    """Three sparse allow-filters on an index of the Python mirror.  40 rows are added AT the queries (each becomes its query's
    nearest row, at the end of a list: in tiles whose words were zero in every mask, or that did not exist); only filter 0 allows
    their ids.  The next search must rebuild each mask once AND the union of the three: with a stale union those tiles are not read."""
    import quake_amd as quake
    g = torch.Generator().manual_seed(1601)
    n, d, Q = 6000, 32, 40
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(Q, d, generator=g)
    new_ids = np.arange(100000, 100000 + Q, dtype=np.int64)
    rng = np.random.default_rng(1602)
    base = [Y.draw_set(ids.numpy(), 0.02, rng) for _ in range(3)]
    sets = [(np.concatenate([base[0], new_ids]), "allow"), (base[1], "allow"), (base[2], "allow")]
    qf = (np.arange(Q) % 3).astype(np.int32)
    idx = _build(quake, x, ids, 20)
    sp = quake.SearchParams()
    sp.k, sp.nprobe = 10, 5
    sp.filters = [idx.make_filter(torch.from_numpy(S)) for S, _ in sets]
    sp.query_filter = torch.from_numpy(qf)

    def check(tag):
        cent, cids, cv, ci, co = _index_csr(idx)
        r = idx.search(q, sp)
        oi, od = _scatter(Q, sp.k, "l2", qf, sets, lambda rows, S, mode: Y.search(
            np.ascontiguousarray(q.numpy()[rows]), cent, cv, ci, co, sp.nprobe, sp.k, "l2", S, mode, centroid_ids=cids))
        _eq(r.ids, r.distances, oi, od, tag)
        _own_filter_only(r.ids, ci, qf, sets, tag)
        return r.ids.numpy()

    def rebuilds():
        return [f.info()["rebuilds"] for f in sp.filters]

    check("as built")
    r0 = rebuilds()
    idx.add(q.clone(), torch.from_numpy(new_ids))
    gi = check("after add")
    assert (gi[qf == 0][:, 0] == new_ids[qf == 0]).all()  # filter 0: the new row of the query itself comes first
    assert not np.isin(gi[qf != 0], new_ids).any()         # nobody else sees the new ids
    assert rebuilds() == [v + 1 for v in r0]
    check("nothing changed")
    assert rebuilds() == [v + 1 for v in r0]
    idx.remove(torch.from_numpy(new_ids))
    gi = check("after remove")
    assert not np.isin(gi, new_ids).any()
    assert rebuilds() == [v + 2 for v in r0]


# ---- 7. wide rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    d, Q = 3072, 20
    rng = np.random.default_rng(1701)
    sizes = np.array([301, 288, 317, 296, 305, 293], np.int64)
    nlist = sizes.shape[0]
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), sizes)
    vecs = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) + 5
    c = dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets, x=vecs, d=d, metric=metric)
    s, parent = _stores(ctx, c)
    q = _queries(c, Q, seed=1702)
    # uniform 10 %, a contiguous run inside one list (whole tiles without a candidate elsewhere), deny 50 %
    sets = [(Y.draw_set(ids, 0.1, rng), "allow"), (ids[offsets[2] + 40: offsets[2] + 90], "allow"), (Y.draw_set(ids, 0.5, rng), "deny")]
    qf = (np.arange(Q) % 3).astype(np.int32)
    fs = _filters(s, sets)
    gi, gd = ctx.search(parent, s, q, 3, 10, metric, filters=fs, query_filter=qf)
    assert ctx.last_scan_kernel() == PER_QUERY_WIDE
    oi, od = _yard_search(q, c, 3, 10, metric, qf, sets)
    _eq(gi, gd, oi, od, metric)
    _own_filter_only(gi, ids, qf, sets, metric)
    _close(fs)
    s.close()
    parent.close()


# ---- 8. memory spaces and entry points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_memory_spaces_and_entry_points(ctx, corpora, dev):
    c, s, parent = corpora(128, "l2")
    rng = np.random.default_rng(1801)
    Q, nprobe, k = 53, 4, 10
    q = _queries(c, Q, seed=1802)
    sets = _five_sets(c["ids"], rng)
    qf = (np.arange(Q) % 5).astype(np.int32)
    oi, od = _yard_search(q, c, nprobe, k, "l2", qf, sets)
    fs = _filters(s, sets, dev)
    xq = torch.from_numpy(q).cuda() if dev else q
    qfm = torch.from_numpy(qf).cuda() if dev else qf
    gi, gd = ctx.search(parent, s, xq, nprobe, k, "l2", filters=fs, query_filter=qfm)
    ctx.synchronize()
    _eq(gi, gd, oi, od, "search")
    ti, td, tp = ctx.search_tracked(parent, s, xq, nprobe, k, "l2", filters=fs, query_filter=qfm)
    ui, ud, up = ctx.search_tracked(parent, s, xq, nprobe, k, "l2")
    ctx.synchronize()
    _eq(ti, td, oi, od, "search_tracked")
    np.testing.assert_array_equal(_np(tp), _np(up))  # the probed lists are the unfiltered call's
    pids, _ = ctx.coarse(parent, xq, nprobe, "l2")
    ci, cd = ctx.scan(s, xq, pids, k, "l2", filters=fs, query_filter=qfm)
    ctx.synchronize()
    _eq(ci, cd, oi, od, "coarse + scan")
    _own_filter_only(ci, c["ids"], qf, sets, "coarse + scan")
    if dev:
        # a device qfilter is not read by the host: numbers outside [0, F) give those queries all-padding rows, nothing faults
        bad = qf.copy()
        bad[7], bad[30] = 5, -1
        gi, gd = ctx.search(parent, s, xq, nprobe, k, "l2", filters=fs, query_filter=torch.from_numpy(bad).cuda())
        ctx.synchronize()
        bi, bd = _yard_search(q, c, nprobe, k, "l2", bad, sets)
        assert (bi[[7, 30]] == -1).all()
        _eq(gi, gd, bi, bd, "out-of-range filter numbers")
    _close(fs)


# ---- 9. both mirrors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


@pytest.mark.parametrize("nlist", [0, 20])
def test_both_mirrors(qb, nlist):
    import quake_amd as quake
    g = torch.Generator().manual_seed(1901)
    n, d, Q = 6000, 32, 53
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(Q, d, generator=g)
    sets = _five_sets(ids.numpy(), np.random.default_rng(1902))
    qf = (np.arange(Q) % 5).astype(np.int32)
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, nlist)
        sp = mod.SearchParams()
        assert list(sp.filters) == [] and sp.query_filter is None
        before = repr(sp)
        sp.k, sp.nprobe = 10, 5
        plain = idx.search(q, sp)
        sp.filters = [idx.make_filter(torch.from_numpy(S), mode == "deny") for S, mode in sets]
        sp.query_filter = torch.from_numpy(qf)
        for track in (False, True):
            if name == "python":
                idx.track_hits = track
            else:
                idx.set_track_hits(track)
            r = idx.search(q, sp)
            rd = idx.search(q.cuda(), sp)  # device tensors
            assert torch.equal(rd.ids.cpu(), r.ids) and torch.equal(rd.distances.cpu(), r.distances)
            out[(name, track)] = (r.ids.numpy(), r.distances.numpy())
            _own_filter_only(r.ids, ids.numpy(), qf, sets, (name, track))
        if name == "python":
            idx.track_hits = False
        else:
            idx.set_track_hits(False)
        sp.filters = []
        sp.query_filter = None
        assert "filter" not in before and repr(mod.SearchParams()) == before  # the summary does not know the extension
        again = idx.search(q, sp)
        assert torch.equal(again.ids, plain.ids)
        if name == "python":  # the yardstick over the index's own partitions
            if nlist == 0:
                pv, pi = idx._store.get_list(0)
                offs = np.array([0, n], np.int64)
                oi, od = _scatter(Q, 10, "l2", qf, sets, lambda rows, S, mode: Y.search(
                    np.ascontiguousarray(q.numpy()[rows]), None, pv, pi, offs, 1, 10, "l2", S, mode))
            else:
                cent, cids, cv, ci, co = _index_csr(idx)
                oi, od = _scatter(Q, 10, "l2", qf, sets, lambda rows, S, mode: Y.search(
                    np.ascontiguousarray(q.numpy()[rows]), cent, cv, ci, co, 5, 10, "l2", S, mode, centroid_ids=cids))
            for track in (False, True):
                _eq(*out[(name, track)], oi, od, (nlist, track))
    for track in (False, True):  # (both mirrors ran the same k-means: the same partitions, the same tensors)
        np.testing.assert_array_equal(out[("python", track)][0], out[("compiled", track)][0])
        np.testing.assert_array_equal(out[("python", track)][1].view(np.uint32), out[("compiled", track)][1].view(np.uint32))


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_abi(ctx, corpora):
    from quake_amd.capi import QK_MAX_BATCH_FILTERS, Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(128, "l2")
    c2, s2, parent2 = corpora(128, "ip")
    Q = 8
    q = _queries(c, Q, seed=3)
    S = c["ids"][:4000]
    f = Filter(s, S, "allow")
    f2 = Filter(s2, c2["ids"][:100], "allow")
    qf = np.zeros(Q, np.int32)
    pids1 = np.zeros((Q, 1), np.int64)
    oi, od = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", S, "allow")

    def still_answers(tag):
        gi, gd = ctx.search(parent, s, q, 4, 10, "l2", filters=[f], query_filter=qf)
        _eq(gi, gd, oi, od, tag)

    def raw(filters_arr, F, qfilter, k=10):
        """qk_search_filtered_batch with host buffers, as given"""
        out_i, out_d = np.empty((Q, k), np.int64), np.empty((Q, k), np.float32)
        return ctx.lib.qk_search_filtered_batch(ctx.h, parent.h, s.h, q.ctypes.data_as(C.c_void_p), Q, 4, k, 1, filters_arr, F,
                                                qfilter.ctypes.data_as(C.c_void_p), out_i.ctypes.data_as(C.c_void_p),
                                                out_d.ctypes.data_as(C.c_void_p), 0, None)

    one = (C.c_void_p * 1)(f.h)
    assert raw(one, 0, qf) == 1 and b"F=0" in ctx.lib.qk_last_error()  # QK_ERR_INVALID
    still_answers("F < 1")
    assert raw((C.c_void_p * 2)(f.h, None), 2, qf) == 1 and b"null" in ctx.lib.qk_last_error()
    still_answers("null handle")
    many = (C.c_void_p * (QK_MAX_BATCH_FILTERS + 1))(*([f.h] * (QK_MAX_BATCH_FILTERS + 1)))
    assert raw(many, QK_MAX_BATCH_FILTERS + 1, qf) == 4 and b"QK_MAX_BATCH_FILTERS" in ctx.lib.qk_last_error()  # QK_ERR_UNSUPPORTED
    still_answers("F > QK_MAX_BATCH_FILTERS")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search(parent, s, q, 4, 10, "l2", filters=[f, f2], query_filter=qf)
    still_answers("another store's filter")
    for bad in (1, -1):
        qb_ = qf.copy()
        qb_[5] = bad
        with pytest.raises(QuakeHipError, match=r"QK_ERR_INVALID.*outside \[0, F=1\)"):
            ctx.search(parent, s, q, 4, 10, "l2", filters=[f], query_filter=qb_)
        with pytest.raises(QuakeHipError, match=r"QK_ERR_INVALID.*outside \[0, F=1\)"):
            ctx.scan(s, q, pids1, 10, "l2", filters=[f], query_filter=qb_)
        with pytest.raises(QuakeHipError, match=r"QK_ERR_INVALID.*outside \[0, F=1\)"):
            ctx.search_tracked(parent, s, q, 4, 10, "l2", filters=[f], query_filter=qb_)
    still_answers("host qfilter out of range")
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.search(parent, s, q, 4, QK_MAX_K + 1, "l2", filters=[f], query_filter=qf)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.scan(s, q, pids1, QK_MAX_K + 1, "l2", filters=[f], query_filter=qf)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.search_tracked(parent, s, q, 4, QK_MAX_K + 1, "l2", filters=[f], query_filter=qf)
    still_answers("k > QK_MAX_K")
    # the wrapper's own argument rules
    with pytest.raises(ValueError, match="exclusive"):
        ctx.search(parent, s, q, 4, 10, "l2", filter=f, filters=[f], query_filter=qf)
    with pytest.raises(ValueError, match="together"):
        ctx.search(parent, s, q, 4, 10, "l2", filters=[f])
    with pytest.raises(ValueError, match="together"):
        ctx.scan(s, q, pids1, 10, "l2", query_filter=qf)
    with pytest.raises(ValueError, match="one entry per query"):
        ctx.search(parent, s, q, 4, 10, "l2", filters=[f], query_filter=qf[:5])
    still_answers("wrapper refusals")
    f.close()
    f2.close()


def test_refusals_of_both_mirrors(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(71)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    Q = 10
    qq = torch.randn(Q, 16, generator=g)
    qf = torch.zeros(Q, dtype=torch.int32)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        grp = _build(mod, x, ids, 16, workers=2)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        f = idx.make_filter(ids[:1000])
        sp.filter = f
        single = idx.search(qq, sp)
        sp.filter = None

        def valid(tag):
            sp.filters, sp.query_filter = [f], qf
            r = idx.search(qq, sp)
            assert torch.equal(r.ids, single.ids) and torch.equal(r.distances, single.distances), tag

        valid("first")
        sp.filter = f
        with pytest.raises(RuntimeError, match="exclusive"):
            idx.search(qq, sp)
        sp.filter = None
        valid("both filter and filters")
        sp.query_filter = None
        with pytest.raises(RuntimeError, match="together"):
            idx.search(qq, sp)
        sp.filters, sp.query_filter = [], qf
        with pytest.raises(RuntimeError, match="together"):
            idx.search(qq, sp)
        valid("only one of the pair")
        sp.query_filter = qf[:7]
        with pytest.raises(RuntimeError, match="one entry per query"):
            idx.search(qq, sp)
        valid("query_filter of another length")
        sp.filters = [f, other.make_filter(ids[:1000])]
        with pytest.raises(RuntimeError, match="another"):
            idx.search(qq, sp)
        valid("a filter of another index")
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.search(qq, sp)
        sp.recall_target = -1.0
        valid("recall_target")
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.search(qq, sp)
        valid("num_workers")
        sp.k = QK_MAX_K + 1
        with pytest.raises(RuntimeError, match="QK_MAX_K"):
            idx.search(qq, sp)
        sp.k = 5
        valid("k > QK_MAX_K")
        sp.filters, sp.query_filter = [], None
        assert tuple(grp.search(qq, sp).ids.shape) == (Q, 5)
