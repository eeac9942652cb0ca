"""Search over NaN, Inf and overflowing values on the device (the contract: DESIGN.md 5.8.1, include/quake_hip.h) against the oracle,
whose rule tests/test_nonfinite_oracle.py pins: a (query, row) pair whose canonical value is NaN is never a candidate, +-inf are
ordinary values in front of the padding, -0 and +0 tie and the lower id goes first.

tests/nonfinite_yardstick.py plants special rows of one input class (NaN, Inf, overflow, underflow / zero) into an ordinary corpus --
first tile, last partial tile, inside the 128-row head that seeds a bound, a list of five specials only -- and aims queries, some of
them special themselves, at those lists.  Every class goes, under L2 and IP, through every path that computes a key: the shapes are
the ones tests/test_scan_form_selection_gpu.py pins as the smallest that select each form, and the form is asserted.  Ids are
compared exactly, distances as uint32 (zeros by value), and every answer is also checked directly: no id of a NaN pair appears.

(Named like test_range_search.py and test_filtered_search.py: a *_gpu.py file needs a stated place in conftest.collection_rank.  The
AST walk of test_suite_is_deterministic.py therefore does not read this file; no test here reads a clock or builds a cost model.)"""
import numpy as np
import pytest

import filter_yardstick as FY
import nonfinite_yardstick as NF
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu

SHORT = (60000, 1024, 128)   # 58 rows per list
LONG = (100000, 64, 128)     # 1560 rows per list
WIDE = (2400, 12, 3072)      # the row count of test_wide_dim.py::test_search_and_scan_bit_exact


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    c.set_form_feedback(False)  # which form answers is asserted: the static rule alone
    yield c
    for _, parent, s in _CACHE.values():
        s.close()
        parent.close()
    _CACHE.clear()
    c.close()


_CACHE = {}


def _parent(ctx, cent, ids=None):
    from quake_amd.capi import Store
    n, d = cent.shape
    p = Store(ctx, d)
    p.build_csr(np.array([0, n], np.int64), np.arange(n, dtype=np.int64) if ids is None else ids, cent)
    return p


def _case(ctx, cls, metric, shape):
    """(corpus, parent store, store) of one class on one shape, kept while the next test wants the same class and metric"""
    key = (cls, metric) + shape
    if key not in _CACHE:
        for k_ in [k_ for k_ in _CACHE if k_[:2] != (cls, metric)]:
            _, parent, s = _CACHE.pop(k_)
            s.close()
            parent.close()
        from quake_amd.capi import Store
        n, nlist, d = shape
        c = NF.corpus(cls, metric, n, nlist, d, seed=5 + d)
        s = Store(ctx, d)
        s.build_csr(c["offsets"], c["ids"], c["vecs"])
        _CACHE[key] = (c, _parent(ctx, c["centroids"]), s)
    return _CACHE[key]


def _check(c, q, special, gi, gd, oi, od):
    NF.assert_same_answer(gi, gd, oi, od)
    NF.assert_no_nan_pair(c, q, special, gi)


# (form, shape, k, Q, nprobe): the table of the issue; None = the path has no name of its own (k > QK_MAX_K: the key-emission scan)
FORMS = [
    ("k_scan", SHORT, 10, 1024, 1),
    ("k_scan_rl", SHORT, 10, 256, 4),
    ("k_search_small", SHORT, 10, 32, 10),
    ("k_search_small", SHORT, 10, 1, 10),
    (None, SHORT, 1000, 48, 4),
    ("k_scan (query-sharing)", LONG, 32, 1024, 8),
    ("k_scan_rl (mixed)", LONG, 10, 1024, 8),
    ("k_scan_wide", WIDE, 10, 33, 8),
]


# (the decorator nearest the function varies slowest: all forms of one class and metric run side by side, on one cached corpus)
@pytest.mark.parametrize("form,shape,k,nq,nprobe", FORMS, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, tuple) else "x".join(map(str, v)))
@pytest.mark.parametrize("cls", NF.CLASSES)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_every_scan_form(ctx, form, shape, k, nq, nprobe, cls, metric):
    c, parent, s = _case(ctx, cls, metric, shape)
    q, special = NF.queries(c, nq, seed=6)
    NF.assert_special_queries_meet_specials(c, q, special, nprobe)
    if form == "k_scan_rl (mixed)":  # hot lists (>= 18 probing queries) and a cold one, each with planted rows
        _, cnt = NF.probe_counts(c, q, nprobe)
        assert min(cnt[h] for h in c["hosts"]) >= 18 and 1 <= cnt[c["tiny"]] < 18, (cnt[list(c["hosts"])], cnt[c["tiny"]])
    gi, gd = ctx.search(parent, s, q, nprobe, k, metric)
    if form is not None:
        assert ctx.last_scan_kernel() == form
    oi, od = NF.expected(c, q, nprobe, k)
    _check(c, q, special, gi, gd, oi, od)
    if cls == "nan" and nq > 1:
        np.testing.assert_array_equal(gi[1], -1)  # the all-NaN query: padding only
        assert (gd[1] == (-np.inf if metric == "ip" else np.inf)).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_tracked_search_and_scan_of_given_lists(ctx, cls, metric):
    """qk_search_tracked (the probed lists are the oracle's coarse answer, -1 where no centroid is left) and qk_scan over given
    lists: the list of five specials and a list that holds planted ones, for every query -- in the underflow class that is the
    signed-zero pair under its own query (the lower id sits on the -0.0 row)"""
    c, parent, s = _case(ctx, cls, metric, SHORT)
    q, special = NF.queries(c, 256, seed=6)
    gi, gd, gp = ctx.search_tracked(parent, s, q, 4, 10, metric)
    assert ctx.last_scan_kernel() == "k_scan_rl"
    oi, od = NF.expected(c, q, 4, 10)
    _check(c, q, special, gi, gd, oi, od)
    op, _ = O.coarse(q, c["centroids"], None, 4, metric, num_threads=8)
    np.testing.assert_array_equal(gp, op)
    pids = np.array([c["tiny"], c["hosts"][0]], np.int64)
    gi, gd = ctx.scan(s, q, pids, 10, metric)
    oi, od = O.batched_serial_scan(q, c["vecs"], c["ids"], c["offsets"], pids, 10, metric, num_threads=8)
    _check(c, q, special, gi, gd, oi, od)
    gi, gd = ctx.scan(s, q[8:11], pids[:1], 10, metric)  # five rows for k = 10: everything that is not NaN, then the padding
    oi, od = O.batched_serial_scan(q[8:11], c["vecs"], c["ids"], c["offsets"], pids[:1], 10, metric)
    NF.assert_same_answer(gi, gd, oi, od)
    np.testing.assert_array_equal(gi[:, 5:], -1)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_filtered_and_per_query_filtered(ctx, cls, metric):
    """selectivity 0.5, specials on both sides of every filter; four filters for the per-query form"""
    from quake_amd.capi import Filter
    c, parent, s = _case(ctx, cls, metric, SHORT)
    q, special = NF.queries(c, 256, seed=6)
    rng = np.random.default_rng(7)
    sets = []
    for f in range(4):
        S = FY.draw_set(c["ids"][c["ids"] >= 15], 0.5, rng)
        sets.append(np.concatenate([S, np.arange(15, dtype=np.int64)[(np.arange(15) + f) % 2 == 0]]))
    filters = [Filter(s, S, "allow") for S in sets]
    try:
        gi, gd = ctx.search(parent, s, q, 4, 10, metric, filter=filters[0])
        assert ctx.last_scan_kernel() == "k_scan (filtered)"
        oi, od = FY.search(q, c["centroids"], c["vecs"], c["ids"], c["offsets"], 4, 10, metric, sets[0], "allow")
        _check(c, q, special, gi, gd, oi, od)
        qf = (np.arange(q.shape[0]) % 4).astype(np.int32)
        gi, gd = ctx.search(parent, s, q, 4, 10, metric, filters=filters, query_filter=qf)
        assert ctx.last_scan_kernel() == "k_scan (filtered, per query)"
        for f in range(4):
            oi, od = FY.search(q[qf == f], c["centroids"], c["vecs"], c["ids"], c["offsets"], 4, 10, metric, sets[f], "allow")
            NF.assert_same_answer(gi[qf == f], gd[qf == f], oi, od)
        NF.assert_no_nan_pair(c, q, special, gi)
    finally:
        for f in filters:
            f.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_range_search(ctx, cls, metric):
    """a finite radius (L2 4.0: about the distance of a query to the rows of its own cluster, 0.3 noise per coordinate at d = 128; IP
    0.8 on unit vectors) and the widest one: every row of the probed lists that is not a NaN pair comes back, +-inf ones included;
    lims exact"""
    c, parent, s = _case(ctx, cls, metric, SHORT)
    q, special = NF.queries(c, 40, seed=6)
    for radius in ((4.0, np.inf) if metric == "l2" else (0.8, -np.inf)):
        gl, gi, gd = ctx.range_search(parent, s, q, 4, radius, metric)
        ol, oi, od = RY.search(q, c["centroids"], c["vecs"], c["ids"], c["offsets"], 4, radius, metric)
        np.testing.assert_array_equal(gl, ol)
        NF.assert_same_answer(gi, gd, oi, od)
        assert not np.isnan(gd).any()
        for i in range(q.shape[0]):  # (the direct check wants one row of ids per query)
            NF.assert_no_nan_pair(c, q[i:i + 1], np.zeros(1 if i in special else 0, np.int64), gi[None, gl[i]:gl[i + 1]])


# ---- the coarse step: NaN / Inf / 2^64 centroids ----------------------------------------------------------------------------------
# (kernel, centroids, queries): the smallest counts at which test_dense_fused_gpu.py, test_dense_pf_gpu.py and
# test_scan_gpu.py::test_mid_sized_batches_one_launch_coarse reach each form at nprobe 8 and 32 -- 1000 centroids x 64 queries is inside
# k_coarse_small's envelope (<= 256 queries, <= 256 K pairs) and 8005 x 40 outside it and under the 64 queries of the other two,
# which leaves the key matrix (both report "k_dense"); nprobe 1 is the nearest-centroid kernel (k_dense_argmin) at all four
COARSE = [("k_dense_fused", 1024, 300), ("k_dense_pf", 5000, 300), ("k_dense", 8005, 40), ("k_dense", 1000, 64)]


def _centroids(cls, metric, n, nq, few=False):
    rng = np.random.default_rng(n + nq)
    cent = rng.standard_normal((n, 128)).astype(np.float32)
    if metric == "ip":
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    clean = cent.copy()
    pos = np.array([1, 2, 70, n // 2, n - 1])
    cent[pos] = NF.special_rows(cls, cent[pos])
    if few:  # ten centroids are left without a NaN
        bad = np.ones(n, bool)
        bad[rng.choice(n, 10, replace=False)] = False
        bad[pos] = True
        cent.view(np.uint32)[bad, 9] = 0x7FC00000
    c = dict(centroids=clean, x=clean, hosts=(1, 2), tiny=70, cls=cls, metric=metric, d=128)
    q, special = NF.queries(c, nq, seed=n)  # (aimed at where the planted centroids were; the class's special queries)
    return cent, q, special


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", ["nan", "inf", "overflow"])
@pytest.mark.parametrize("kernel,n,nq", COARSE)
def test_coarse_kernels(ctx, kernel, n, nq, cls, metric):
    cent, q, special = _centroids(cls, metric, n, nq)
    parent = _parent(ctx, cent)
    try:
        for nprobe in (1, 8, 32):
            gp, gd = ctx.coarse(parent, q, nprobe, metric)
            assert ctx.last_scan_kernel() == ("k_dense" if nprobe == 1 else kernel)
            op, od = O.coarse(q, cent, None, nprobe, metric, num_threads=8)
            NF.assert_same_answer(gp, gd, op, od)
            val = O.pair_values(q, cent, metric)
            for i in range(nq):
                assert not np.isin(gp[i], np.nonzero(np.isnan(val[i]))[0]).any()
    finally:
        parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kernel,n,nq", COARSE)
def test_coarse_with_fewer_centroids_than_nprobe(ctx, kernel, n, nq, metric):
    """all but ten centroids hold a NaN: nprobe 32 answers those ten and 22 times -1"""
    cent, q, special = _centroids("nan", metric, n, nq, few=True)
    parent = _parent(ctx, cent)
    try:
        for nprobe in (1, 32):
            gp, gd = ctx.coarse(parent, q, nprobe, metric)
            assert ctx.last_scan_kernel() == ("k_dense" if nprobe == 1 else kernel)
            op, od = O.coarse(q, cent, None, nprobe, metric, num_threads=8)
            NF.assert_same_answer(gp, gd, op, od)
        live = np.ones(nq, bool)
        live[special] = False
        np.testing.assert_array_equal(gp[:, 10:], -1)
        assert (gp[live, :10] >= 0).all() and not np.isnan(cent[gp[live, :10]]).any()
    finally:
        parent.close()


# ---- nprobe 1 over 40960+ queries: the coarse step runs on the k-means assign's prefiltered kernels (k_assign_pf) -------------------
HUGE = 40960  # qk_assign_pf_supported: from this many rows on (64+ centroids, d % 8 == 0, d <= 128)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", ["nan", "inf", "overflow"])
def test_nearest_list_of_a_huge_batch_with_special_centroids(ctx, cls, metric):
    """one query short of the hand-over and at it: the same answer, the oracle's -- no NaN centroid, -1 for the all-NaN query"""
    cent, q0, special = _centroids(cls, metric, 256, 64)
    q = np.ascontiguousarray(np.tile(q0, (HUGE // 64, 1)))
    op, od = O.coarse(q0, cent, None, 1, metric)
    parent = _parent(ctx, cent)
    try:
        for n, kernel in ((HUGE, "k_assign_pf"), (HUGE - 1, "k_dense")):
            gp, gd = ctx.coarse(parent, q[:n], 1, metric)
            assert ctx.last_scan_kernel() == kernel
            NF.assert_same_answer(gp, gd, np.tile(op, (HUGE // 64, 1))[:n], np.tile(od, (HUGE // 64, 1))[:n])
        val = O.pair_values(q0, cent, metric)
        for i in range(64):
            assert not np.isin(gp[i], np.nonzero(np.isnan(val[i]))[0]).any()
        if cls == "nan":
            assert (gp[1::64] == -1).all()
    finally:
        parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_search_of_a_huge_batch(ctx, cls, metric):
    """qk_search with nprobe 1 takes the same coarse kernel (its packed list numbers go straight to the scan)"""
    c, parent, s = _case(ctx, cls, metric, (20000, 256, 128))
    q0, special = NF.queries(c, 64, seed=6)
    q = np.ascontiguousarray(np.tile(q0, (HUGE // 64, 1)))
    ctx.coarse(parent, q, 1, metric)
    assert ctx.last_scan_kernel() == "k_assign_pf"
    gi, gd = ctx.search(parent, s, q, 1, 10, metric)
    oi, od = NF.expected(c, q0, 1, 10)
    NF.assert_same_answer(gi, gd, np.tile(oi, (HUGE // 64, 1)), np.tile(od, (HUGE // 64, 1)))
    NF.assert_no_nan_pair(c, q0, special, gi[:64])


# ---- the two host mirrors, and the forms against each other ------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", ["python", "compiled"])
def test_mirrors_store_a_nan_row_and_never_return_it(mirror):
    import torch
    if mirror == "python":
        import quake_amd as mod
    else:
        from quake_amd.build_ext import build_bindings
        build_bindings()
        import quake_amd.bindings as mod
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3000, 32, generator=g)
    q = torch.nn.functional.normalize(torch.randn(40, 32, generator=g))
    idx = mod.QuakeIndex()
    bp = mod.IndexBuildParams()
    bp.nlist, bp.metric = 12, "ip"
    idx.build(x, torch.arange(3000), bp)
    sp = mod.SearchParams()
    sp.k, sp.nprobe = 10, 12
    before = idx.search(q, sp)
    nx = torch.nn.functional.normalize(torch.randn(4, 32, generator=g))
    nx[2, 5] = float("nan")
    nid = torch.arange(3000, 3004)
    idx.add(nx, nid)
    assert idx.ntotal() == 3004
    stored = idx.search(q, sp)
    assert not (stored.ids == 3002).any() and not torch.isnan(stored.distances).any()
    idx.remove(torch.tensor([3002]))
    without = idx.search(q, sp)
    np.testing.assert_array_equal(stored.ids.numpy(), without.ids.numpy())  # the stored NaN row changed no answer
    np.testing.assert_array_equal(stored.distances.numpy().view(np.uint32), without.distances.numpy().view(np.uint32))
    idx.remove(torch.tensor([3000, 3001, 3003]))
    after = idx.search(q, sp)
    np.testing.assert_array_equal(before.ids.numpy(), after.ids.numpy())
    np.testing.assert_array_equal(before.distances.numpy().view(np.uint32), after.distances.numpy().view(np.uint32))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_forms_agree_on_the_bits(metric):
    """one store, one batch, the form chosen by the feedback rule under injected figures (test_scan_feedback_gpu.py: on this shape
    all three forms are admissible and the first eight calls try each): tile form, per-wave walk and mixed sequence give the same bits"""
    import torch
    from quake_amd.capi import Context, Store
    ctx = Context(0)
    ctx.set_form_feedback(True)
    c = NF.corpus("nan", metric, 200000, 64, 64, seed=21)
    s = Store(ctx, 64)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = _parent(ctx, c["centroids"])
    q, special = NF.queries(c, 1024, seed=23)
    oi, od = NF.expected(c, q, 4, 10)
    qd = torch.from_numpy(q).cuda()
    forms = set()
    for _ in range(8):
        ctx.set_form_times((3.0, 2.0, 1.0))
        gi, gd = ctx.search(parent, s, qd, 4, 10, metric)
        torch.cuda.synchronize()  # (the measurement in flight is harvested by the next call)
        forms.add(ctx.last_scan_kernel())
        _check(c, q, special, gi.cpu().numpy(), gd.cpu().numpy(), oi, od)
    assert "k_scan_rl" in forms and "k_scan_rl (mixed)" in forms and forms & {"k_scan", "k_scan (query-sharing)"}, forms
    s.close()
    parent.close()
    ctx.close()
