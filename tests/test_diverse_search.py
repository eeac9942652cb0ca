"""Diversified search (qk_diverse_search / qk_diverse_scan; Context.diverse_search / diverse_scan; QuakeIndex.diverse_search in
both mirrors): per query, k of its fetch_k nearest rows chosen greedily by maximal marginal relevance.

Every comparison is exact equality of ids, distance bits and ranks with tests/diverse_yardstick.py (pinned on the CPU by
tests/test_diverse_oracle.py).  The candidates and pairwise values of a situation are computed once per fetch_k
(diverse_yardstick.prepare) and shared by the k and lambda of that situation.  No assertion reads a clock.  Every test asserts on
its own inputs that the situation it is about occurs."""
import ctypes as C

import numpy as np
import pytest
import torch

import diverse_yardstick as DY
import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu

NAMES = DY.NAMES
LAMBDAS = (0.0, 0.3, 0.5, 1.0)
FETCH = (1, 2, 17, 64, 65, 256)
STAGE_ALL_BYTES = 144 << 10     # qk_diverse.hip: a query's rows are staged in LDS while C * (dpad + 4) * 4 bytes fit this


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    assert len(got) >= 3
    for name, g, w in zip(NAMES, got, want):
        g, w = _np(g), _np(w)
        if name == "dist":
            g, w = np.ascontiguousarray(g, np.float32).view(np.uint32), np.ascontiguousarray(w, np.float32).view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, tag))


def _stores(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def corpus(d, nlist, n, metric, seed, empty=2, dup=0.25):
    """RY.corpus with near-duplicates planted: a fraction `dup` of the rows are exact copies of other rows of their list (same
    vector, another id) -- the case the feature exists for, and the source of equal distances and equal costs"""
    c = RY.corpus(d, nlist, n, metric, seed, empty=empty)
    rng = np.random.default_rng(seed + 7)
    offs = c["offsets"]
    ncopy = 0
    for p in range(nlist):
        lo, hi = int(offs[p]), int(offs[p + 1])
        m = int((hi - lo) * dup)
        if hi - lo < 4 or m == 0:
            continue
        dst = lo + rng.permutation(hi - lo)[:m]
        src = lo + rng.integers(0, hi - lo, size=m)
        c["vecs"][dst] = c["vecs"][src]
        ncopy += m
    assert dup == 0 or ncopy > 0
    return c


def shapes_in_lds(C_, d):
    return C_ * (((d + 15) // 16) * 16 + 4) * 4 <= STAGE_ALL_BYTES


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    """per (metric, d): a corpus of about 2500 rows in 12 lists (two empty, one of 5 and one of 7 rows) with planted copies, its
    stores and 17 queries; prepared candidates are memoised per situation"""
    cache = {}

    def get(metric, d=33):
        if (metric, d) not in cache:
            c = corpus(d, 12, 2500, metric, seed=401 + d + (0 if metric == "l2" else 1000))
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and 5 in sizes and 7 in sizes
            s, parent = _stores(ctx, c)
            cache[(metric, d)] = dict(c=c, s=s, parent=parent, q=RY.queries(c, 17, seed=402 + d), memo={}, metric=metric)
        return cache[(metric, d)]

    yield get
    for e in cache.values():
        e["s"].close()
        e["parent"].close()


def _prep(e, C_, nprobe=3, q=None, **kw):
    key = (C_, nprobe, None if q is None else q.tobytes(), tuple(sorted((k, str(v)) for k, v in kw.items() if k not in ("S", "pids"))),
           None if kw.get("S") is None else kw["S"].tobytes(), None if kw.get("pids") is None else kw["pids"].tobytes())
    if key not in e["memo"]:
        c = e["c"]
        cent = None if (nprobe is None or kw.get("pids") is not None) else c["cent"]
        e["memo"][key] = DY.prepare(e["q"] if q is None else q, cent, c["vecs"], c["ids"], c["offsets"], nprobe, C_, e["metric"], **kw)
    return e["memo"][key]


# ---- 1. the grid: dimension x fetch_k x k x lambda, both metrics ---------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 33, 96])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_grid(ctx, corpora, metric, d):
    e = corpora(metric, d)
    s, parent, q = e["s"], e["parent"], e["q"]
    reordered = ties = 0
    for C_ in FETCH:
        prep = _prep(e, C_)
        assert max(p[0].shape[0] for p in prep) == C_, "every query has fetch_k candidates here"
        assert shapes_in_lds(C_, d)
        ties += sum(int((np.diff(p[1]) == 0).sum()) for p in prep)
        for k in sorted({1, 2, C_} & set(range(1, C_ + 1))):
            for lam in LAMBDAS:
                want = DY.expected_batch(prep, k, lam, metric)
                got = ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric)
                _eq(got, want, (metric, d, C_, k, lam))
                reordered += int(((want[2] != np.arange(k)[None, :]) & (want[0] >= 0)).any())
                if lam == 1.0:
                    np.testing.assert_array_equal(want[2], np.where(want[0] >= 0, np.arange(k, dtype=np.int32)[None, :], -1))
    assert reordered >= 6, "the selection departs from the plain order in this grid"
    assert ties > 0, "planted copies give equal distances"


# ---- 2. batch sizes; a row is the call with that query alone -----------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_batch_sizes_and_row_independence(ctx, corpora, metric):
    e = corpora(metric)
    s, parent = e["s"], e["parent"]
    q65 = RY.queries(e["c"], 65, seed=411)
    for Q in (1, 17, 65):
        q = np.ascontiguousarray(q65[:Q])
        for C_, k, lam in ((64, 2, 0.3), (17, 17, 0.5), (65, 10, 0.0)):
            want = DY.expected_batch(_prep(e, C_, q=q), k, lam, metric)
            _eq(ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric), want, (metric, Q, C_, k, lam))
    full = ctx.diverse_search(parent, s, q65, 3, 10, 65, 0.3, metric)
    for qi in (0, 16, 17, 64):
        one = ctx.diverse_search(parent, s, np.ascontiguousarray(q65[qi:qi + 1]), 3, 10, 65, 0.3, metric)
        _eq(one, [f[qi:qi + 1] for f in full], ("alone", metric, qi))


# ---- 3. both forms of the selection kernel: the threshold between them, wide rows ----------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_staging_threshold(ctx, metric):
    """d = 200 (dpad 208): 173 candidates are the last whose rows fit the LDS budget, 174 take the form that re-reads the arena"""
    d = 200
    assert shapes_in_lds(173, d) and not shapes_in_lds(174, d)
    c = corpus(d, 6, 900, metric, seed=421, empty=0)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 5, seed=422)
    for C_ in (173, 174, 256):
        prep = DY.prepare(q, None, c["vecs"], c["ids"], c["offsets"], None, C_, metric)     # every list: 900 rows
        assert min(p[0].shape[0] for p in prep) == C_
        for k, lam in ((2, 0.5), (30, 0.3), (C_, 0.0)):
            _eq(ctx.diverse_search(None, s, q, 1, k, C_, lam, metric), DY.expected_batch(prep, k, lam, metric), (metric, C_, k, lam))
    s.close()
    parent.close()


@pytest.mark.parametrize("d", [2600, 4100])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric, d):
    """d = 2600: the wide-row scan finds the candidates; d = 4100: a row (and the staged vector) is larger than 16 KiB.  fetch_k 2
    and 8 stage the rows in LDS, 17 re-reads them"""
    c = corpus(d, 3, 200, metric, seed=431 + d, empty=0)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 3, seed=432)
    assert shapes_in_lds(2, d) and shapes_in_lds(8, d) and not shapes_in_lds(17, d)
    pids = np.array([[2, 0], [1, 2], [2, -1]], np.int64)     # (the pids form: a search with a parent may take the one-launch kernel)
    ctx.scan(s, q, pids, 17, metric)
    assert ctx.last_scan_kernel().startswith("k_scan_wide"), "the candidate search of these rows is the wide-row scan"
    for C_ in (2, 8, 17):
        prep = DY.prepare(q, None, c["vecs"], c["ids"], c["offsets"], None, C_, metric, pids=pids)
        for k, lam in ((1, 0.5), (2, 0.3), (C_, 0.5), (C_, 0.0)):
            _eq(ctx.diverse_scan(s, q, pids, k, C_, lam, metric), DY.expected_batch(prep, k, lam, metric), (metric, d, C_, k, lam))
            assert ctx.last_scan_kernel().startswith("k_scan_wide")
        want = DY.case(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 2, C_, C_, 0.3, metric)
        _eq(ctx.diverse_search(parent, s, q, 2, C_, C_, 0.3, metric), want, ("with parent", metric, d, C_))
    s.close()
    parent.close()


# ---- 4. the lists: parent, no parent, pids; the squared domain ------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_list_forms(ctx, corpora, metric):
    e = corpora(metric)
    c, s, parent, q = e["c"], e["s"], e["parent"], e["q"]
    for C_, k, lam in ((64, 10, 0.3), (17, 17, 0.5)):
        # every list (parent == NULL)
        want = DY.expected_batch(_prep(e, C_, nprobe=None), k, lam, metric)
        _eq(ctx.diverse_search(None, s, q, 1, k, C_, lam, metric), want, ("flat", metric, C_))
        # nprobe 1 and more lists than there are
        for nprobe in (1, 50):
            want = DY.expected_batch(_prep(e, C_, nprobe=nprobe), k, lam, metric)
            _eq(ctx.diverse_search(parent, s, q, nprobe, k, C_, lam, metric), want, ("nprobe", nprobe, metric, C_))
        # pids with -1, empty lists (0, 1), the short lists (2, 3) and rows of -1 only
        sizes = np.diff(c["offsets"])
        assert sizes[0] == 0 and sizes[1] == 0 and sizes[2] == 5 and sizes[3] == 7
        pids = RY.probed(q, c["cent"], c["offsets"], 4, metric).copy()
        pids[:, 1] = -1
        pids[1] = [0, 1, -1, -1]     # nothing but empty lists: no candidate
        pids[2] = [-1, -1, -1, -1]
        pids[3] = [2, -1, 1, 3]      # 12 candidates: fewer than fetch_k
        want = DY.expected_batch(_prep(e, C_, nprobe=None, pids=pids), k, lam, metric)
        assert (want[0][1] == -1).all() and (want[0][2] == -1).all() and (want[0][3] >= 0).sum() == min(k, 12)
        _eq(ctx.diverse_scan(s, q, pids, k, C_, lam, metric), want, ("pids", metric, C_))
        _eq(ctx.diverse_scan(s, torch.from_numpy(q).cuda(), torch.from_numpy(pids).cuda(), k, C_, lam, metric), want, ("pids, device", metric, C_))
        one = np.array([4, 2, -1], np.int64)     # one row of lists for every query
        want = DY.expected_batch(_prep(e, C_, nprobe=None, pids=np.ascontiguousarray(np.broadcast_to(one, (17, 3)))), k, lam, metric)
        _eq(ctx.diverse_scan(s, q, one, k, C_, lam, metric), want, ("pids, one row", metric, C_))


def test_squared_l2(ctx, corpora):
    e = corpora("l2")
    s, parent, q = e["s"], e["parent"], e["q"]
    differs = 0
    for C_, k, lam in ((64, 10, 0.3), (17, 17, 0.5), (65, 2, 0.0), (64, 5, 1.0)):
        want_sqrt = DY.expected_batch(_prep(e, C_), k, lam, "l2")
        want_sq = DY.expected_batch(_prep(e, C_, squared=True), k, lam, "l2")
        differs += int((want_sq[2] != want_sqrt[2]).any())
        ctx.set_squared_l2(True)
        try:
            _eq(ctx.diverse_search(parent, s, q, 3, k, C_, lam, "l2"), want_sq, ("squared", C_, k, lam))
        finally:
            ctx.set_squared_l2(False)
        _eq(ctx.diverse_search(parent, s, q, 3, k, C_, lam, "l2"), want_sqrt, ("sqrt again", C_, k, lam))
    assert differs > 0, "the selection depends on the domain the costs are computed in"


# ---- 5. filters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filters(ctx, corpora, metric):
    from quake_amd.capi import Attr, Filter
    e = corpora(metric)
    c, s, parent, q = e["c"], e["s"], e["parent"], e["q"]
    ids = c["ids"]
    rng = np.random.default_rng(441)
    C_, k = 64, 10
    S = FY.draw_set(ids, 0.3, rng)
    pids = RY.probed(q, c["cent"], c["offsets"], 3, metric)
    a = Attr(s)
    a.set(ids, ids % 11)
    allowed_where = ids[(ids % 11 >= 2) & (ids % 11 <= 4)]
    for tag, flt, kw in (("allow", Filter(s, S, "allow"), dict(S=S, mode="allow")),
                         ("deny", Filter(s, S, "deny"), dict(S=S, mode="deny")),
                         ("where", Filter.where(s, [(a, "range", 2, 4)]), dict(S=allowed_where, mode="allow"))):
        for lam in (0.0, 0.5, 1.0):
            want = DY.expected_batch(_prep(e, C_, **kw), k, lam, metric)
            assert (want[0] >= 0).all()
            _eq(ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric, filter=flt), want, (tag, metric, lam))
            wantp = DY.expected_batch(_prep(e, C_, nprobe=None, pids=pids, **kw), k, lam, metric)
            _eq(ctx.diverse_scan(s, q, pids, k, C_, lam, metric, filter=flt), wantp, (tag, "scan", metric, lam))
            _eq(wantp, want, "the pids of the coarse step give the search")
        flt.close()
    # filters that leave no candidate, fewer than k, and between k and fetch_k in the probed lists of query 0
    p0 = DY.prepare(q[:1], c["cent"], c["vecs"], ids, c["offsets"], 3, 256, metric)[0][0]
    assert p0.shape[0] == 256
    for tag, S2, n_want in (("none", np.array([10 ** 9], np.int64), 0), ("fewer than k", p0[5:9], 4), ("between k and C", p0[3:40], 37)):
        flt = Filter(s, S2, "allow")
        # (a filter without candidates: nothing for the oracle to search)
        prep = _prep(e, C_, S=S2, mode="allow") if n_want else [(np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros((0, 0), np.float32))] * 17
        assert prep[0][0].shape[0] == n_want
        for lam in (0.3, 1.0):
            want = DY.expected_batch(prep, k, lam, metric)
            assert (want[0][0] >= 0).sum() == min(k, n_want) and (want[2][0][min(k, n_want):] == -1).all()
            _eq(ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric, filter=flt), want, (tag, metric, lam))
        flt.close()
    a.close()


# ---- 6. memory, NULL outputs, determinism, timing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_memory_null_outputs_and_determinism(ctx, corpora, metric):
    from quake_amd.capi import metric_code
    e = corpora(metric)
    s, parent, q = e["s"], e["parent"], e["q"]
    C_, k, lam = 65, 10, 0.3
    want = DY.expected_batch(_prep(e, C_), k, lam, metric)
    host = ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric)
    _eq(host, want, "host")
    assert host[2].dtype == np.int32
    dev = ctx.diverse_search(parent, s, torch.from_numpy(q).cuda(), 3, k, C_, lam, metric)
    assert all(t.is_cuda for t in dev) and dev[2].dtype == torch.int32
    _eq(dev, want, "device")
    again = ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric)
    for x, y in zip(host, again):
        assert x.tobytes() == y.tobytes()
    for wd, wr in ((False, True), (True, False), (False, False)):
        for xq in (q, torch.from_numpy(q).cuda()):
            got = ctx.diverse_search(parent, s, xq, 3, k, C_, lam, metric, want_dist=wd, want_rank=wr)
            assert (got[1] is None) == (not wd) and (got[2] is None) == (not wr)
            for name, g, w in zip(NAMES, got, host):
                if g is not None:
                    assert _np(g).tobytes() == w.tobytes(), (name, wd, wr)
    # NULL outputs leave the caller's buffers alone (raw call, both memories)
    P = lambda b: C.c_void_p(b.ctypes.data) if isinstance(b, np.ndarray) else C.c_void_p(b.data_ptr())  # noqa: E731
    for mem, xq in ((0, q), (1, torch.from_numpy(q).cuda())):
        if mem == 0:
            bufs = [np.full(h.shape, -7, h.dtype) for h in host]
        else:
            bufs = [torch.full(tuple(h.shape), -7, dtype={np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32,
                                                           np.dtype(np.int32): torch.int32}[h.dtype], device="cuda") for h in host]
        st = ctx.lib.qk_diverse_search(ctx.h, parent.h, s.h, P(xq), 17, 3, k, C_, C.c_float(lam), metric_code(metric), None, P(bufs[0]),
                                       None, None, mem, None)
        assert st == 0
        assert _np(bufs[0]).tobytes() == host[0].tobytes() and (_np(bufs[1]) == -7).all() and (_np(bufs[2]) == -7).all()
    # timing: the candidate search's figures; the tail is part of the total only
    ctx.set_timing(1)
    try:
        got = ctx.diverse_search(parent, s, q, 3, k, C_, lam, metric, timing=True)
        assert ctx.last_scan_kernel() != ""
        plain = ctx.search(parent, s, q, 3, C_, metric, timing=True)
        # fetch_k 17 of 17 queries: the candidate search is the one-launch kernel, which leaves no scalars behind
        small = ctx.diverse_search(parent, s, q, 3, 5, 17, lam, metric, timing=True)
        small_kernel = ctx.last_scan_kernel()
        small_plain = ctx.search(parent, s, q, 3, 17, metric, timing=True)
    finally:
        ctx.set_timing(0)
    _eq(got, want, "with timing")
    tm, tp = got[3], plain[2]
    assert tm["partitions_scanned"] == tp["partitions_scanned"] > 0 and tm["scan_bytes"] == tp["scan_bytes"]
    assert tm["scan_ms"] > 0 and tm["total_ms"] > tm["scan_ms"]
    _eq(small, DY.expected_batch(_prep(e, 17), 5, lam, metric), "with timing, small batch")
    assert small_kernel == "k_search_small" and small[3]["partitions_scanned"] == small_plain[2]["partitions_scanned"] == 17 * 3
    assert small[3]["scan_ms"] > 0 and small[3]["total_ms"] > small[3]["scan_ms"]


# ---- 7. lambda = 1 and fetch_k == k against the device's own search ---------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_against_the_search_itself(ctx, corpora, metric):
    from quake_amd.capi import Filter
    e = corpora(metric)
    s, parent, q = e["s"], e["parent"], e["q"]
    flt = Filter(s, e["c"]["ids"][::3], "allow")
    for f in (None, flt):
        for C_ in (17, 256):
            si, sd = ctx.search(parent, s, q, 3, C_, metric, filter=f)
            for k in (1, 10, C_):
                gi, gd, gr = ctx.diverse_search(parent, s, q, 3, k, C_, 1.0, metric, filter=f)
                np.testing.assert_array_equal(gi, si[:, :k])
                np.testing.assert_array_equal(gd.view(np.uint32), sd[:, :k].view(np.uint32))
                np.testing.assert_array_equal(gr, np.where(si[:, :k] >= 0, np.arange(k, dtype=np.int32)[None, :], -1))
            n = (si >= 0).sum(axis=1)       # (the filter leaves some queries fewer than 256 candidates: padding follows them)
            assert (n > 0).all() and (f is not None or (n == C_).any())
            for lam in (0.0, 0.5):
                gi, gd, gr = ctx.diverse_search(parent, s, q, 3, C_, C_, lam, metric, filter=f)
                for qi in range(17):
                    assert sorted(gr[qi, :n[qi]].tolist()) == list(range(n[qi])) and gr[qi, 0] == 0 and (gr[qi, n[qi]:] == -1).all()
                at = np.where(gr >= 0, gr, C_ - 1).astype(np.int64)      # (a padded entry of the search row stands for padding)
                assert (si[np.arange(17), C_ - 1] == -1)[n < C_].all()
                np.testing.assert_array_equal(gi, np.take_along_axis(si, at, axis=1))
                np.testing.assert_array_equal(gd.view(np.uint32), np.take_along_axis(sd, at, axis=1).view(np.uint32))
    flt.close()


# ---- 8. liveness: the rows move under add / remove ---------------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = corpus(32, 12, 2500, "l2", seed=451)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(452)
    q = RY.queries(c, 17, seed=453)
    pids = RY.probed(q, c["cent"], c["offsets"], 4, "l2")

    def check(tag):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(12)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        out = None
        for C_, k, lam in ((64, 10, 0.3), (17, 17, 0.0)):
            want = DY.case(q, None, vecs, ids, offs, None, k, C_, lam, "l2", pids=pids)
            _eq(ctx.diverse_scan(s, q, pids, k, C_, lam, "l2"), want, (tag, C_, k))
            out = out or want
        return out

    w0 = check("as built")
    s.remove_ids(np.unique(np.concatenate([c["ids"][::5], w0[0][:, 1]])))     # every query loses its second pick, lists get holes
    w1 = check("remove")
    assert not np.isin(w1[0], w0[0][:, 1]).any() and (w1[0] != w0[0]).any()
    na = 600
    new_ids = np.arange(10 ** 6, 10 ** 6 + na, dtype=np.int64)
    lists = rng.integers(4, 12, size=na).astype(np.int64)
    new_vecs = (c["cent"][lists] + 0.3 * rng.standard_normal((na, 32))).astype(np.float32)
    lists[:17] = pids[:, 0]
    new_vecs[:17] = q + np.float32(1e-3)         # a new nearest row for every query; the lists outgrow their extents and move
    lists[17:34] = pids[:, 0]
    new_vecs[17:34] = new_vecs[:17]              # ... and an exact copy of it
    s.add_batch(new_ids, new_vecs, lists)
    w2 = check("add")
    assert (w2[0][:, 0] == new_ids[:17]).all() and (w2[0] >= 10 ** 6).sum() > 17
    s.close()
    parent.close()


# ---- 9. limits and errors at the C level ---------------------------------------------------------------------------------------------
def test_limits(ctx, corpora):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter, Store
    e, e2 = corpora("l2"), corpora("ip")
    s, parent, q = e["s"], e["parent"], e["q"][:5]
    pids = RY.probed(q, e["c"]["cent"], e["c"]["offsets"], 3, "l2")
    plain = ctx.diverse_search(parent, s, q, 3, 10, 64, 0.5, "l2")
    for k, C_, lam, match in ((0, 10, 0.5, "QK_ERR_INVALID.*k=0"), (-3, 10, 0.5, "QK_ERR_INVALID.*k=-3"),
                              (11, 10, 0.5, "QK_ERR_INVALID.*fetch_k=10 must be at least k=11"),
                              (10, 257, 0.5, "QK_ERR_UNSUPPORTED.*fetch_k=257 exceeds QK_MAX_FETCH_K=256"),
                              (300, 300, 0.5, "QK_ERR_UNSUPPORTED.*fetch_k=300"),
                              (5, 10, float("nan"), "QK_ERR_INVALID.*lambda"), (5, 10, -0.01, "QK_ERR_INVALID.*lambda"),
                              (5, 10, 1.5, "QK_ERR_INVALID.*lambda"), (5, 10, float("inf"), "QK_ERR_INVALID.*lambda")):
        with pytest.raises(QuakeHipError, match=match):
            ctx.diverse_search(parent, s, q, 3, k, C_, lam, "l2")
        with pytest.raises(QuakeHipError, match=match):
            ctx.diverse_scan(s, q, pids, k, C_, lam, "l2")
    f2 = Filter(e2["s"], e2["c"]["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID"):
        ctx.diverse_search(parent, s, q, 3, 5, 10, 0.5, "l2", filter=f2)
    f2.close()
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*nprobe"):
        ctx.diverse_search(parent, s, q, 0, 5, 10, 0.5, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*partition id list"):
        ctx.diverse_scan(s, q, np.zeros((5, 0), np.int64), 5, 10, 0.5, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_NOT_FOUND.*List does not exist"):
        ctx.diverse_scan(s, q, np.full((5, 1), 99, np.int64), 5, 10, 0.5, "l2")
    # Q == 0 is served
    empty = ctx.diverse_search(parent, s, q[:0], 3, 5, 10, 0.5, "l2")
    assert empty[0].shape == (0, 5) and empty[2].shape == (0, 5)
    # no lists probed: a store without lists -- all padding
    bare = Store(ctx, 33)
    for metric, pad in (("l2", np.inf), ("ip", -np.inf)):
        got = ctx.diverse_search(None, bare, q, 1, 4, 9, 0.5, metric)
        assert (got[0] == -1).all() and (got[1] == pad).all() and (got[2] == -1).all()
    bare.close()
    # the context still answers, and answers the same
    _eq(ctx.diverse_search(parent, s, q, 3, 10, 64, 0.5, "l2"), plain, "after the refusals")
    _eq(ctx.diverse_scan(s, q, pids, 10, 64, 0.5, "l2"), plain, "scan")


# ---- 10. the mirrors ---------------------------------------------------------------------------------------------------------------------
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
    return (r.ids, r.distances, r.ranks)


def _yardstick_of(idx, q, nprobe, k, C_, lam, metric, S=None, mode="allow"):
    """the yardstick over the lists the index holds now: its store read back list by list, the probed lists from the coarse step"""
    st = idx._store
    nl = max(st.list_ids()) + 1
    d = q.shape[1]
    have = set(st.list_ids())
    lists = [st.get_list(p) if p in have else (np.zeros((0, d), np.float32), np.zeros(0, np.int64)) for p in range(nl)]
    vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    pids = (idx._ctx.coarse(idx.parent._store, q, nprobe, metric, values=False)[0] if idx.parent is not None
            else np.ascontiguousarray(np.broadcast_to(np.arange(nl, dtype=np.int64), (q.shape[0], nl))))
    return DY.case(q, None, vecs, ids, offs, None, k, C_, lam, metric, S=S, mode=mode, pids=pids)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(qb, metric, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(461)
    n, d = 3000, 32
    x = torch.randn(n, d, generator=g)
    x[n // 2:] = x[:n // 2] + 0.0       # every vector twice: exact copies under other ids
    ids = torch.randperm(n, generator=g) + 11
    q = x[torch.randint(0, n, (17,), generator=g)] + 0.05 * torch.randn(17, d, generator=g)
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(462)))
    idx = _build(quake, x, ids, 12, metric)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    qn = q.numpy()

    def compare(tag, ks=((3, 20), (10, 64), (17, 17))):
        reordered = 0
        for k, C_ in ks:
            sp, spc = quake.SearchParams(), qb.SearchParams()
            for p in (sp, spc):
                p.nprobe, p.k = 4, k
            for exclude in (None, True):
                sp.filter = None if exclude is None else idx.make_filter(S, exclude)
                spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
                for lam in (0.0, 0.3, 1.0):
                    want = _yardstick_of(idx, qn, 4, k, C_, np.float32(lam), metric, S=None if exclude is None else S.numpy(), mode="deny")
                    reordered += int((want[2] != np.arange(k)[None, :]).any())
                    t = (tag, metric, k, C_, exclude, lam)
                    r = idx.diverse_search(q, sp, C_, lam)
                    _eq(_res(r), want, ("python",) + t)
                    assert r.timing_info.n_queries == 17 and tuple(r.ids.shape) == (17, k) and r.ranks.dtype == torch.int32
                    rd = idx.diverse_search(q.cuda(), sp, fetch_k=C_, lambda_mult=lam)
                    assert all(o.is_cuda for o in _res(rd))
                    _eq(_res(rd), want, ("python, device",) + t)
                    for xq in (q, q.cuda()):
                        rc = loaded.diverse_search(xq, spc, C_, lam)
                        assert rc.ids.is_cuda == xq.is_cuda and rc.ranks.is_cuda == xq.is_cuda and rc.ranks.dtype == torch.int32
                        _eq(_res(rc), want, ("compiled", xq.is_cuda) + t)
            sp.filter = spc.filter = None
        assert reordered > 0
        return sp, spc

    sp, spc = compare("as built")
    # the default lambda_mult is 0.5 in both
    a, b = idx.diverse_search(q, sp, 17), loaded.diverse_search(q, spc, 17)
    _eq(_res(a), _res(idx.diverse_search(q, sp, 17, 0.5)), "default")
    _eq(_res(b), _res(a), "default, compiled")
    for m, p in ((idx, sp), (loaded, spc)):
        empty = m.diverse_search(q[:0], p, 17)
        assert tuple(empty.ids.shape) == (0, 17) and tuple(empty.ranks.shape) == (0, 17) and empty.ranks.dtype == torch.int32
    # the rows move: remove, add, maintenance -- the same changes in both mirrors
    gone = ids[::4]
    new_x = q.repeat(6, 1) + 0.01 * torch.randn(102, d, generator=g)
    new_ids = torch.arange(10 ** 6, 10 ** 6 + 102)
    for m in (idx, loaded):
        m.remove(gone)
        m.add(new_x, new_ids)
    compare("after remove and add", ks=((10, 64),))
    for m in (idx, loaded):
        m.maintenance()
    got = idx.diverse_search(q, sp, 64, 0.3)
    assert (got.ids >= 10 ** 6).any()
    _eq(_res(got), _yardstick_of(idx, qn, 4, 17, 64, np.float32(0.3), metric), "python, after maintenance")
    gotc = loaded.diverse_search(q, spc, 64, 0.3)
    _eq(_res(gotc), _yardstick_of_compiled(loaded, gotc, q, spc, metric), "compiled, after maintenance")


def _yardstick_of_compiled(loaded, got, q, spc, metric):
    """the compiled mirror keeps its store to itself: after its own maintenance its lists need not be the Python mirror's, so its
    answer is checked against the consequences of the definition on its own search -- ranks index the search(k = 64) row"""
    spc64 = type(spc)()
    spc64.nprobe, spc64.k = spc.nprobe, 64
    base = loaded.search(q, spc64)
    rk = got.ranks.to(torch.int64)
    assert (rk[:, 0] == 0).all() and (rk >= 0).all() and all(len(set(r.tolist())) == rk.shape[1] for r in rk)
    return torch.gather(base.ids, 1, rk), torch.gather(base.distances, 1, rk), got.ranks


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(471)
    x = torch.randn(3000, 16, generator=g)
    ids = torch.arange(3000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 12)
        other = _build(mod, x, ids, 12)

        def params(**kw):
            sp = mod.SearchParams()
            sp.k, sp.nprobe = 5, 4
            for k, v in kw.items():
                setattr(sp, k, v)
            return sp

        plain = idx.diverse_search(qq, params(), 20)
        assert (plain.ids >= 0).all()
        for kw, match in ((dict(recall_target=0.9), "recall_target"),
                          (dict(filters=[idx.make_filter(ids[:1000])], query_filter=torch.zeros(10, dtype=torch.int32)), "query_filter"),
                          (dict(max_nprobe=8), "max_nprobe"),
                          (dict(filter_exact_rows=100, filter=idx.make_filter(ids[:50])), "filter_exact_rows"),
                          (dict(filters_exact_rows=100), "filters_exact_rows"),
                          (dict(filter=other.make_filter(ids[:1000])), "another index"),
                          (dict(k=0), "k=0 must be at least 1"),
                          (dict(k=21), "fetch_k=20 must be at least k=21")):
            with pytest.raises(RuntimeError, match=match):
                idx.diverse_search(qq, params(**kw), 20)
        with pytest.raises(RuntimeError, match="fetch_k=257 must not exceed 256"):
            idx.diverse_search(qq, params(), 257)
        for lam, match in ((float("nan"), "lambda_mult is NaN"), (-0.5, r"lambda_mult=-0.5 must lie in \[0, 1\]"), (1.25, "lambda_mult=1.25")):
            with pytest.raises(RuntimeError, match=match):
                idx.diverse_search(qq, params(), 20, lam)
        # a call with two faults raises the same error in both mirrors: refusals, k, fetch_k, lambda, filter
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.diverse_search(qq, params(recall_target=0.9, k=0), 500, 7.0)
        with pytest.raises(RuntimeError, match="k=0"):
            idx.diverse_search(qq, params(k=0), 500, 7.0)
        with pytest.raises(RuntimeError, match="fetch_k=500"):
            idx.diverse_search(qq, params(filter=other.make_filter(ids[:1000])), 500, 7.0)
        with pytest.raises(RuntimeError, match="lambda_mult=7"):
            idx.diverse_search(qq, params(filter=other.make_filter(ids[:1000])), 20, 7.0)
        grp = _build(mod, x, ids, 12, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.diverse_search(qq, params(), 20)
        again = idx.diverse_search(qq, params(), 20)
        for a, b in zip(_res(again), _res(plain)):
            assert torch.equal(a, b)
    from quake_amd.sharded import ShardedIndex
    with pytest.raises(RuntimeError, match="not supported by sharded.py"):
        ShardedIndex(None).diverse_search(qq, 4, 5, 20)
