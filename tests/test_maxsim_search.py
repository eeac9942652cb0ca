"""Multi-vector search (qk_maxsim_search / qk_maxsim_scan; Context.maxsim_search / maxsim_scan; QuakeIndex.multi_vector_search in
both mirrors): per logical query of T sub-queries, the k best values of an attribute column by the sum over the sub-queries of the
best range hit among the value's rows.

Every comparison is exact equality of groups, score bits, matched, n_groups and hits with tests/maxsim_yardstick.py (pinned on the
CPU by tests/test_maxsim_oracle.py); a NaN score counts as the canonical quiet NaN the header documents.  The yardstick is evaluated
once per situation with k = 1024 and cut to the smaller k's: the k best of a total order are a prefix of its 1024 best.  No
assertion reads a clock.  Every test asserts on its own inputs that the situation it is about occurs."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_yardstick as FY
import grouped_yardstick as GY
import maxsim_yardstick as MY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
KS = (1, 10, 1024)
COLS = ("own", "forty", "one", "half", "ext")
NTOK = {1: [1, 0, 1, 1, 1], 3: [3, 0, 2, 1, 3], 64: [64, 0, 17, 1, 40]}
L = 5
MISSING = {"ip": 0.0, "l2": 9.5}


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    MY.assert_equal([_np(g) for g in got[:5]], want, str(tag))


def _cut(want, k):
    return tuple(w[:, :k] for w in want[:3]) + tuple(want[3:])


def _attr(s, ids, vals):
    from quake_amd.capi import Attr
    a = Attr(s)
    a.set(np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(vals, np.int64))
    return a


def _corpus(metric, seed):
    """d = 32, 6000 rows in 12 lists: list 0 holds 2500 rows (it crosses the 1024-key slice), list 1 is empty, the rest share the
    others in odd sizes; ids are a permutation"""
    rng = np.random.default_rng(seed)
    d, nlist, n = 32, 12, 6000
    w = rng.random(10) + 0.3
    sizes = np.concatenate([[2500, 0], np.floor(w / w.sum() * 3500).astype(np.int64)])
    sizes[2] += n - sizes.sum()
    assign = np.repeat(np.arange(nlist), sizes)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    ids = rng.permutation(n).astype(np.int64)
    return dict(cent=cent, vecs=np.ascontiguousarray(x), ids=ids, offsets=offsets, d=d, metric=metric, x=x)


def _columns(ids):
    """(ids, values) of the five columns: every id its own group, 40 scattered groups (-1 among them), one group, a column that
    gives only half the ids a value, the extreme values"""
    half = ids[ids % 2 == 0]
    return dict(own=(ids, ids.copy()), forty=(ids, ids % 40 - 20), one=(ids, np.full(ids.shape[0], 7, np.int64)),
                half=(half, half % 13 - 1), ext=(ids, np.where(ids % 3 == 0, I64MIN, np.where(ids % 3 == 1, I64MAX, -1))))


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    from quake_amd.capi import Filter, Store
    cache = {}

    def get(metric):
        if metric not in cache:
            c = _corpus(metric, 401 if metric == "l2" else 402)
            sizes = np.diff(c["offsets"])
            assert sizes[0] == 2500 and sizes[1] == 0 and sizes.sum() == 6000 and np.array_equal(np.sort(c["ids"]), np.arange(6000))
            s = Store(ctx, 32)
            s.build_csr(c["offsets"], c["ids"], c["vecs"])
            parent = Store(ctx, 32)
            parent.build_csr(np.array([0, 12], np.int64), np.arange(12, dtype=np.int64), c["cent"])
            cols = _columns(c["ids"])
            assert -1 in cols["forty"][1] and cols["half"][0].shape[0] == 3000
            S = FY.draw_set(c["ids"], 0.4, np.random.default_rng(403))
            cache[metric] = dict(c=c, s=s, parent=parent, cols=cols, attrs={k: _attr(s, *v) for k, v in cols.items()}, S=S,
                                 flt=Filter(s, S, "deny"), memo={})
        return cache[metric]

    yield get
    for e in cache.values():
        for a in e["attrs"].values():
            a.close()
        e["flt"].close()
        e["s"].close()
        e["parent"].close()


def _queries(e, T):
    key = ("q", T)
    if key not in e["memo"]:
        c = e["c"]
        rng = np.random.default_rng(410 + T)
        q = (c["x"][rng.integers(0, 6000, size=L * T)] + 0.05 * rng.standard_normal((L * T, 32))).astype(np.float32)
        if c["metric"] == "ip":
            q /= np.linalg.norm(q, axis=1, keepdims=True)
        pids = np.tile(np.arange(12, dtype=np.int64), (L * T, 1))
        pids[rng.random(pids.shape) < 0.2] = -1
        pids[0, 0] = 0   # (the list of 2500 rows is probed)
        e["memo"][key] = (np.ascontiguousarray(q.reshape(L, T, 32)), pids)
    return e["memo"][key]


def _cand(e, T, entry, filtered):
    """(grouped_yardstick.candidates, row values source ids, pids of the call), once per situation"""
    key = ("cand", T, entry, filtered)
    if key not in e["memo"]:
        c = e["c"]
        q3, pids = _queries(e, T)
        vecs, ids, offsets = c["vecs"], c["ids"], c["offsets"]
        if filtered:
            vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, FY.allowed_rows(ids, e["S"], "deny"))
        if entry == "search":
            pids = GY.probed(q3.reshape(L * T, 32), c["cent"], c["offsets"], 3, c["metric"])
        e["memo"][key] = (GY.candidates(q3.reshape(L * T, 32), vecs, ids, offsets, pids, c["metric"]), ids)
    return e["memo"][key]


def _radii(e, T):
    """(tag, radius): none (every probed row), one that keeps a few percent of the unfiltered search's pairs, one that passes nothing"""
    metric = e["c"]["metric"]
    (_, _, val), _ = _cand(e, T, "search", False)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(val) if metric == "l2" else val
    few = float(np.quantile(dist, 0.03 if metric == "l2" else 0.97))
    return [("none", None), ("few", few), ("nothing", -1.0 if metric == "l2" else 1e30)]


# ---- 1. the grid: metric, T, column x entry point, radius, filter, ragged tokens, k, host and device memory ---------------------------
@pytest.mark.parametrize("col", COLS)
@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_grid(ctx, corpora, metric, T, col):
    e = corpora(metric)
    s, parent, a = e["s"], e["parent"], e["attrs"][col]
    q3, pids = _queries(e, T)
    inf = float("inf") if metric == "l2" else float("-inf")
    seen = set()
    for entry in ("search", "scan"):
        for filtered in (False, True):
            cand, ids = _cand(e, T, entry, filtered)
            rowval, rowhas = GY.row_values(ids, *e["cols"][col])
            flt = e["flt"] if filtered else None
            # ragged tokens (0 and T among them) at every radius, with the filter on and off; at the radius that keeps a few percent
            # also every sub-query taking part
            for tag, radius, nt in [(t_, r_, n_) for t_, r_ in _radii(e, T) for n_ in ((NTOK[T], None) if t_ == "few" else (NTOK[T],))]:
                want = MY.reduce(cand, T, rowval, rowhas, 1024, metric, radius, nt, MISSING[metric])
                r = inf if radius is None else radius
                for k in KS:
                    for dev in (False, True):
                        x = torch.from_numpy(q3).cuda() if dev else q3
                        t = (metric, T, col, entry, filtered, tag, k, dev)
                        if entry == "search":
                            got = ctx.maxsim_search(parent, s, x, 3, r, metric, a, k, MISSING[metric], nt, flt)
                            assert ctx.last_scan_kernel() == "k_scan (maxsim)"
                        else:
                            got = ctx.maxsim_scan(s, x, torch.from_numpy(pids).cuda() if dev else pids, r, metric, a, k, MISSING[metric], nt, flt)
                        assert all(torch.is_tensor(g) and g.is_cuda for g in got) if dev else all(isinstance(g, np.ndarray) for g in got)
                        _eq(got, _cut(want, k), t)
                groups, scores, matched, n_groups, hits = want
                if tag == "nothing":
                    assert hits.sum() == 0 and n_groups.sum() == 0 and (groups == 0).all()
                else:
                    assert hits.sum() > 0 and n_groups.max() > 0
                    if nt is not None:
                        assert n_groups[1] == 0 and (hits[1] == 0).all()
                    if n_groups.max() < 1024:
                        seen.add("k exceeds the groups")
                    if n_groups.max() > 1024:
                        seen.add("more groups than the selection sorts")
                    if T > 1 and (matched[groups != 0] < (T if nt is None else np.array(nt).max())).any():
                        seen.add("a term is missing")
                    if hits.max() > 1024:
                        seen.add("a sub-query crosses a slice")
    assert "k exceeds the groups" in seen or col == "own"
    if col == "own":
        assert "more groups than the selection sorts" in seen
    if T > 1 and col in ("own", "half"):
        assert "a term is missing" in seen
    assert "a sub-query crosses a slice" in seen


# ---- 2. planted arithmetic: integer-valued vectors, inner product, every product exact -------------------------------------------------
def test_planted_arithmetic(ctx):
    from quake_amd.capi import Store
    d = 8
    big = np.float32(2.0 ** 26)
    rows = np.zeros((9, d), np.float32)
    rows[0, :3] = (big, 1, -big)      # value 1: the terms 2^26, 1, -2^26 -- only the sequential sum gives 0
    rows[1, :3] = (3, 2, 1)           # value 40 and ...
    rows[2, :3] = (1, 2, 3)           # ... value -40: both score 6
    rows[3, 0] = np.inf               # value 8: -inf under the first sub-query, NaN (no hit) under the others
    rows[4, :3] = (-5, -5, -5)        # value 9: every term negative
    rows[5, 3] = 1                    # value 10: every product 0
    rows[6, :3] = (3, 2, 1)           # no value
    rows[7, :3] = (0, 7, 0)           # value 11, with row 8
    rows[8, :3] = (7, 0, 0)
    ids = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108], np.int64)
    offsets = np.array([0, 4, 4, 9], np.int64)
    col_ids = np.array([100, 101, 102, 103, 104, 105, 107, 108], np.int64)
    col_vals = np.array([1, 40, -40, 8, 9, 10, 11, 11], np.int64)
    q3 = np.zeros((2, 3, d), np.float32)
    q3[0, 0, 0], q3[0, 1, 1], q3[0, 2, 2] = 1, 1, 1
    q3[1, 0, 0], q3[1, 1, 1], q3[1, 2, 2] = -1, 1, 1    # the first sub-query of the second logical query reads -inf off row 3
    s = Store(ctx, d)
    s.build_csr(offsets, ids, rows)
    a = _attr(s, col_ids, col_vals)
    pids = np.array([0, 1, 2], np.int64)
    ninf = float("-inf")
    try:
        for missing in (0.0, float("inf"), ninf, -3.0):
            for radius in (ninf, 0.5):
                want = MY.scan(q3, rows, ids, offsets, pids, 16, "ip", col_ids, col_vals, radius=radius, missing=missing)
                got = ctx.maxsim_scan(s, q3, pids, radius, "ip", a, 16, missing)
                _eq(got, want, ("planted", missing, radius))
                _eq(ctx.maxsim_search(None, s, torch.from_numpy(q3).cuda(), 1, radius, "ip", a, 16, missing), want, ("planted, device", missing))
                g, sc, m, n, h = want
                if missing == 0.0 and radius == ninf:
                    at = {int(v): j for j, v in enumerate(g[0][:n[0]])}
                    assert sc[0][at[1]] == 0.0 and sc[0][at[40]] == 6.0 == sc[0][at[-40]] and at[-40] + 1 == at[40]   # the tie: -40 first
                    assert sc[0][at[11]] == 14.0 and n[0] == 7 and h[0].tolist() == [9, 8, 8]   # (0 * inf: a NaN product is no hit)
                    assert np.isposinf(sc[0][at[8]]) and at[8] == 0                            # +inf + 0 + 0
                    assert np.isneginf(sc[1][list(g[1][:n[1]]).index(8)])                      # -inf + 0 + 0
                if missing == float("inf") and radius == ninf:
                    j = list(g[1][:n[1]]).index(8)
                    assert np.isnan(sc[1][j]) and j == n[1] - 1 and m[1][j] == 1    # -inf + inf: the NaN score comes last
                if missing == float("inf") and radius == 0.5:
                    assert np.isposinf(sc[0][:n[0]]).any()                             # a missing term alone: +inf
                if missing == ninf and radius == 0.5:
                    assert np.isneginf(sc[0][:n[0]]).any()
        # any order but the sequential one changes the bits: the same three sub-queries, the second and third exchanged
        want = MY.scan(q3[:1, [0, 2, 1]], rows, ids, offsets, pids, 16, "ip", col_ids, col_vals)
        assert want[1][0][list(want[0][0]).index(1)] == 1.0
        _eq(ctx.maxsim_scan(s, q3[:1, [0, 2, 1]], pids, ninf, "ip", a, 16, 0.0), want, "exchanged")
    finally:
        a.close()
        s.close()


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_identities(ctx, corpora, metric):
    e = corpora(metric)
    s, parent, c = e["s"], e["parent"], e["c"]
    inf = float("inf") if metric == "l2" else float("-inf")
    # T = 1, every id its own group, no radius: grouped search's groups and distances
    q1, p1 = _queries(e, 1)
    k = 50
    gi, gd, gg = ctx.scan_grouped(s, q1[:, 0], p1, k, metric, e["attrs"]["own"])
    assert all(np.unique(gd[i]).shape[0] == k for i in range(L)), "the scores must not tie"
    got = ctx.maxsim_scan(s, q1, p1, inf, metric, e["attrs"]["own"], k, MISSING[metric])
    assert np.array_equal(got[0], gg) and np.array_equal(got[0], gi) and (got[2] == 1).all()
    assert np.array_equal(got[1].view(np.uint32), (gd + np.float32(0.0)).astype(np.float32).view(np.uint32))
    # row l equals the call of l alone; a call run twice; the logical queries reversed
    q3, p3 = _queries(e, 3)
    radius = _radii(e, 3)[1][1]
    nt = np.array(NTOK[3], np.int32)
    for col in ("forty", "half"):
        a = e["attrs"][col]
        full = ctx.maxsim_scan(s, q3, p3, radius, metric, a, 10, MISSING[metric], nt, e["flt"])
        assert full[4].sum() > 0
        again = ctx.maxsim_scan(s, q3, p3, radius, metric, a, 10, MISSING[metric], nt, e["flt"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(full, again))
        for l in range(L):
            one = ctx.maxsim_scan(s, q3[l:l + 1], p3[3 * l:3 * l + 3], radius, metric, a, 10, MISSING[metric], nt[l:l + 1], e["flt"])
            assert all(x[0].tobytes() == y[l].tobytes() for x, y in zip(one, full)), (col, l)
        rev = ctx.maxsim_scan(s, q3[::-1], p3.reshape(L, 3, -1)[::-1].reshape(L * 3, -1), radius, metric, a, 10, MISSING[metric], nt[::-1].copy(),
                              e["flt"])
        assert all(x[::-1].tobytes() == y.tobytes() for x, y in zip(rev, full))
        # hits are the lims of the range call
        lims = ctx.range_scan(s, q3.reshape(L * 3, 32), p3, radius, metric, filter=e["flt"], cap=0)[0]
        want = np.diff(_np(lims)).reshape(L, 3) * (np.arange(3)[None, :] < nt[:, None])
        assert np.array_equal(full[4], want)
        fs = ctx.maxsim_search(parent, s, q3, 3, radius, metric, a, 10, MISSING[metric])
        lims = ctx.range_search(parent, s, q3.reshape(L * 3, 32), 3, radius, metric, cap=0)[0]
        assert np.array_equal(fs[4], np.diff(_np(lims)).reshape(L, 3))


def test_squared_l2_and_null_outputs(ctx, corpora):
    from quake_amd.capi import metric_code
    e = corpora("l2")
    s, parent, a = e["s"], e["parent"], e["attrs"]["forty"]
    q3, _ = _queries(e, 3)
    cand, ids = _cand(e, 3, "search", False)
    rowval, rowhas = GY.row_values(ids, *e["cols"]["forty"])
    ctx.set_squared_l2(True)
    try:
        want = MY.reduce(cand, 3, rowval, rowhas, 10, "l2", None, None, 2.0, squared=True)
        _eq(ctx.maxsim_search(parent, s, q3, 3, float("inf"), "l2", a, 10, 2.0), want, "squared")
    finally:
        ctx.set_squared_l2(False)
    host = ctx.maxsim_search(parent, s, q3, 3, float("inf"), "l2", a, 10, 2.0)
    P = lambda b: C.c_void_p(b.ctypes.data) if isinstance(b, np.ndarray) else C.c_void_p(b.data_ptr())  # noqa: E731
    tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}
    xf = np.ascontiguousarray(q3.reshape(L * 3, 32))
    for mem, xq in ((0, xf), (1, torch.from_numpy(xf).cuda())):
        for skip in range(1, 5):   # every output but the groups may be NULL, each on its own
            bufs = [np.full(h.shape, -7, h.dtype) if mem == 0 else torch.full(tuple(h.shape), -7, dtype=tdt[h.dtype], device="cuda")
                    for h in host]
            ptrs = [None if j == skip else P(b) for j, b in enumerate(bufs)]
            st = ctx.lib.qk_maxsim_search(ctx.h, parent.h, s.h, P(xq), L, 3, None, 3, metric_code("l2"), C.c_float(float("inf")), None, a.h,
                                          C.c_float(2.0), 10, *ptrs, mem, None)
            assert st == 0
            for j in range(5):
                assert (_np(bufs[j]) == -7).all() if j == skip else _np(bufs[j]).tobytes() == host[j].tobytes(), (mem, skip, j)


# ---- 4. several passes ------------------------------------------------------------------------------------------------------------------
def test_passes(ctx):
    """The construction of tests/test_grouped_search.py::test_passes: one unprobed list of 300 000 rows makes a call with P = 32 run
    in many passes while the probed work stays tiny.  The pass count follows the workspace rule of include/quake_hip.h: the wide-k
    rule over the sub-queries, lowered to a multiple of T."""
    from quake_amd.capi import Store
    d, nsmall, big = 16, 48, 300000
    rng = np.random.default_rng(491)
    sizes = rng.integers(0, 60, size=nsmall)
    sizes[[3, 17]] = 0
    sizes = np.concatenate([sizes, [big]]).astype(np.int64)
    offsets = np.zeros(nsmall + 2, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    Lq, T, P, k = 341, 3, 32, 10
    q3 = rng.standard_normal((Lq, T, d)).astype(np.float32)
    pids = np.stack([rng.permutation(nsmall)[:P] for _ in range(Lq * T)]).astype(np.int64)
    pids[rng.random(pids.shape) < 0.05] = -1
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    vals = ids % 40 - 20
    a = _attr(s, ids, vals)
    ub = P * big
    qc = min(Lq * T, (1 << 29) // ub) // T * T            # sub-queries per pass: a logical query never straddles a pass
    # (the tables are laid out inside a pass by the hits -- about 2 700 per logical query here, far from the pool's bound -- and do
    # not change the pass count)
    passes = -(-Lq * T // qc)
    assert passes == 19 and passes > 1 and qc % 3 == 0 and qc == 54
    want = MY.scan(q3, vecs, ids, offsets, pids, k, "l2", ids, vals, missing=1.0)
    assert (want[3] == 40).all()
    ctx.set_timing(1)
    try:
        *got, tm = ctx.maxsim_scan(s, q3, pids, float("inf"), "l2", a, k, 1.0, timing=True)
        assert tm["n_items"] == passes
        _eq(got, want, "passes")
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 5. limits and errors at the C level ------------------------------------------------------------------------------------------------
def test_limits(ctx, corpora):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter, Store
    e, e2 = corpora("l2"), corpora("ip")
    s, parent, a = e["s"], e["parent"], e["attrs"]["forty"]
    q3, p3 = _queries(e, 3)
    plain = ctx.maxsim_search(parent, s, q3, 3, 6.0, "l2", a, 10, 1.0)
    assert plain[4].sum() > 0

    def both(match, x=q3, k=10, missing=1.0, nt=None, attr=a, radius=6.0, flt=None, pids=p3):
        with pytest.raises(QuakeHipError, match=match):
            ctx.maxsim_search(parent, s, x, 3, radius, "l2", attr, k, missing, nt, flt)
        if x.shape[1] > 0:   # (without sub-queries there is no pids array to hand over)
            with pytest.raises(QuakeHipError, match=match):
                ctx.maxsim_scan(s, x, pids, radius, "l2", attr, k, missing, nt, flt)

    for k, match in ((0, "QK_ERR_INVALID.*k=0"), (-3, "QK_ERR_INVALID.*k=-3"), (1025, "QK_ERR_UNSUPPORTED.*k=1025 exceeds QK_MAXSIM_MAX_K")):
        both(match, k=k)
    both("QK_ERR_UNSUPPORTED.*T=65 exceeds QK_MAXSIM_MAX_TOKENS", x=np.zeros((2, 65, 32), np.float32), pids=np.arange(12))
    both("QK_ERR_INVALID.*T=0", x=np.zeros((2, 0, 32), np.float32), pids=np.arange(12))
    both("QK_ERR_INVALID.*missing is NaN", missing=float("nan"))
    both("QK_ERR_INVALID.*NaN", radius=float("nan"))
    both("QK_ERR_INVALID.*n_tokens\\[2\\]=4", nt=[3, 0, 4, 1, 1])
    both("QK_ERR_INVALID.*n_tokens\\[0\\]=-1", nt=[-1, 0, 3, 1, 1])
    both("QK_ERR_INVALID.*another store", attr=e2["attrs"]["forty"])
    both("QK_ERR_INVALID.*null", attr=None)
    f2 = Filter(e2["s"], e2["c"]["ids"][:100], "allow")
    both("QK_ERR_INVALID.*another store", flt=f2)
    f2.close()
    # a device n_tokens is clamped, not refused
    xd = torch.from_numpy(q3).cuda()
    wild = ctx.maxsim_search(parent, s, xd, 3, 6.0, "l2", a, 10, 1.0, torch.tensor([3, -5, 99, 1, 2], dtype=torch.int32, device="cuda"))
    tame = ctx.maxsim_search(parent, s, q3, 3, 6.0, "l2", a, 10, 1.0, [3, 0, 3, 1, 2])
    _eq(wild, tame, "clamped")
    # L == 0 is served
    empty = ctx.maxsim_search(parent, s, q3[:0], 3, 6.0, "l2", a, 5)
    assert empty[0].shape == (0, 5) and empty[4].shape == (0, 3)
    # no lists probed: a store without lists -- all padding and zeros
    bare = Store(ctx, 32)
    ab = _attr(bare, [1], [1])
    for metric, pad in (("l2", np.inf), ("ip", -np.inf)):
        got = ctx.maxsim_search(None, bare, q3, 1, 6.0, metric, ab, 4, 1.0)
        assert (got[0] == 0).all() and (got[1] == pad).all() and all((got[j] == 0).all() for j in (2, 3, 4))
    ab.close()
    bare.close()
    _eq(ctx.maxsim_search(parent, s, q3, 3, 6.0, "l2", a, 10, 1.0), plain, "after the refusals")


# ---- 6. the mirrors -----------------------------------------------------------------------------------------------------------------------
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
    return (r.groups, r.scores, r.matched, r.n_groups, r.hits)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(qb, metric, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(461)
    n, d, Lq, T = 6000, 32, 7, 4
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = x[torch.randint(0, n, (Lq * T,), generator=g)].reshape(Lq, T, d) + 0.1 * torch.randn(Lq, T, d, generator=g)
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(462)))
    idx = _build(quake, x, ids, 20, metric)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    for m in (idx, loaded):
        m.set_attribute("doc", ids[::2], ids[::2] % 97 - 3)
    radius = 5.5 if metric == "l2" else 6.0
    inf = float("inf") if metric == "l2" else float("-inf")
    missing = 3.25 if metric == "l2" else None
    nts = [4, 0, 2, 4, 1, 3, 4]
    for k in (3, 300):
        sp, spc = quake.SearchParams(), qb.SearchParams()
        for p in (sp, spc):
            p.nprobe, p.k = 5, k
        for exclude in (None, True):
            sp.filter = None if exclude is None else idx.make_filter(S, exclude)
            spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
            for rad in (None, radius):
                for nt in (None, nts):
                    want = idx._ctx.maxsim_search(idx.parent._store if idx.parent is not None else None, idx._store, q.numpy(), 5,
                                                  inf if rad is None else rad, metric, idx._attributes()["doc"], k,
                                                  0.0 if missing is None else missing, nt, sp.filter._h if sp.filter is not None else None)
                    assert want[4].sum() > 0 and want[3].max() > 0
                    t = (metric, k, exclude, rad, nt)
                    r = idx.multi_vector_search(q, "doc", sp, radius=rad, n_tokens=nt, missing=missing)
                    _eq(_res(r), want, ("python",) + t)
                    assert r.column == "doc" and r.timing_info.n_queries == Lq and tuple(r.groups.shape) == (Lq, k)
                    rd = idx.multi_vector_search(q.cuda(), "doc", sp, radius=rad, n_tokens=None if nt is None else torch.tensor(nt), missing=missing)
                    assert all(o.is_cuda for o in _res(rd))
                    _eq(_res(rd), want, ("python, device",) + t)
                    for xq in (q, q.cuda()):
                        rc = loaded.multi_vector_search(xq, "doc", spc, radius=rad, n_tokens=nt, missing=missing)
                        assert rc.groups.is_cuda == xq.is_cuda and rc.hits.is_cuda == xq.is_cuda and rc.column == "doc"
                        _eq(_res(rc), want, ("compiled", xq.is_cuda) + t)
        sp.filter = spc.filter = None
    for m, p in ((idx, sp), (loaded, spc)):
        empty = m.multi_vector_search(q[:0], "doc", p, missing=1.0)
        assert tuple(empty.groups.shape) == (0, 300) and tuple(empty.hits.shape) == (0, T) and tuple(empty.n_groups.shape) == (0,)


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(471)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(6, 3, 16, generator=g)
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

        plain = idx.multi_vector_search(qq, "doc", params(), radius=5.0, missing=1.0)
        assert plain.hits.sum() > 0
        for kw, match in ((dict(recall_target=0.9), "recall_target"),
                          (dict(filters=[idx.make_filter(ids[:1000])], query_filter=torch.zeros(6, dtype=torch.int32)), "query_filter"),
                          (dict(max_nprobe=8), "max_nprobe"),
                          (dict(filter_exact_rows=100, filter=idx.make_filter(ids[:50])), "filter_exact_rows"),
                          (dict(filters_exact_rows=100), "filters_exact_rows"),
                          (dict(filter=other.make_filter(ids[:1000])), "another index"),
                          (dict(k=0), "k=0 must be between 1 and 1024"),
                          (dict(k=1025), "k=1025 must be between 1 and 1024")):
            with pytest.raises(RuntimeError, match=match):
                idx.multi_vector_search(qq, "doc", params(**kw), radius=5.0, missing=1.0)
        with pytest.raises(RuntimeError, match="unknown attribute column 'nope'"):
            idx.multi_vector_search(qq, "nope", params(), missing=1.0)
        with pytest.raises(RuntimeError, match="NaN"):
            idx.multi_vector_search(qq, "doc", params(), radius=float("nan"), missing=1.0)
        with pytest.raises(RuntimeError, match="missing must be given for the l2 metric"):
            idx.multi_vector_search(qq, "doc", params())
        with pytest.raises(RuntimeError, match="missing is NaN"):
            idx.multi_vector_search(qq, "doc", params(), missing=float("nan"))
        with pytest.raises(RuntimeError, match=r"n_tokens\[1\]=4 must be between 0 and T=3"):
            idx.multi_vector_search(qq, "doc", params(), missing=1.0, n_tokens=[3, 4, 0, 1, 2, 3])
        with pytest.raises(RuntimeError, match="n_tokens has 2 entries for 6 queries"):
            idx.multi_vector_search(qq, "doc", params(), missing=1.0, n_tokens=[3, 1])
        with pytest.raises(RuntimeError, match="T=65 vectors per query must be between 1 and 64"):
            idx.multi_vector_search(torch.zeros(2, 65, 16), "doc", params(), missing=1.0)
        with pytest.raises(RuntimeError, match=r"x must be \[L, T, d\]"):
            idx.multi_vector_search(qq[0], "doc", params(), missing=1.0)
        # a call with two faults raises the same error in both mirrors: refusals, column, k, T, n_tokens, missing, filter, radius
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.multi_vector_search(qq, "nope", params(recall_target=0.9))
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.multi_vector_search(qq, "nope", params(k=0))
        with pytest.raises(RuntimeError, match="k=0"):
            idx.multi_vector_search(qq, "doc", params(k=0), radius=float("nan"))
        with pytest.raises(RuntimeError, match="missing must be given"):
            idx.multi_vector_search(qq, "doc", params(filter=other.make_filter(ids[:1000])), radius=float("nan"))
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.multi_vector_search(qq, "doc", params(), missing=1.0)
        again = idx.multi_vector_search(qq, "doc", params(), radius=5.0, missing=1.0)
        for u, v in zip(_res(again), _res(plain)):
            assert torch.equal(u, v)
