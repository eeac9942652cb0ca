"""Deep quantized search on the device (qk_sq8_search_deep / qk_sq8_scan_deep; Context.sq8_search / sq8_scan with deep=True;
QuakeIndex.quantized_search(deep=True) in both mirrors) against tests/sq8_yardstick.py: ids and distance bits."""
import numpy as np
import pytest
import torch

import oracle as O
import sq8_yardstick as SY
from quake_amd.capi import Context, Store

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 500, 1500, 3000, 700, 4500, 33]
CAP = 4096  # QK_SQ8_DEEP_CAP: entries of a query's contested slice


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, tag):
    torch.cuda.synchronize()
    gi, gd = (o.cpu().numpy() if torch.is_tensor(o) else o for o in got[:2])
    want = tuple(o.cpu().numpy() if torch.is_tensor(o) else o for o in want[:2])
    assert (gi == want[0]).all(), (tag, "ids")
    assert (_bits(gd) == _bits(want[1])).all(), (tag, "distances")


def make_case(d, Q, nprobe, metric, seed, sizes=SIZES, grid=False):
    """len(sizes) lists around their centroids in CSR (= arena) order; query i sits next to list 1 + i % 7, so nprobe 1 reaches the
    lists of 1 and 33 rows (fewer rows than fetch_k: padding).  grid: every value a small multiple of the code step 2^-5 (the planted
    +-127 steps in column 0 fix the scale), so that equal integer keys are the rule."""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    cent = (0.6 * rng.standard_normal((n, d))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lists = np.repeat(np.arange(n), sizes)
    vecs = np.clip(cent[lists] + 0.3 * rng.standard_normal((lists.shape[0], d)), -3.5, 3.5).astype(np.float32)
    q = (cent[1 + np.arange(Q) % (n - 1)] + 0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    if grid:
        step = np.float32(0.03125)
        vecs = (step * rng.integers(-2, 3, vecs.shape)).astype(np.float32)
        vecs[offsets[2], 0], vecs[offsets[2] + 1, 0] = 127 * step, -127 * step
        q = (step * rng.integers(-2, 3, q.shape)).astype(np.float32)
        assert SY.params(vecs, metric)[1] == step
    ids = rng.permutation(lists.shape[0]).astype(np.int64) + 7
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    return dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets, q=q, pids=pids)


def _at_cut(c, metric, fetch_k, qi=0):
    """how many probed rows of query qi share the approximate key of the fetch_k-th place"""
    m, s = SY.params(c["vecs"], metric)
    rows = np.concatenate([np.arange(c["offsets"][p], c["offsets"][p + 1]) for p in c["pids"][qi] if p >= 0])
    key = SY.keys(SY.query_codes(c["q"][qi:qi + 1], m, s, metric)[0], SY.codes(c["vecs"][rows], m, s), metric)
    return int((key == np.sort(key)[fetch_k - 1]).sum()) if rows.shape[0] >= fetch_k else 0


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def _stores(ctx, c, d):
    s = Store(ctx, d)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = Store(ctx, d)
    n = c["cent"].shape[0]
    parent.build_csr(np.array([0, n], np.int64), np.arange(n, dtype=np.int64), c["cent"])
    return s, parent


# (d, metric, Q, nprobe, k, fetch_k): every value of each list at least once, not their product
SHAPES = [(64, "l2", 1, 1, 1, 1), (100, "ip", 17, 3, 10, 448), (192, "l2", 33, 8, 10, 449), (64, "ip", 33, 3, 100, 1000),
          (100, "l2", 17, 8, 448, 4096), (192, "ip", 17, 1, 10, 449), (64, "l2", 17, 1, 100, 1000), (100, "ip", 1, 8, 448, 4096)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_%s_Q%d_np%d_k%d_f%d" % s)
def test_against_the_yardstick(ctx, shape):
    d, metric, Q, nprobe, k, fk = shape
    c = make_case(d, Q, nprobe, metric, seed=2500 + d + Q + fk)
    probed = np.diff(c["offsets"])[c["pids"]].sum(1)
    assert nprobe > 1 or Q == 1 or (probed < min(fk, k)).any()   # (nprobe 1: a query that ends in padding)
    want = SY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, metric)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.sq8_search(parent, s, c["q"], nprobe, k, fk, metric, deep=True), want, "search, host")
    assert ctx.last_scan_kernel() == "k_scan (int8 codes, counting)"
    _eq(ctx.sq8_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, metric, deep=True), want, "scan, device")
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("fetch_k", [1000, 4096])
def test_more_equal_keys_at_the_cut_than_the_contested_slice_holds(ctx, metric, fetch_k):
    """600 + 5000 identical rows in two probed lists, the list of 5000 named first: the candidates are the first fetch_k of them in
    arena order -- the 600 and the head of the 5000 -- whatever the probe order, and the answer the smallest ids among those."""
    d, sizes = 64, [0, 1, 500, 600, 3000, 700, 5000, 33]
    c = make_case(d, 3, 2, metric, seed=77, sizes=sizes)
    o = c["offsets"]
    v = c["cent"][6] * np.float32(2.0 if metric == "ip" else 1.0)
    c["vecs"][o[3]:o[4]] = v
    c["vecs"][o[6]:o[7]] = v
    c["q"][:] = v + np.float32(0.01)
    c["pids"] = np.array([[6, 3], [3, 6], [6, 3]], np.int64)
    assert _at_cut(c, metric, fetch_k) == 5600 > CAP
    want = SY.case(c["q"], c["vecs"], c["ids"], o, c["pids"], 100, fetch_k, metric)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.sq8_scan(s, c["q"], c["pids"], 100, fetch_k, metric, deep=True), want, fetch_k)
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_values_on_the_code_grid(ctx, metric):
    d = 64
    c = make_case(d, 17, 3, metric, seed=31, grid=True)
    assert max(_at_cut(c, metric, 1000, qi) for qi in range(17)) > 1
    s, parent = _stores(ctx, c, d)
    for k, fk in ((10, 449), (100, 1000)):
        _eq(ctx.sq8_search(parent, s, c["q"], 3, k, fk, metric, deep=True), SY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, metric), fk)
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_agrees_with_the_shipped_calls(ctx, metric):
    d = 100
    c = make_case(d, 33, 3, metric, seed=5)
    s, parent = _stores(ctx, c, d)
    for fk in (1, 40, 448):
        k = min(fk, 10)
        _eq(ctx.sq8_search(parent, s, c["q"], 3, k, fk, metric, deep=True), ctx.sq8_search(parent, s, c["q"], 3, k, fk, metric), fk)
    sel = np.nonzero(np.diff(c["offsets"])[c["pids"]].sum(1) <= 4096)[0]
    assert sel.shape[0] > 0
    _eq(ctx.sq8_search(parent, s, c["q"][sel], 3, 100, 4096, metric, deep=True), ctx.search(parent, s, c["q"][sel], 3, 100, metric), "covers")
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    d = 64
    c = make_case(d, 17, 3, "l2", seed=6)
    s, parent = _stores(ctx, c, d)
    lib, q = ctx.lib, torch.from_numpy(c["q"]).cuda()
    pids = torch.from_numpy(c["pids"]).cuda()
    ids = torch.full((17, 449), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 449), -7.0, device="cuda")
    UNSUPPORTED = 4
    for k, fk in ((10, 4097), (449, 4096), (449, 449)):
        assert lib.qk_sq8_search_deep(ctx.h, parent.h, s.h, q.data_ptr(), 17, 3, k, fk, 1, ids.data_ptr(), dist.data_ptr(), 1, None) == UNSUPPORTED
        assert lib.qk_sq8_scan_deep(ctx.h, s.h, q.data_ptr(), 17, pids.data_ptr(), 3, k, fk, 1, ids.data_ptr(), dist.data_ptr(), 1, None) == UNSUPPORTED
    assert lib.qk_sq8_search(ctx.h, parent.h, s.h, q.data_ptr(), 17, 3, 10, 449, 1, ids.data_ptr(), dist.data_ptr(), 1, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (ids == -7).all() and (dist == -7.0).all()
    s.close()
    parent.close()


def test_mirrors(tmp_path):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    g = torch.Generator().manual_seed(78)
    n, d, k, fk, metric = 6000, 128, 10, 1000, "l2"
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = x[torch.randint(0, n, (33,), generator=g)] + 0.05 * torch.randn(33, d, generator=g)
    idx = quake.QuakeIndex()
    bp = quake.IndexBuildParams()
    bp.nlist, bp.metric = 12, metric
    idx.build(x, ids, bp)
    idx.save(str(tmp_path / "index"))
    loaded = qb.QuakeIndex()
    loaded.load(str(tmp_path / "index"))
    lists = [idx._store.get_list(p) for p in range(12)]
    vecs, vids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    pids = idx._ctx.coarse(idx.parent._store, q.numpy(), 4, metric, values=False)[0]
    # (a built index keeps arena order only inside a list: the queries whose cut falls between two different keys)
    sel = [qi for qi in range(33) if _at_cut(dict(vecs=vecs, offsets=offs, pids=pids, q=q.numpy()), metric, fk, qi) == 1]
    assert len(sel) >= 8
    q, pids = q[sel], pids[sel]
    want = SY.case(q.numpy(), vecs, vids, offs, pids, k, fk, metric, cut_in_one_list=True)
    for mod, m in ((quake, idx), (qb, loaded)):
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, k
        r = m.quantized_search(q.cuda(), sp, fk, deep=True)
        _eq((r.ids, r.distances), want, mod.__name__)
        with pytest.raises(RuntimeError, match="fetch_k=1000 must not exceed 448"):
            m.quantized_search(q, sp, fk)
