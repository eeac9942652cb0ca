"""Product-quantized search on the device (qk_pq_search / qk_pq_scan; Context.pq_search / pq_scan; Store.pq_*) against
tests/pq_yardstick.py: ids and distance bits.  The codebooks are supplied -- the sub-vectors of 256 seeded rows, two codewords of
sub-space 0 equal -- so that nothing but the training test depends on training."""
import numpy as np
import pytest
import torch

import oracle as O
import pq_yardstick as PY
from quake_amd._lib import QK_MEM_DEVICE, QK_METRIC_L2
from quake_amd.capi import Context, Store

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 500, 1500, 3000, 700, 4500, 33]
UNSUPPORTED, INVALID = 4, 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, tag):
    torch.cuda.synchronize()
    gi, gd = (o.cpu().numpy() if torch.is_tensor(o) else o for o in got[:2])
    want = tuple(o.cpu().numpy() if torch.is_tensor(o) else o for o in want[:2])
    assert (gi == want[0]).all(), (tag, "ids")
    assert (_bits(gd) == _bits(want[1])).all(), (tag, "distances")


def make_case(d, M, Q, nprobe, metric, seed, sizes=SIZES):
    """len(sizes) lists around their centroids in CSR (= arena) order; query i sits next to list i % len(sizes), so nprobe 1 reaches
    the empty list and the lists of 1 and 33 rows.  The three smallest lists are neighbours: nprobe 3 from a query next to one of
    them reaches those three and nothing else (34 rows of SIZES: padding from k = 100 on)"""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    cent = (0.6 * rng.standard_normal((n, d))).astype(np.float32)
    small = np.argsort(sizes, kind="stable")[:3]
    cent[small[1:]] = cent[small[0]] + (0.05 * rng.standard_normal((2, d))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lists = np.repeat(np.arange(n), sizes)
    vecs = np.clip(cent[lists] + 0.3 * rng.standard_normal((lists.shape[0], d)), -3.5, 3.5).astype(np.float32)
    q = (cent[np.arange(Q) % n] + 0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    ids = rng.permutation(lists.shape[0]).astype(np.int64) + 7
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    cb = np.ascontiguousarray(vecs[rng.choice(vecs.shape[0], 256, replace=False)].reshape(256, M, d // M).transpose(1, 0, 2))
    cb[0, 7] = cb[0, 3]  # (the rows that lie on it meet two equal e: the smaller c is the code)
    return dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets, q=q, pids=pids, cb=cb)


def _want(c, k, fk, metric, **kw):
    return PY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, metric, c["cb"], **kw)


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def _stores(ctx, c, d, codebooks=True):
    s = Store(ctx, d)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = Store(ctx, d)
    n = c["cent"].shape[0]
    parent.build_csr(np.array([0, n], np.int64), np.arange(n, dtype=np.int64), c["cent"])
    if codebooks:
        s.pq_set_codebooks(c["cb"])
    return s, parent


# (d, M, metric, Q, nprobe, k, fetch_k): every value of each list at least once, not their product
SHAPES = [(1, 1, "l2", 33, 1, 1, 1), (96, 32, "ip", 33, 8, 100, 1000), (130, 65, "l2", 17, 3, 448, 4096), (128, 128, "ip", 17, 3, 100, 1000),
          (100, 25, "l2", 33, 1, 100, 1000), (768, 96, "ip", 1, 8, 10, 448), (8192, 128, "l2", 17, 3, 10, 448)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_M%d_%s_Q%d_np%d_k%d_f%d" % s)
def test_against_the_yardstick(ctx, shape):
    """Before any device call the yardstick shows what the case proves: some query returns a row, some query has several rows at
    the cut key, so the tie rule decides (fetch_k = 1 too: two rows share the smallest key), and some query ends in padding.  The
    one exception: with every list probed, each query sees all rows of the store and none can end in padding -- which is also
    where the single query goes, since one query cannot both end in padding and have a cut."""
    d, M, metric, Q, nprobe, k, fk = shape
    # (dsub 64: the LDS limit of the encode; 33 MB of rows are enough, and lists of 0 + 1 + 5 rows end in padding at k = 10)
    sizes = SIZES if d < 8192 else [0, 1, 5, 300, 700]
    c = make_case(d, M, Q, nprobe, metric, seed=2700 + d + Q + fk, sizes=sizes)
    want = _want(c, k, fk, metric, want_cut=True)
    assert (want[0][:, 0] >= 0).any() and want[2].max() > 1
    assert nprobe == len(sizes) or (want[0][:, -1] == -1).any()
    s, parent = _stores(ctx, c, d, codebooks=False)
    before = s.device_bytes()
    arena_rows = before // (4 * ((d + 15) // 16 * 16) + 12)
    s.pq_set_codebooks(c["cb"])
    info = s.pq_info()
    assert (info["M"], info["dsub"], info["codebooks"], info["valid"], info["bytes"]) == (M, d // M, True, False, 0)
    assert (s.pq_codebooks() == c["cb"]).all() and s.device_bytes() == before
    _eq(ctx.pq_search(parent, s, c["q"], nprobe, k, fk, metric), want, "search, host")
    assert ctx.last_scan_kernel() == "k_pq_select (PQ codes)"
    info = s.pq_info()
    assert info["valid"] and info["bytes"] == s.device_bytes() - before == 16 * ((M + 15) // 16) * arena_rows > 0
    _eq(ctx.pq_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, metric), want, "scan, device")
    s.pq_drop()
    info = s.pq_info()
    assert not info["valid"] and info["bytes"] == 0 and info["codebooks"] and s.device_bytes() == before
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_probe_order_against_arena_order(ctx, metric):
    """600 + 5000 identical rows in two probed lists, the list of 5000 named first: the candidates are the first fetch_k of them in
    arena order -- the 600 and the head of the 5000 -- whatever the probe order"""
    d, M, sizes = 100, 25, [0, 1, 500, 600, 3000, 700, 5000, 33]
    c = make_case(d, M, 3, 2, metric, seed=77, sizes=sizes)
    o = c["offsets"]
    c["vecs"][o[3]:o[4]] = c["vecs"][o[6]:o[7]] = c["cent"][6]
    c["q"][:] = c["cent"][6] + np.float32(0.01)
    c["pids"] = np.array([[6, 3], [3, 6], [6, 3]], np.int64)
    want = _want(c, 100, 1000, metric, want_cut=True)
    assert (want[2] == 5600).all()
    s, parent = _stores(ctx, c, d)
    _eq(ctx.pq_scan(s, c["q"], c["pids"], 100, 1000, metric), want, metric)
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fetch_k_covers_the_probed_rows_and_the_store_changes(ctx, metric):
    d, M, sizes = 100, 25, [0, 1, 500, 1500, 300, 700, 1200, 33]  # (any three lists hold at most 3400 rows)
    c = make_case(d, M, 33, 3, metric, seed=5, sizes=sizes)
    c["q"][1, 5], c["q"][2, 7], c["q"][3, :2] = np.nan, np.inf, (-np.inf, np.nan)  # (every u of these queries is 0)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.pq_search(parent, s, c["q"], 3, 100, 4096, metric), ctx.search(parent, s, c["q"], 3, 100, metric), "covers")
    # rows leave a list and rows join the last list of the arena: the codebooks stay, stale codes would show
    for change in (lambda: s.remove_ids(c["ids"][c["offsets"][4] + 10:c["offsets"][4] + 40]),
                   lambda: s.add_entries(7, np.arange(8, dtype=np.int64) + 100000, np.full((8, d), 3.0, np.float32))):
        change()
        info = s.pq_info()
        assert not info["valid"] and info["codebooks"] and (s.pq_codebooks() == c["cb"]).all()
        lists = [s.get_list(p) for p in range(len(SIZES))]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
        want = PY.case(c["q"], vecs, ids, offs, c["pids"], 10, 448, metric, c["cb"])
        _eq(ctx.pq_scan(s, c["q"], c["pids"], 10, 448, metric), want, "changed")
        assert s.pq_info()["valid"]
    s.close()
    parent.close()


def test_training(ctx):
    d, M, k, fk = 32, 8, 10, 100
    c = make_case(d, M, 17, 3, "l2", seed=41, sizes=[0, 1, 500, 1500, 1300, 700, 33])
    s, parent = _stores(ctx, c, d, codebooks=False)
    s.pq_train(ctx, M, max_rows=4096, niter=5, seed=3)
    c["cb"] = s.pq_codebooks()
    assert c["cb"].shape == (M, 256, d // M) and np.isfinite(c["cb"]).all() and s.pq_info()["codebooks"]
    _eq(ctx.pq_search(parent, s, c["q"], 3, k, fk, "l2"), _want(c, k, fk, "l2"), "trained")
    # 256 codewords against one: the reconstruction error lies strictly below the rows' total variance
    x = c["vecs"].astype(np.float64)
    cx = PY.codes(c["vecs"], c["cb"])
    recon = np.concatenate([c["cb"][m][cx[:, m]] for m in range(M)], 1)
    assert ((x - recon) ** 2).sum(1).mean() < ((x - x.mean(0)) ** 2).sum(1).mean()
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    d, M = 64, 16
    c = make_case(d, M, 17, 3, "l2", seed=6)
    s, parent = _stores(ctx, c, d, codebooks=False)
    flat = Store(ctx, d)
    flat.build_csr(np.array([0, c["vecs"].shape[0]], np.int64), c["ids"], c["vecs"])
    flat.pq_set_codebooks(c["cb"])
    lib, q = ctx.lib, torch.from_numpy(c["q"]).cuda()
    pids = torch.from_numpy(np.ascontiguousarray(c["pids"])).cuda()
    ids = torch.full((17, 449), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 449), -7.0, device="cuda")
    L2, DEV = QK_METRIC_L2, QK_MEM_DEVICE

    def search(st, k, fk, par=parent):
        return lib.qk_pq_search(ctx.h, par.h if par else None, st.h, q.data_ptr(), 17, 3, k, fk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None)

    def scan(st, k, fk):
        return lib.qk_pq_scan(ctx.h, st.h, q.data_ptr(), 17, pids.data_ptr(), 3, k, fk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None)

    assert search(s, 10, 448) == scan(s, 10, 448) == UNSUPPORTED and b"train or set codebooks first" in lib.qk_last_error()
    for shape, status in (((3, 256, 21), INVALID), ((129, 256, 1), UNSUPPORTED)):  # M does not divide d; M > 128
        assert lib.qk_store_pq_set_codebooks(s.h, shape[0], np.zeros(shape, np.float32).ctypes.data) == status
    wide = Store(ctx, 130)  # dsub = 65
    assert lib.qk_store_pq_set_codebooks(wide.h, 2, np.zeros((2, 256, 65), np.float32).ctypes.data) == UNSUPPORTED
    wide.close()
    bad = c["cb"].copy()
    bad[5, 200, 1] = np.inf
    assert lib.qk_store_pq_set_codebooks(s.h, M, bad.ctypes.data) == INVALID and not s.pq_info()["codebooks"]
    s.pq_set_codebooks(c["cb"])
    for k, fk, status in ((11, 10, INVALID), (10, 4097, UNSUPPORTED), (449, 4096, UNSUPPORTED)):
        assert search(s, k, fk) == scan(s, k, fk) == status
    assert search(flat, 10, 448, par=None) == UNSUPPORTED and b"flat index" in lib.qk_last_error()
    # a store that holds a value that is not finite has no mirror
    s.add_entries(5, np.array([424242], np.int64), np.full((1, d), np.inf, np.float32))
    assert scan(s, 10, 448) == UNSUPPORTED
    assert b"list 5 holds a value that is not finite" in lib.qk_last_error() and not s.pq_info()["valid"]
    torch.cuda.synchronize()
    assert (ids == -7).all() and (dist == -7.0).all()
    for st in (s, parent, flat):
        st.close()


def test_mirrors(tmp_path):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    g = torch.Generator().manual_seed(78)
    n, d, M, k, fk, metric = 6000, 128, 16, 10, 1000, "l2"
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = x[torch.randint(0, n, (33,), generator=g)] + 0.05 * torch.randn(33, d, generator=g)
    cb = x[:256].reshape(256, M, d // M).transpose(0, 1).contiguous()
    built = quake.QuakeIndex()
    bp = quake.IndexBuildParams()
    bp.nlist, bp.metric = 12, metric
    built.build(x, ids, bp)
    built.save(str(tmp_path / "index"))
    # (ties at the cut are the rule and follow the arena: every mirror against the C call on an arena laid out as its own)
    loaded, loaded_cpp = quake.QuakeIndex(), qb.QuakeIndex()
    loaded.load(str(tmp_path / "index"))
    loaded_cpp.load(str(tmp_path / "index"))
    for mod, m, ref in ((quake, built, built), (quake, loaded, loaded), (qb, loaded_cpp, loaded)):
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, k
        with pytest.raises(RuntimeError, match="train or set codebooks first"):
            m.pq_search(q.cuda(), sp, fk)
        m.set_pq_codebooks(cb)
        ref._store.pq_set_codebooks(cb)  # (the reference of the C++ mirror is another index; the previous iteration trained codebooks on `loaded`)
        r = m.pq_search(q.cuda(), sp, fk)
        _eq((r.ids, r.distances), ref._ctx.pq_search(ref.parent._store, ref._store, q.cuda(), 4, k, fk, metric), mod.__name__)
        with pytest.raises(RuntimeError, match="fetch_k=4097 must not exceed 4096"):
            m.pq_search(q, sp, 4097)
        m.train_pq(8, max_rows=4096, niter=2, seed=1)
        assert m.pq_search(q.cuda(), sp, fk).ids.shape == (33, k)
