"""Binary search on the device (qk_bin_search / qk_bin_scan; Context.bin_search / bin_scan; QuakeIndex.binary_search in both
mirrors) against tests/bin_yardstick.py: ids and distance bits."""
import numpy as np
import pytest
import torch

import bin_yardstick as BY
import oracle as O
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


def make_case(d, Q, nprobe, metric, seed, sizes=SIZES):
    """len(sizes) lists around their centroids in CSR (= arena) order; query i sits next to list 1 + i % 7, so nprobe 1 reaches the
    lists of 1 and 33 rows (fewer rows than fetch_k: padding)"""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    cent = (0.6 * rng.standard_normal((n, d))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lists = np.repeat(np.arange(n), sizes)
    vecs = np.clip(cent[lists] + 0.3 * rng.standard_normal((lists.shape[0], d)), -3.5, 3.5).astype(np.float32)
    q = (cent[1 + np.arange(Q) % (n - 1)] + 0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    ids = rng.permutation(lists.shape[0]).astype(np.int64) + 7
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    return dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets, q=q, pids=pids)


def _at_cut(c, metric, fetch_k, qi=0):
    """how many probed rows of query qi share the Hamming key of the fetch_k-th place"""
    m = BY.params(c["vecs"], metric)
    rows = np.concatenate([np.arange(c["offsets"][p], c["offsets"][p + 1]) for p in c["pids"][qi] if p >= 0])
    key = BY.keys(BY.codes(c["q"][qi], m), BY.codes(c["vecs"][rows], m))
    return int((key == np.sort(key)[fetch_k - 1]).sum()) if rows.shape[0] >= fetch_k else 0


def _want(c, k, fk, metric):
    return BY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, metric)


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
SHAPES = [(1, "l2", 17, 3, 10, 448), (100, "ip", 33, 8, 100, 1000), (128, "ip", 1, 1, 1, 1), (130, "ip", 17, 3, 448, 4096),
          (192, "l2", 33, 8, 10, 448), (1, "ip", 17, 8, 448, 4096), (128, "l2", 17, 1, 100, 1000), (130, "l2", 33, 3, 100, 1000)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_%s_Q%d_np%d_k%d_f%d" % s)
def test_against_the_yardstick(ctx, shape):
    d, metric, Q, nprobe, k, fk = shape
    c = make_case(d, Q, nprobe, metric, seed=2600 + d + Q + fk)
    probed = np.diff(c["offsets"])[c["pids"]].sum(1)
    assert nprobe > 1 or Q == 1 or (probed < min(fk, k)).any()   # (nprobe 1: a query that ends in padding)
    assert fk == 1 or max(_at_cut(c, metric, fk, qi) for qi in range(Q)) > 1  # (equal keys at the cut: the tie rule decides)
    want = _want(c, k, fk, metric)
    s, parent = _stores(ctx, c, d)
    assert not s.bin_info()["valid"]
    before = s.device_bytes()
    _eq(ctx.bin_search(parent, s, c["q"], nprobe, k, fk, metric), want, "search, host")
    assert ctx.last_scan_kernel() == "k_bin_select (sign codes)"
    info = s.bin_info()
    assert info["valid"] and info["bytes"] == s.device_bytes() - before > 0 and info["bytes"] % (16 * ((d + 127) // 128)) == 0
    _eq(ctx.bin_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, metric), want, "scan, device")
    s.bin_drop()
    assert not s.bin_info()["valid"] and s.bin_info()["bytes"] == 0 and s.device_bytes() == before
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_probe_order_against_arena_order(ctx, metric):
    """600 + 5000 identical rows in two probed lists, the list of 5000 named first: the candidates are the first fetch_k of them in
    arena order -- the 600 and the head of the 5000 -- whatever the probe order"""
    d, sizes = 100, [0, 1, 500, 600, 3000, 700, 5000, 33]
    c = make_case(d, 3, 2, metric, seed=77, sizes=sizes)
    o = c["offsets"]
    c["vecs"][o[3]:o[4]] = c["vecs"][o[6]:o[7]] = c["cent"][6]
    c["q"][:] = c["cent"][6] + np.float32(0.01)
    c["pids"] = np.array([[6, 3], [3, 6], [6, 3]], np.int64)
    assert _at_cut(c, metric, 1000) == 5600
    s, parent = _stores(ctx, c, d)
    _eq(ctx.bin_scan(s, c["q"], c["pids"], 100, 1000, metric), _want(c, 100, 1000, metric), metric)
    s.close()
    parent.close()


@pytest.mark.parametrize("fetch_k", [1000, 4096])
def test_beyond_the_lds_key_cache(ctx, fetch_k):
    d = 64
    probe = Store(ctx, d)
    cap = probe.bin_info()["cache_rows"]  # (0 in a build without the cache, whose capacity at d = 64 would be 73072 rows)
    probe.close()
    c = make_case(d, 3, 2, "l2", seed=91, sizes=[0, 1, 500, max(cap, 73072) + 1000, 33])
    c["pids"] = np.array([[3, 2], [2, 3], [3, 4]], np.int64)
    assert _at_cut(c, "l2", fetch_k) > 1
    s, parent = _stores(ctx, c, d)
    _eq(ctx.bin_scan(s, c["q"], c["pids"], 100, fetch_k, "l2"), _want(c, 100, fetch_k, "l2"), fetch_k)
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fetch_k_covers_the_probed_rows_and_the_store_changes(ctx, metric):
    d = 100
    c = make_case(d, 33, 3, metric, seed=5)
    s, parent = _stores(ctx, c, d)
    sel = np.nonzero(np.diff(c["offsets"])[c["pids"]].sum(1) <= 4096)[0]
    assert sel.shape[0] > 0
    _eq(ctx.bin_search(parent, s, c["q"][sel], 3, 100, 4096, metric), ctx.search(parent, s, c["q"][sel], 3, 100, metric), "covers")
    # rows leave a list, and rows that move column 0's centre join the last list of the arena: a stale mirror would show
    for change in (lambda: s.remove_ids(c["ids"][c["offsets"][4] + 10:c["offsets"][4] + 40]),
                   lambda: s.add_entries(7, np.arange(8, dtype=np.int64) + 100000, np.full((8, d), 9.0, np.float32))):
        change()
        assert not s.bin_info()["valid"]
        lists = [s.get_list(p) for p in range(len(SIZES))]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
        _eq(ctx.bin_scan(s, c["q"], c["pids"], 10, 448, metric), BY.case(c["q"], vecs, ids, offs, c["pids"], 10, 448, metric), "changed")
        assert s.bin_info()["valid"]
    s.bin_drop()
    _eq(ctx.bin_scan(s, c["q"], c["pids"], 10, 448, metric), BY.case(c["q"], vecs, ids, offs, c["pids"], 10, 448, metric), "rebuilt")
    assert s.bin_info()["valid"]
    s.close()
    parent.close()


def test_ip_with_nan_inf_and_signed_zeros(ctx):
    d = 100
    c = make_case(d, 17, 3, "ip", seed=12)
    rng = np.random.default_rng(13)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
    for p in (2, 3, 4):  # a few values in every tenth row of three lists
        rows = np.arange(c["offsets"][p], c["offsets"][p + 1], 10)
        c["vecs"][rows[:, None], rng.integers(0, d, (rows.shape[0], 3))] = special[rng.integers(0, 5, (rows.shape[0], 3))]
    c["q"][0, 5], c["q"][1, :5], c["q"][2, 7] = np.nan, special[[3, 4, 1, 2, 3]], np.inf
    want = _want(c, 10, 448, "ip")
    assert (want[0][0] == -1).all() and (want[0][3] >= 0).all()  # (a NaN in the query: every exact key is NaN, nothing is returned)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.bin_scan(s, c["q"], c["pids"], 10, 448, "ip"), want, "ip")
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    d = 64
    c = make_case(d, 17, 3, "l2", seed=6)
    s, parent = _stores(ctx, c, d)
    lib, q = ctx.lib, torch.from_numpy(c["q"]).cuda()
    pids = torch.from_numpy(np.ascontiguousarray(np.resize(c["pids"], (17, 1025)))).cuda()
    ids = torch.full((17, 449), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 449), -7.0, device="cuda")
    L2, DEV = QK_METRIC_L2, QK_MEM_DEVICE
    for k, fk, status in ((10, 4097, UNSUPPORTED), (449, 4096, UNSUPPORTED), (11, 10, INVALID)):
        assert lib.qk_bin_search(ctx.h, parent.h, s.h, q.data_ptr(), 17, 3, k, fk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None) == status
        assert lib.qk_bin_scan(ctx.h, s.h, q.data_ptr(), 17, pids.data_ptr(), 3, k, fk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None) == status
    assert lib.qk_bin_scan(ctx.h, s.h, q.data_ptr(), 17, pids.data_ptr(), 1025, 10, 448, L2, ids.data_ptr(), dist.data_ptr(), DEV, None) == UNSUPPORTED
    # an L2 store that holds a value that is not finite has no mirror
    s.add_entries(5, np.array([424242], np.int64), np.full((1, d), np.inf, np.float32))
    assert lib.qk_bin_scan(ctx.h, s.h, q.data_ptr(), 17, pids.data_ptr(), 3, 10, 448, L2, ids.data_ptr(), dist.data_ptr(), DEV, None) == UNSUPPORTED
    assert b"list 5 holds a value that is not finite" in lib.qk_last_error() and not s.bin_info()["valid"]
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
        r = m.binary_search(q.cuda(), sp, fk)
        _eq((r.ids, r.distances), ref._ctx.bin_search(ref.parent._store, ref._store, q.cuda(), 4, k, fk, metric), mod.__name__)
        with pytest.raises(RuntimeError, match="fetch_k=4097 must not exceed 4096"):
            m.binary_search(q, sp, 4097)
