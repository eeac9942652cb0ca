"""Rescored binary search on the device (qk_bin_search_rescored / qk_bin_scan_rescored; Context.bin_search / bin_scan with rescore_k;
QuakeIndex.binary_search(rescore_k=) in both mirrors) against a numpy reference composed of tests/bin_yardstick.py and
tests/sq8_yardstick.py: ids and distance bits.  The corpus, the comparison and the context are tests/test_bin_search.py's."""
import numpy as np
import pytest
import torch

import bin_yardstick as BY
import oracle as O
import sq8_yardstick as SY
from quake_amd._lib import QK_MEM_DEVICE, QK_METRIC_L2
from test_bin_search import INVALID, UNSUPPORTED, _eq, _stores, ctx, make_case  # noqa: F401 (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [0, 1, 15, 16, 17, 33, 300, 257]


def stages(q, vecs, offsets, pids, fetch_k, rescore_k, metric):
    """per query (probed rows, stage-1 shortlist, its integer keys, the survivors), all arena rows"""
    m = BY.params(vecs, metric)
    bx, bq = BY.codes(vecs, m), BY.codes(q, m)
    m8, s8 = SY.params(vecs, metric)
    cx, cq = SY.codes(vecs, m8, s8), SY.query_codes(q, m8, s8, metric)
    out = []
    for qi in range(q.shape[0]):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[qi] if p >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
        short = rows[np.lexsort((rows, BY.keys(bq[qi], bx[rows])))[:fetch_k]]
        key = SY.keys(cq[qi], cx[short], metric)
        out.append((rows, short, key, short[np.lexsort((short, key))[:rescore_k]]))
    return out


def reference(q, vecs, ids, offsets, pids, k, fetch_k, rescore_k, metric):
    """expected (ids [Q, k], dist [Q, k]): sq8_yardstick.case over each query's survivors as a store of their own with a fetch_k that
    takes them all -- O.pair_values and the final (key, id) order exactly as that function ends"""
    q, vecs, ids = np.ascontiguousarray(q, F), np.ascontiguousarray(vecs, F), np.asarray(ids, np.int64)
    parts = [SY.case(q[qi:qi + 1], vecs[st[3]], ids[st[3]], np.array([0, st[3].shape[0]]), np.zeros((1, 1), np.int64), k, max(st[3].shape[0], 1), metric)
             for qi, st in enumerate(stages(q, vecs, offsets, pids, fetch_k, rescore_k, metric))]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


N_SAME = 24


def plant_tie(c, p):
    """N_SAME identical vectors under different ids at the head of list p, and the first query that probes p on top of them: Hamming
    distance 0, so they lead that query's stage-1 shortlist, with one integer key.  Returns the query (None: nobody probes p)"""
    o = c["offsets"][p]
    c["vecs"][o:o + N_SAME] = c["vecs"][o]
    hit = np.nonzero((c["pids"] == p).any(1))[0]
    c["q"][hit[:1]] = c["vecs"][o]
    return int(hit[0]) if hit.shape[0] else None


def tie_across_the_cut(st, rescore_k):
    """the reference's cut falls inside a run of equal integer keys"""
    ks = np.sort(st[2])
    return ks.shape[0] > rescore_k and ks[rescore_k - 1] == ks[rescore_k]


# (d, Q, nprobe, k, rescore_k, fetch_k): every value of each list at least once, not their product
SHAPES = [(40, 1, 1, 1, 1, 1), (40, 17, 4, 1, 1, 17), (64, 33, 1, 10, 10, 64), (64, 17, 4, 10, 16, 17), (200, 33, 4, 10, 17, 300),
          (200, 17, 1, 10, 17, 300), (768, 17, 4, 100, 448, 448), (768, 33, 4, 100, 448, 4096), (2048, 17, 4, 10, 17, 300),
          (2048, 1, 1, 10, 10, 64), (40, 33, 4, 100, 448, 4096), (768, 1, 4, 10, 16, 17)]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_Q%d_np%d_k%d_r%d_f%d" % s)
def test_against_the_reference(ctx, shape, metric):
    d, Q, nprobe, k, rk, fk = shape
    c = make_case(d, Q, nprobe, metric, seed=2800 + d + Q + fk, sizes=SIZES)
    qt = plant_tie(c, 6)
    st = stages(c["q"], c["vecs"], c["offsets"], c["pids"], fk, rk, metric)
    if Q > 1:
        assert fk <= 17 or any(x[0].shape[0] < fk for x in st)    # a query with fewer probed rows than fetch_k
        assert nprobe > 1 or any(x[0].shape[0] < rk for x in st)  # nprobe 1: fewer than rescore_k
        assert rk >= min(N_SAME, fk) or tie_across_the_cut(st[qt], rk)  # a short rescore_k: the cut inside the planted block
    want = reference(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, rk, metric)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.bin_search(parent, s, c["q"], nprobe, k, fk, metric, rescore_k=rk), want, "search, host")
    assert ctx.last_scan_kernel() == "k_bin_select (sign codes) + k_sq8_rerank (int8 codes)"
    _eq(ctx.bin_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, metric, rescore_k=rk), want, "scan, device")
    assert s.bin_info()["valid"] and s.sq8_info()["valid"]
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_4096_candidates_fill_the_key_array(ctx, metric):
    d, fk, rk, k = 40, 4096, 448, 100
    c = make_case(d, 3, 2, metric, seed=41, sizes=[3000, 2000])
    c["pids"] = np.array([[0, 1], [1, 0], [0, 1]], np.int64)
    o = c["offsets"]
    c["vecs"][o[1] - 300:o[1] + 300] = c["vecs"][o[1]]  # one key for 600 rows across the two lists, most of them behind the cut
    c["q"][0] = c["vecs"][o[1]]
    st = stages(c["q"], c["vecs"], o, c["pids"], fk, rk, metric)
    assert all(x[1].shape[0] == 4096 for x in st) and tie_across_the_cut(st[0], rk)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.bin_scan(s, c["q"], c["pids"], k, fk, metric, rescore_k=rk), reference(c["q"], c["vecs"], c["ids"], o, c["pids"], k, fk, rk, metric), metric)
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_consequences_and_a_store_that_changes(ctx, metric):
    d, nprobe, k = 200, 4, 10
    c = make_case(d, 33, nprobe, metric, seed=9, sizes=SIZES)
    s, parent = _stores(ctx, c, d)
    q, pids = c["q"], c["pids"]
    assert np.diff(c["offsets"])[pids].sum(1).max() <= 640
    _eq(ctx.bin_scan(s, q, pids, k, 300, metric, rescore_k=300), ctx.bin_scan(s, q, pids, k, 300, metric), "rescore_k == fetch_k")
    _eq(ctx.bin_scan(s, q, pids, k, 640, metric, rescore_k=17), ctx.sq8_scan(s, q, pids, k, 17, metric), "fetch_k covers")
    covered = np.nonzero(np.diff(c["offsets"])[pids].sum(1) <= 448)[0]
    assert covered.shape[0] > 0
    _eq(ctx.bin_search(parent, s, q[covered], nprobe, k, 448, metric, rescore_k=448), ctx.search(parent, s, q[covered], nprobe, k, metric), "both cover")
    # rows leave a list, and a row that doubles column 0's range joins the last list of the arena: both mirrors are stale
    big = c["vecs"][:1].copy()
    big[0, 0] = c["vecs"][:, 0].max() + (c["vecs"][:, 0].max() - c["vecs"][:, 0].min())
    for change in (lambda: s.remove_ids(c["ids"][c["offsets"][6] + 10:c["offsets"][6] + 40]),
                   lambda: s.add_entries(7, np.array([100000], np.int64), big)):
        change()
        assert not s.bin_info()["valid"] and not s.sq8_info()["valid"]
        lists = [s.get_list(p) for p in range(len(SIZES))]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
        _eq(ctx.bin_scan(s, q, pids, k, 300, metric, rescore_k=17), reference(q, vecs, ids, offs, pids, k, 300, 17, metric), "changed")
        assert s.bin_info()["valid"] and s.sq8_info()["valid"]
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    lib, L2, DEV = ctx.lib, QK_METRIC_L2, QK_MEM_DEVICE
    ids = torch.full((17, 449), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 449), -7.0, device="cuda")

    def both(s, parent, q, pids, Q, k, fk, rk):
        a = lib.qk_bin_search_rescored(ctx.h, parent.h, s.h, q.data_ptr(), Q, 3, k, fk, rk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None)
        b = lib.qk_bin_scan_rescored(ctx.h, s.h, q.data_ptr(), Q, pids.data_ptr(), 3, k, fk, rk, L2, ids.data_ptr(), dist.data_ptr(), DEV, None)
        assert a == b
        return a

    for d in (64, 2112):
        c = make_case(d, 17, 3, "l2", seed=6, sizes=SIZES)
        s, parent = _stores(ctx, c, d)
        q, pids = torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda()
        if d == 2112:
            assert both(s, parent, q, pids, 17, 10, 64, 10) == UNSUPPORTED and b"d=2112 exceeds QK_SQ8_MAX_D" in lib.qk_last_error()
        else:
            for k, fk, rk, status in ((10, 64, 9, INVALID), (10, 64, 65, INVALID), (10, 4096, 449, UNSUPPORTED), (10, 4097, 10, UNSUPPORTED)):
                assert both(s, parent, q, pids, 17, k, fk, rk) == status, (k, fk, rk)
            assert both(s, parent, q, pids, 0, 10, 64, 10) == 0
            flat = lib.qk_bin_search_rescored(ctx.h, None, parent.h, q.data_ptr(), 17, 1, 10, 64, 10, L2, ids.data_ptr(), dist.data_ptr(), DEV, None)
            assert flat == UNSUPPORTED and b"flat index" in lib.qk_last_error()
            s.add_entries(5, np.array([424242], np.int64), np.full((1, d), np.nan, F))
            assert both(s, parent, q, pids, 17, 10, 64, 10) == UNSUPPORTED
            assert b"quantized search: list 5 holds a value that is not finite" in lib.qk_last_error()
            assert not s.bin_info()["valid"] and not s.sq8_info()["valid"]
        s.close()
        parent.close()
    torch.cuda.synchronize()
    assert (ids == -7).all() and (dist == -7.0).all()


def test_mirrors(tmp_path):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    g = torch.Generator().manual_seed(79)
    n, d, k, fk, rk, metric = 6000, 128, 10, 1000, 40, "l2"
    x = torch.randn(n, d, generator=g)
    q = x[torch.randint(0, n, (33,), generator=g)] + 0.05 * torch.randn(33, d, generator=g)
    built, bp = quake.QuakeIndex(), quake.IndexBuildParams()
    bp.nlist, bp.metric = 12, metric
    built.build(x, torch.randperm(n, generator=g) + 11, bp)
    built.save(str(tmp_path / "index"))
    loaded, loaded_cpp = quake.QuakeIndex(), qb.QuakeIndex()
    loaded.load(str(tmp_path / "index"))
    loaded_cpp.load(str(tmp_path / "index"))
    # the reference on the loaded index's own arena: its lists in order, the lists its coarse step picks
    lists = [loaded._store.get_list(p) for p in range(12)]
    vecs, vids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    pids = O.coarse(q.numpy(), loaded.parent._store.get_list(0)[0], None, 4, metric)[0]
    want = reference(q.numpy(), vecs, vids, offs, pids, k, fk, rk, metric)
    for mod, m in ((quake, loaded), (qb, loaded_cpp)):
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, k
        for xq in (q, q.cuda()):
            r = m.binary_search(xq, sp, fk, rescore_k=rk)
            _eq((r.ids, r.distances), want, mod.__name__)
        old, none = m.binary_search(q, sp, fk), m.binary_search(q, sp, fk, rescore_k=None)
        _eq((none.ids, none.distances), (old.ids, old.distances), "rescore_k=None")
        sp.recall_target = 0.9
        with pytest.raises(NotImplementedError):
            m.binary_search(q, sp, fk, rescore_k=rk)
