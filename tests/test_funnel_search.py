"""Funnel search on the device (qk_funnel_search / qk_funnel_scan; Context.funnel_search / funnel_scan; QuakeIndex.funnel_search in
both mirrors) against tests/funnel_yardstick.py: ids and distance bits."""
import numpy as np
import pytest
import torch

import funnel_yardstick as FY
import oracle as O
from quake_amd._lib import QuakeHipError
from quake_amd.capi import Context, Store

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17, 33, 300, 257]
BIG = 6  # the list query 0 lives in


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, tag):
    torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
    gi, gd = (o.cpu().numpy() if torch.is_tensor(o) else o for o in got[:2])
    want = tuple(o.cpu().numpy() if torch.is_tensor(o) else o for o in want[:2])
    assert (gi == want[0]).all(), (tag, "ids")
    assert (_bits(gd) == _bits(want[1])).all(), (tag, "distances")


def _rank(q0, vecs, offsets, pids0, dp, metric):
    """rows of query 0's probed lists, best prefix key first"""
    n = int(sum(offsets[p + 1] - offsets[p] for p in pids0))
    r, _ = O.batched_serial_scan(q0[None, :dp].copy(), np.ascontiguousarray(vecs[:, :dp]), np.arange(vecs.shape[0], dtype=np.int64), offsets,
                                 pids0[None, :].copy(), n, metric)
    return r[0][r[0] >= 0]


def make_case(d, dp, Q, nprobe, fetch_k, metric, seed):
    """8 lists of SIZES rows around their centroids; query 0 next to list BIG.  Planted for query 0: a row with a NaN in the prefix, a
    row with a NaN only in the tail and a top prefix key, an id stored twice, two ids with bit-equal rows, a group of four rows that
    share their prefix and differ in the tail, the candidate of the worst prefix rank with the best exact key, and the row just
    outside the candidates with a better exact key still (search() would return it first; funnel search must not return it)."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((len(SIZES), d)).astype(np.float32) * 2
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    lists = np.repeat(np.arange(len(SIZES)), SIZES)
    vecs = (cent[lists] + rng.standard_normal((lists.shape[0], d))).astype(np.float32)
    ids = rng.permutation(lists.shape[0]).astype(np.int64) + 7
    q = (cent[rng.integers(0, len(SIZES), Q)] + rng.standard_normal((Q, d))).astype(np.float32)
    q[0] = cent[BIG] + 0.5 * rng.standard_normal(d).astype(np.float32)
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    big = np.arange(offsets[BIG], offsets[BIG + 1])
    tail = dp < d
    near = (3.0 if metric == "ip" else 1.0) * q[0, :dp]
    vecs[big[0], 3] = np.nan
    if tail:
        vecs[big[1], :dp] = near
        vecs[big[1], d - 1] = np.nan
    ids[big[3]] = ids[big[2]]
    if BIG in pids[0]:
        rk = _rank(q[0], vecs, offsets, pids[0], dp, metric)
        vecs[rk[-1]] = vecs[rk[2]]                       # bit-equal rows under two ids, adjacent prefix ranks
        rk = _rank(q[0], vecs, offsets, pids[0], dp, metric)
        vecs[rk[-4:-1], :dp] = vecs[rk[12], :dp]          # the group that shares its prefix
        rk = _rank(q[0], vecs, offsets, pids[0], dp, metric)
        if tail and fetch_k < rk.shape[0]:
            best = (50.0 if metric == "ip" else 1.0) * q[0, dp:]
            vecs[rk[fetch_k - 1], dp:] = best + (0.0 if metric == "ip" else 1.0)
            vecs[rk[fetch_k], dp:] = (2.0 if metric == "ip" else 1.0) * best
    return dict(cent=cent, vecs=vecs, ids=ids, offsets=offsets, q=q, pids=pids)


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


# (d, prefix_dim, Q, nprobe, k, fetch_k): every value of the issue's lists, not their product; 700 > the rows any query probes
SHAPES = [(48, 16, 1, 1, 1, 1), (48, 16, 17, 4, 10, 64), (40, 16, 33, 4, 10, 10), (40, 40, 17, 4, 10, 64), (128, 32, 33, 1, 10, 64),
          (128, 64, 17, 4, 100, 448), (128, 128, 33, 4, 100, 448), (768, 256, 17, 4, 10, 64), (768, 256, 1, 1, 10, 10),
          (4096, 256, 17, 4, 100, 448), (4096, 256, 33, 1, 1, 1), (128, 32, 17, 4, 10, 448)]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_p%d_Q%d_np%d_k%d_f%d" % s)
def test_against_the_yardstick(ctx, shape, metric):
    d, dp, Q, nprobe, k, fk = shape
    c = make_case(d, dp, Q, nprobe, fk, metric, seed=1100 + d + dp + Q + fk)
    want = FY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, dp, metric)
    s, parent = _stores(ctx, c, d)
    _eq(ctx.funnel_search(parent, s, c["q"], nprobe, k, fk, dp, metric), want, "search, host")
    assert ctx.last_scan_kernel() == "k_scan (prefix)"
    _eq(ctx.funnel_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, dp, metric), want, "scan, device")
    if dp == d:  # the same as search(), bit for bit
        _eq(ctx.funnel_search(parent, s, c["q"], nprobe, k, fk, dp, metric), ctx.search(parent, s, c["q"], nprobe, k, metric), "prefix_dim == d")
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fetch_k_covers_the_probed_rows_and_the_store_changes(ctx, metric):
    d, dp = 48, 16
    c = make_case(d, dp, 17, 4, 448, metric, seed=9)
    s, parent = _stores(ctx, c, d)
    probed = (c["offsets"][1:] - c["offsets"][:-1])[c["pids"]].sum(1)
    k = 100
    sel = np.nonzero(probed <= 448)[0]
    assert sel.shape[0] > 0
    _eq(ctx.funnel_search(parent, s, c["q"][sel], 4, k, 448, dp, metric), ctx.search(parent, s, c["q"][sel], 4, k, metric), "covers")
    # the rows move between two calls: stale prefix norms would show in the second
    _eq(ctx.funnel_scan(s, c["q"], c["pids"], 10, 64, dp, metric), FY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], 10, 64, dp, metric), "before")
    lists = [(c["vecs"][c["offsets"][p]:c["offsets"][p + 1]], c["ids"][c["offsets"][p]:c["offsets"][p + 1]]) for p in range(len(SIZES))]
    gone = lists[BIG][1][10:40]
    new_x = (c["q"][:8] * np.float32(1.25)).astype(np.float32)
    new_i = np.arange(8, dtype=np.int64) + 100000
    s.remove_ids(gone)
    s.add_entries(5, new_i, new_x)
    keep = ~np.isin(lists[BIG][1], gone)
    lists[BIG] = (lists[BIG][0][keep], lists[BIG][1][keep])
    lists[5] = (np.concatenate([lists[5][0], new_x]), np.concatenate([lists[5][1], new_i]))
    vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    _eq(ctx.funnel_scan(s, c["q"], c["pids"], 10, 64, dp, metric), FY.case(c["q"], vecs, ids, offs, c["pids"], 10, 64, dp, metric), "after")
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    d = 48
    c = make_case(d, 16, 17, 4, 64, "l2", seed=5)
    s, parent = _stores(ctx, c, d)
    lib, q = ctx.lib, torch.from_numpy(c["q"]).cuda()
    ids = torch.full((17, 10), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 10), -7.0, device="cuda")

    def call(store, par, k, fk, dp):
        return lib.qk_funnel_search(ctx.h, par.h if par is not None else None, store.h, q.data_ptr(), 17, 4, k, fk, dp, 1, ids.data_ptr(),
                                    dist.data_ptr(), 1, None)

    flat = Store(ctx, d)
    flat.build_csr(np.array([0, 40], np.int64), np.arange(40, dtype=np.int64), c["vecs"][-40:])
    INVALID, UNSUPPORTED = 1, 4
    for args, code in (((s, parent, 10, 64, 8), INVALID), ((s, parent, 10, 64, 24), INVALID), ((s, parent, 10, 64, 64), INVALID),
                       ((s, parent, 0, 64, 16), INVALID), ((s, parent, 10, 9, 16), INVALID), ((s, parent, 10, 449, 16), UNSUPPORTED),
                       ((flat, None, 10, 20, 16), UNSUPPORTED)):
        assert call(*args) == code, args[2:]
    wide = Store(ctx, 2048)
    assert lib.qk_funnel_search(ctx.h, None, wide.h, q.data_ptr(), 0, 4, 1, 1, 1040, 1, ids.data_ptr(), dist.data_ptr(), 1, None) == UNSUPPORTED
    assert (ids == -7).all() and (dist == -7.0).all()
    with pytest.raises(QuakeHipError):
        ctx.funnel_search(parent, s, c["q"], 4, 10, 9, 16, "l2")
    for st in (flat, wide, s, parent):
        st.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(metric, tmp_path):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    g = torch.Generator().manual_seed(77)
    n, d, dp, k, fk = 3000, 48, 16, 10, 64
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = x[torch.randint(0, n, (17,), generator=g)] + 0.05 * torch.randn(17, d, generator=g)
    idx = quake.QuakeIndex()
    bp = quake.IndexBuildParams()
    bp.nlist, bp.metric = 12, metric
    idx.build(x, ids, bp)
    idx.save(str(tmp_path / "index"))
    loaded = qb.QuakeIndex()
    loaded.load(str(tmp_path / "index"))
    st = idx._store
    lists = [st.get_list(p) for p in range(12)]
    vecs, vids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    pids = idx._ctx.coarse(idx.parent._store, q.numpy(), 4, metric, values=False)[0]
    want = FY.case(q.numpy(), vecs, vids, offs, pids, k, fk, dp, metric)
    for mod, m in ((quake, idx), (qb, loaded)):
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, k
        for xq in (q, q.cuda()):
            r = m.funnel_search(xq, sp, dp, fk)
            assert r.ids.is_cuda == xq.is_cuda
            _eq((r.ids, r.distances), want, (mod.__name__, xq.is_cuda))
        sp.recall_target = 0.9
        with pytest.raises(NotImplementedError, match="recall_target"):
            m.funnel_search(q, sp, dp, fk)
