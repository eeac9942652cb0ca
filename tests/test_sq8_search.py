"""Quantized search on the device (qk_sq8_search / qk_sq8_scan; Context.sq8_search / sq8_scan; QuakeIndex.quantized_search in both
mirrors) against tests/sq8_yardstick.py: ids and distance bits."""
import numpy as np
import pytest
import torch

import oracle as O
import sq8_yardstick as SY
from quake_amd._lib import QuakeHipError
from quake_amd.capi import Context, Store

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17, 33, 300, 257]
BIG = 6  # the list query 0 lives in
A = np.float32(3.96875)  # 127 / 32: the planted extremes of column 0, which make the scale of both metrics 2^-5
S = np.float32(0.03125)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, tag):
    torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
    gi, gd = (o.cpu().numpy() if torch.is_tensor(o) else o for o in got[:2])
    want = tuple(o.cpu().numpy() if torch.is_tensor(o) else o for o in want[:2])
    assert (gi == want[0]).all(), (tag, "ids")
    assert (_bits(gd) == _bits(want[1])).all(), (tag, "distances")


def make_case(d, Q, nprobe, fetch_k, metric, seed):
    """8 lists of SIZES rows around their centroids, every value inside (-A, A); query 0 next to list BIG.  Planted for query 0: the
    rows that hold column 0's min and max, -A and A (codes -127 and 127; the scale is 2^-5 exactly); coordinates exactly halfway
    between two codes (2.5 and 3.5 scales: 2 and 4); a query coordinate outside the store's range (column 1; L2 clamps it); and,
    where the shape allows it (fetch_k + 1 <= 65 probed rows; d <= 200, beyond which a step inside a cell is lost in the float32 key), a block of fetch_k + 1 rows with equal codes and the best approximate keys
    of the query, bit-equal under different ids but for column 0, where they move inside one code cell: the last candidate in
    arena order gets the best exact key of the candidates, the row behind it -- the first one outside -- a better one still
    (search() would return it first; quantized search must not return it)."""
    rng = np.random.default_rng(seed)
    cent = (0.6 * rng.standard_normal((len(SIZES), d))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    lists = np.repeat(np.arange(len(SIZES)), SIZES)
    vecs = np.clip(cent[lists] + 0.3 * rng.standard_normal((lists.shape[0], d)), -3.5, 3.5).astype(np.float32)
    ids = rng.permutation(lists.shape[0]).astype(np.int64) + 7
    q = (cent[rng.integers(0, len(SIZES), Q)] + 0.3 * rng.standard_normal((Q, d))).astype(np.float32)
    q[0] = cent[BIG] + 0.15 * rng.standard_normal(d).astype(np.float32)
    big = np.arange(offsets[BIG], offsets[BIG + 1])
    vecs[big[4], 0], vecs[big[5], 0], vecs[big[6], 0], vecs[big[7], 0] = A, -A, 2.5 * S, 3.5 * S
    q[0, 1] = 9.0
    q[0, 0] = abs(q[0, 0]) + 0.5
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    m, s = SY.params(vecs, metric)
    rows0 = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[0]])
    free = rows0[~np.isin(rows0, big[4:8])]
    if BIG in pids[0] and fetch_k + 1 <= min(65, free.shape[0]) and d <= 200:
        key = SY.keys(SY.query_codes(q[:1], m, s, metric)[0], SY.codes(vecs[free], m, s), metric)
        block = np.sort(free[np.argsort(key, kind="stable")[:fetch_k + 1]])
        v0 = np.clip((3.0 if metric == "ip" else 1.0) * q[0], -3.5, 3.5).astype(np.float32)
        v0[0] = S * np.rint(v0[0] / S)   # a cell's centre (column 0's centre is 0); the rows move inside the cell
        vecs[block] = v0
        vecs[block[-2], 0] += np.float32(0.3) * S
        vecs[block[-1], 0] += np.float32(0.4) * S
        if metric == "l2":
            q[0, 0] = v0[0] + np.float32(0.45) * S
        m, s = SY.params(vecs, metric)
        key = SY.keys(SY.query_codes(q[:1], m, s, metric)[0], SY.codes(vecs[rows0], m, s), metric)
        assert (np.sort(rows0[np.lexsort((rows0, key))[:fetch_k + 1]]) == block).all() and np.unique(key[np.isin(rows0, block)]).shape[0] == 1
        ex = O.pair_values(q[:1], vecs[block], metric)[0] * (-1 if metric == "ip" else 1)
        assert ex[-1] < ex[-2] and (ex[-2] < ex[:-2]).all()
        assert (pids == O.coarse(q, cent, None, nprobe, metric)[0]).all()
    assert s == S and m[0] == 0
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


# (d, Q, nprobe, k, fetch_k): every value of the issue's lists, not their product
SHAPES = [(40, 1, 1, 1, 1), (40, 17, 4, 10, 64), (64, 33, 4, 10, 10), (64, 17, 1, 10, 64), (128, 33, 1, 10, 10), (128, 17, 4, 100, 448),
          (200, 33, 4, 10, 64), (200, 1, 1, 1, 1), (768, 17, 4, 10, 64), (768, 33, 1, 100, 448), (2048, 17, 4, 100, 448), (2048, 1, 1, 10, 10)]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_Q%d_np%d_k%d_f%d" % s)
def test_against_the_yardstick(ctx, shape, metric):
    d, Q, nprobe, k, fk = shape
    c = make_case(d, Q, nprobe, fk, metric, seed=2300 + d + Q + fk)
    want = SY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, metric)
    s, parent = _stores(ctx, c, d)
    assert not s.sq8_info()["valid"]
    before = s.device_bytes()
    _eq(ctx.sq8_search(parent, s, c["q"], nprobe, k, fk, metric), want, "search, host")
    assert ctx.last_scan_kernel() == "k_scan (int8 codes)"
    info = s.sq8_info()
    assert info["valid"] and info["scale"] == S and info["bytes"] == s.device_bytes() - before and info["bytes"] % (64 * ((d + 63) // 64) + 4) == 0
    _eq(ctx.sq8_scan(s, torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["pids"]).cuda(), k, fk, metric), want, "scan, device")
    s.sq8_drop()
    assert s.sq8_info() == {"valid": False, "bytes": 0, "scale": 0.0} and s.device_bytes() == before
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fetch_k_covers_the_probed_rows_and_the_store_changes(ctx, metric):
    d = 40
    c = make_case(d, 17, 4, 448, metric, seed=9)
    s, parent = _stores(ctx, c, d)
    probed = (c["offsets"][1:] - c["offsets"][:-1])[c["pids"]].sum(1)
    sel = np.nonzero(probed <= 448)[0]
    assert sel.shape[0] > 0
    _eq(ctx.sq8_search(parent, s, c["q"][sel], 4, 100, 448, metric), ctx.search(parent, s, c["q"][sel], 4, 100, metric), "covers")
    # rows leave and a row that doubles column 0's range arrives: the scale changes, a stale mirror would show
    _eq(ctx.sq8_scan(s, c["q"], c["pids"], 10, 64, metric), SY.case(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], 10, 64, metric), "before")
    gone = c["ids"][c["offsets"][BIG] + 10:c["offsets"][BIG] + 40]
    new_x = (c["q"][:8] * np.float32(0.5)).astype(np.float32)
    new_x[0, 0] = 3 * A
    s.remove_ids(gone)
    s.add_entries(5, np.arange(8, dtype=np.int64) + 100000, new_x)
    assert not s.sq8_info()["valid"]
    lists = [s.get_list(p) for p in range(len(SIZES))]
    vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    assert SY.params(vecs, metric)[1] != S
    _eq(ctx.sq8_scan(s, c["q"], c["pids"], 10, 64, metric), SY.case(c["q"], vecs, ids, offs, c["pids"], 10, 64, metric, cut_in_one_list=True), "after")
    s.close()
    parent.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    d = 40
    c = make_case(d, 17, 4, 64, "l2", seed=5)
    s, parent = _stores(ctx, c, d)
    lib, q = ctx.lib, torch.from_numpy(c["q"]).cuda()
    ids = torch.full((17, 10), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((17, 10), -7.0, device="cuda")

    def call(store, par, k, fk, nq=17):
        return lib.qk_sq8_search(ctx.h, par.h if par is not None else None, store.h, q.data_ptr(), nq, 4, k, fk, 1, ids.data_ptr(), dist.data_ptr(), 1, None)

    flat = Store(ctx, d)
    flat.build_csr(np.array([0, 40], np.int64), np.arange(40, dtype=np.int64), c["vecs"][-40:])
    bad = c["vecs"].copy()
    bad[c["offsets"][3] + 2, 5] = np.nan
    nan_store = Store(ctx, d)
    nan_store.build_csr(c["offsets"], c["ids"], bad)
    wide = Store(ctx, 2112)
    INVALID, UNSUPPORTED = 1, 4
    for args, code in (((s, parent, 0, 64), INVALID), ((s, parent, 10, 9), INVALID), ((s, parent, 10, 449), UNSUPPORTED),
                       ((wide, None, 1, 1, 0), UNSUPPORTED), ((flat, None, 10, 20), UNSUPPORTED), ((nan_store, parent, 10, 64), UNSUPPORTED)):
        assert call(*args) == code, args[2:]
    torch.cuda.synchronize()
    assert (ids == -7).all() and (dist == -7.0).all()
    with pytest.raises(QuakeHipError, match="list 3 holds a value that is not finite"):
        ctx.sq8_search(parent, nan_store, c["q"], 4, 10, 64, "l2")
    assert call(s, parent, 10, 64, 0) == 0  # Q == 0
    for st in (flat, wide, nan_store, s, parent):
        st.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mirrors(metric, tmp_path):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    g = torch.Generator().manual_seed(77)
    n, d, k, fk = 3000, 40, 10, 64
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
    lists = [idx._store.get_list(p) for p in range(12)]
    vecs, vids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
    pids = idx._ctx.coarse(idx.parent._store, q.numpy(), 4, metric, values=False)[0]
    want = SY.case(q.numpy(), vecs, vids, offs, pids, k, fk, metric)
    for mod, m in ((quake, idx), (qb, loaded)):
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, k
        for xq in (q, q.cuda()):
            r = m.quantized_search(xq, sp, fk)
            assert r.ids.is_cuda == xq.is_cuda
            _eq((r.ids, r.distances), want, (mod.__name__, xq.is_cuda))
        sp.recall_target = 0.9
        with pytest.raises(NotImplementedError, match="recall_target"):
            m.quantized_search(q, sp, fk)
