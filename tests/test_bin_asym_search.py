"""Asymmetric binary search on the device (qk_bin_search_asym / qk_bin_scan_asym; Context.bin_search / bin_scan with asymmetric=True;
no index-level form) against the definition (include/quake_hip.h, "binary search, asymmetric")
written out in numpy below: ids and distance bits.  Centres and bits are tests/bin_yardstick.py's, the int8 stage is
tests/sq8_yardstick.py's, the exact finish goes through the oracle as bin_yardstick.case ends.  The corpus, the comparison and the
context are tests/test_bin_search.py's."""
import numpy as np
import pytest
import torch

import bin_yardstick as BY
import oracle as O
import sq8_yardstick as SY
from quake_amd._lib import QK_MEM_HOST, QK_METRIC_IP, QK_METRIC_L2
from test_bin_search import UNSUPPORTED, _eq, _stores, ctx, make_case  # noqa: F401 (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [0, 1, 15, 33, 3300, 257, 700, 40]  # list 4: more than three walk steps of 1024 rows
BLOCK = 48  # identical rows planted in list 4
KERNEL = "k_bin_select_asym (sign codes)"


def factors(vecs, m):
    """(r2, w) of every row: four chains over the columns j = g (mod 4), every operation rounded to float32"""
    v = vecs - m
    a, l = np.zeros((vecs.shape[0], 4), F), np.zeros((vecs.shape[0], 4), F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(vecs.shape[1]):
            a[:, j % 4] = a[:, j % 4] + v[:, j] * v[:, j]
            l[:, j % 4] = l[:, j % 4] + np.abs(v[:, j])
        r2, l1 = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3]), (l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3])
        w = np.where(l1 == 0, F(0), r2 / l1)
    assert r2.dtype == w.dtype == F
    return r2, w


def query(q, m):
    """(lo, delta, u [d]) of one query"""
    with np.errstate(invalid="ignore", over="ignore"):
        qp = q - m
        qp = np.where(np.isfinite(qp) & (qp != 0), qp, F(0))
        lo, hi = qp.min(), qp.max()
        delta = (hi - lo) / F(15)
        delta = F(1) if delta == 0 else delta
        u = np.clip(np.nan_to_num(np.rint((qp - lo) / delta), nan=0.0), 0, 15).astype(np.int64)
    assert lo.dtype == delta.dtype == F
    return lo, delta, u


def images(q, m, bx, r2, w, metric):
    """the key images of one query against rows with bits bx and factors (r2, w)"""
    lo, delta, u = query(q, m)
    t, p = 2 * (bx.astype(np.int64) @ u) - u.sum(), 2 * bx.sum(1, dtype=np.int64) - q.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        e = delta * t.astype(F) + lo * p.astype(F)
        key = -(w * e) if metric == "ip" else r2 - F(2) * (w * e)
    assert key.dtype == F
    b = key.view(np.uint32)
    return np.where(np.isnan(key), np.uint32(0xFFFFFFFF), np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000)))


def reference(q, vecs, ids, offsets, pids, k, fetch_k, rescore_k, metric):
    """expected (ids [Q, k], dist [Q, k]), and per query the sorted images of its probed rows"""
    q, vecs, ids = np.ascontiguousarray(q, F), np.ascontiguousarray(vecs, F), np.asarray(ids, np.int64)
    m = BY.params(vecs, metric)
    bx, (r2, w) = BY.codes(vecs, m), factors(vecs, m)
    if rescore_k:
        m8, s8 = SY.params(vecs, metric)
        cx, cq = SY.codes(vecs, m8, s8), SY.query_codes(q, m8, s8, metric)
    out, imgs = [], []
    for qi in range(q.shape[0]):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1]) for p in pids[qi] if p >= 0] + [np.zeros(0, np.int64)]).astype(np.int64)
        img = images(q[qi], m, bx[rows], r2[rows], w[rows], metric)
        imgs.append(np.sort(img))
        rows = rows[np.lexsort((rows, img))[:fetch_k]]
        if rescore_k:
            rows = rows[np.lexsort((rows, SY.keys(cq[qi], cx[rows], metric)))[:rescore_k]]
        # (the exact finish: bin_yardstick.case over the survivors as a store of their own, with a fetch_k that takes them all)
        out.append(BY.case(q[qi:qi + 1], vecs[rows], ids[rows], np.array([0, rows.shape[0]]), np.zeros((1, 1), np.int64), k, max(rows.shape[0], 1), metric))
    return (np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])), imgs


def asym_case(d, Q, nprobe, metric, seed):
    """test_bin_search's corpus with BLOCK identical rows in the middle of list 4 and query 3 on top of them (IP: a long vector, so
    that the block leads the query's ranking under either metric).  scan_pids: the last pid of query 0 is -1, the first of query 1
    the empty list"""
    c = make_case(d, Q, nprobe, metric, seed=seed, sizes=SIZES)
    o = c["offsets"][4] + 1000
    c["vecs"][o:o + BLOCK] = c["vecs"][o] * F(1.5 if metric == "ip" else 1.0)
    c["q"][3] = c["vecs"][o]
    c["pids"] = O.coarse(c["q"], c["cent"], None, nprobe, metric)[0]
    assert (c["pids"][3] == 4).any()
    assert nprobe == 1 or (np.diff(c["offsets"][c["pids"]], axis=1) < 0).any()  # pids that are not in arena order
    c["scan_pids"] = c["pids"].copy()
    c["scan_pids"][0, -1], c["scan_pids"][1, 0] = -1, 0
    return c


# (d, Q, nprobe, k, fetch_k, rescore_k)
SHAPES = [(40, 9, 1, 1, 1, 0), (128, 9, 3, 10, 10, 0), (200, 9, 3, 10, 40, 0), (264, 9, 3, 10, 40, 17), (128, 9, 1, 10, 300, 0),
          (200, 4, 4, 100, 4096, 448)]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_Q%d_np%d_k%d_f%d_r%d" % s)
def test_against_the_definition(ctx, shape, metric):
    d, Q, nprobe, k, fk, rk = shape
    c = asym_case(d, Q, nprobe, metric, seed=2900 + d + fk)
    want, imgs = reference(c["q"], c["vecs"], c["ids"], c["offsets"], c["pids"], k, fk, rk, metric)
    probed = np.array([i.shape[0] for i in imgs])
    assert probed[3] > 3 * 1024                            # every walk of query 3 crosses step boundaries
    assert fk >= BLOCK or imgs[3][fk - 1] == imgs[3][fk]   # equal images on both sides of the cut: the tie rule decides
    assert fk < 300 or ((probed < fk) & (probed > 0)).any()  # fewer probed rows than fetch_k: padding
    s, parent = _stores(ctx, c, d)
    assert not s.bin_asym_info()["valid"]
    before = s.device_bytes()
    _eq(ctx.bin_search(parent, s, c["q"], nprobe, k, fk, metric, rescore_k=rk or None, asymmetric=True), want, "search, host")
    assert ctx.last_scan_kernel() == KERNEL + (" + k_sq8_rerank (int8 codes)" if rk else "")
    info = s.bin_asym_info()
    assert info["valid"] and info["bytes"] % 128 == 0 and info["bytes"] >= 8 * sum(SIZES)
    assert s.device_bytes() - before == info["bytes"] + s.bin_info()["bytes"] + (s.sq8_info()["bytes"] if rk else 0)
    want_scan = reference(c["q"], c["vecs"], c["ids"], c["offsets"], c["scan_pids"], k, fk, rk, metric)[0]
    qd, pd = torch.from_numpy(c["q"]).cuda(), torch.from_numpy(c["scan_pids"]).cuda()
    _eq(ctx.bin_scan(s, qd, pd, k, fk, metric, rescore_k=rk or None, asymmetric=True), want_scan, "scan, device")
    s.bin_drop()
    assert not s.bin_asym_info()["valid"] and s.bin_asym_info()["bytes"] == 0
    s.close()
    parent.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_identities_and_a_store_that_changes(ctx, metric):
    d, nprobe, k = 200, 3, 10
    c = asym_case(d, 9, nprobe, metric, seed=31)
    s, parent = _stores(ctx, c, d)
    q, pids = np.ascontiguousarray(c["q"]), np.ascontiguousarray(c["pids"])
    sel = np.nonzero(np.diff(c["offsets"])[pids].sum(1) <= 4096)[0]
    assert sel.shape[0] > 1
    _eq(ctx.bin_search(parent, s, q[sel], nprobe, k, 4096, metric, asymmetric=True), ctx.search(parent, s, q[sel], nprobe, k, metric), "covers")
    today = ctx.bin_scan(s, q, pids, k, 40, metric)
    _eq(ctx.bin_scan(s, q, pids, k, 40, metric, asymmetric=False), today, "asymmetric=False")
    assert ctx.last_scan_kernel() == "k_bin_select (sign codes)"
    _eq(today, BY.case(q, c["vecs"], c["ids"], c["offsets"], pids, k, 40, metric), "today's call")
    # rows leave a list, and a row that doubles column 0's range joins the last list of the arena: mirror and factors are stale
    big = c["vecs"][:1].copy()
    big[0, 0] = c["vecs"][:, 0].max() + (c["vecs"][:, 0].max() - c["vecs"][:, 0].min())
    for change in (lambda: s.remove_ids(c["ids"][c["offsets"][4] + 990:c["offsets"][4] + 1020]),
                   lambda: s.add_entries(7, np.array([100000], np.int64), big)):
        change()
        assert not s.bin_asym_info()["valid"]
        lists = [s.get_list(p) for p in range(len(SIZES))]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], d)
        _eq(ctx.bin_scan(s, q, pids, k, 40, metric, asymmetric=True), reference(q, vecs, ids, offs, pids, k, 40, 0, metric)[0], "changed")
        assert s.bin_asym_info()["valid"]
    # a row whose centred squared norm overflows: no factors, by name, nothing written
    s.add_entries(5, np.array([424242], np.int64), np.full((1, d), 3e38, F))
    out = np.full((9, k), -7, np.int64)
    rc = ctx.lib.qk_bin_scan_asym(ctx.h, s.h, q.ctypes.data, 9, pids.ctypes.data, nprobe, k, 40, 0, QK_METRIC_L2 if metric == "l2" else QK_METRIC_IP,
                                  out.ctypes.data, None, QK_MEM_HOST, None)
    # (L2: the value moves column 0's centre to 1.5e38, so every row overflows and list 1 is the first that holds one)
    bad = 1 if metric == "l2" else 5
    assert rc == UNSUPPORTED and b"binary search, asymmetric: list %d holds a row whose norm factors are not finite" % bad in ctx.lib.qk_last_error()
    assert (out == -7).all() and not s.bin_asym_info()["valid"]
    s.close()
    parent.close()

