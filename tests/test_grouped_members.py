"""Grouped search with members (qk_search_grouped_n / qk_scan_grouped_n; Context.search_grouped / scan_grouped with group_size;
QuakeIndex.grouped_search(..., group_size) in both mirrors): the group_size best rows of each of the k best groups.

Every comparison is bit for bit -- ids, the uint32 view of the distances, groups -- against tests/grouped_members_yardstick.py
(pinned on the CPU by tests/test_grouped_members_oracle.py).  No assertion reads a clock.  Every test asserts on its own inputs that
the situation it is about occurs."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import filter_yardstick as FY
import grouped_members_yardstick as GMY
import grouped_yardstick as GY
import nonfinite_yardstick as NFY
import oracle as O
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def _stores(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def _np(a):
    if torch.is_tensor(a):
        if a.is_cuda:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        return a.cpu().numpy()
    return np.asarray(a)


def _eq(got, want, tag):
    np.testing.assert_array_equal(_np(got[0]), want[0], err_msg="ids " + str(tag))
    np.testing.assert_array_equal(_np(got[1]).view(np.uint32), np.asarray(want[1]).view(np.uint32), err_msg="dist " + str(tag))
    np.testing.assert_array_equal(_np(got[2]), want[2], err_msg="groups " + str(tag))


def _attr(s, ids, vals):
    from quake_amd.capi import Attr
    a = Attr(s)
    a.set(np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(vals, np.int64))
    return a


def _short_and_long(want, counts, m):
    """(a live group with padding among its members, a returned group with more candidates than m) in an expected result"""
    wi, _, wg = want
    short = bool(((wi[:, :, 0] >= 0) & (wi[:, :, m - 1] < 0)).any()) if m > 1 else False
    more = any(counts[i].get(int(g), 0) > m for i in range(wi.shape[0]) for g, h in zip(wg[i], wi[i, :, 0]) if h >= 0)
    return short, more


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


CARDS = ("one", "n8", "own")


def _card_values(ids, card):
    """the group of every id: one group for all, about n / 8 groups scattered over the int64 range, every id its own group"""
    if card == "one":
        return np.full(ids.shape[0], 42, np.int64)
    if card == "n8":
        return (ids % (ids.shape[0] // 8)) * 1000003 - 7
    return ids * 3 - 1000


@pytest.fixture(scope="module")
def corpora(ctx):
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c = RY.corpus(d, 64, 20000, metric, seed=500 + d + (1 if metric == "ip" else 0))
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and ((sizes > 0) & (sizes < 16)).sum() >= 1 and (sizes % 16 != 0).any()
            s, parent = _stores(ctx, c)
            cols = {card: _attr(s, c["ids"], _card_values(c["ids"], card)) for card in CARDS}
            cache[(d, metric)] = (c, s, parent, cols)
        return cache[(d, metric)]

    yield get
    for c, s, p, cols in cache.values():
        for a in cols.values():
            a.close()
        s.close()
        p.close()


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[64, 128], nprobe=[1, 4, 64], Q=[1, 17, 33], k=[1, 10, 449, "over"], m=[1, 2, 3, 16],
            card=list(CARDS), mem=["host", "device"], entry=["search_grouped", "coarse+scan_grouped"])
K_OVER = 3000  # more than the 2500 groups of "n8" (and than the one of "one")


def _expects_short(c):   # every row its own group: members 1 .. m - 1 of every live group are padding
    return c["card"] == "own" and c["m"] > 1


def _expects_more(c):    # one group holds every candidate of four or more probed lists: far more than m
    return c["card"] == "one" and c["m"] in (2, 3) and c["nprobe"] >= 4


def _grid():
    """every value of every axis, in combinations a fixed seed decides (the pruning of tests/test_grouped_search.py)"""
    rng = np.random.default_rng(20250907)
    n = 24
    cols = {}
    for name, vals in AXES.items():
        seq = []
        while len(seq) < n:
            seq += [vals[i] for i in rng.permutation(len(vals))]
        cols[name] = seq[:n]
    cases = [{name: cols[name][i] for name in AXES} for i in range(n)]
    for name, vals in AXES.items():
        assert {c[name] for c in cases} == set(vals), name
    # the grid holds groups with fewer candidates than m (padding inside a live group) and groups with more: test_grid asserts
    # on those cases' own expected results that it happens
    assert any(_expects_short(c) for c in cases) and any(_expects_more(c) for c in cases)
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, case):
    c, s, parent, cols = corpora(case["d"], case["metric"])
    metric, nprobe, Q, card, m = case["metric"], case["nprobe"], case["Q"], case["card"], case["m"]
    k = K_OVER if case["k"] == "over" else case["k"]
    q = RY.queries(c, Q, seed=zlib.crc32(repr(sorted(case.items(), key=str)).encode()) % (1 << 30))
    pids = GY.probed(q, c["cent"], c["offsets"], nprobe, metric)
    vals = _card_values(c["ids"], card)
    want = GMY.scan(q, c["vecs"], c["ids"], c["offsets"], pids, k, m, metric, c["ids"], vals)
    assert want[0].shape == (Q, k, m) and want[2].shape == (Q, k)
    short, more = _short_and_long(want, GMY.group_counts(q, c["vecs"], c["ids"], c["offsets"], pids, metric, c["ids"], vals), m)
    if _expects_short(case):
        assert short
    if _expects_more(case):
        assert more
    if case["k"] == "over" and card != "own":
        assert (want[0][:, -1] == -1).all() and (want[0][:, 0, 0] >= 0).all()   # fewer groups than k: padded group slots
    dev = case["mem"] == "device"
    xq = torch.from_numpy(q).cuda() if dev else q
    if case["entry"] == "search_grouped":
        got = ctx.search_grouped(parent, s, xq, nprobe, k, metric, cols[card], group_size=m)
    else:
        gp, _ = ctx.coarse(parent, xq, nprobe, metric)
        got = ctx.scan_grouped(s, xq, gp, k, metric, cols[card], group_size=m)
    ctx.synchronize()
    assert ctx.last_scan_kernel() == "k_scan (grouped)"
    assert tuple(got[0].shape) == (Q, k, m) and tuple(got[1].shape) == (Q, k, m) and tuple(got[2].shape) == (Q, k)
    _eq(got, want, case)


# ---- 2. the identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_identities(ctx, corpora, metric):
    c, s, parent, cols = corpora(64, metric)
    q = RY.queries(c, 33, seed=201)
    xd = torch.from_numpy(q).cuda()
    ctx.set_timing(1)
    try:
        for card, nprobe, k in (("n8", 4, 10), ("one", 4, 3), ("own", 1, 449)):
            for xq in (q, xd):
                old = ctx.search_grouped(parent, s, xq, nprobe, k, metric, cols[card], timing=True)
                # m = 1 through the new entry: the same three arrays, the same passes
                new = ctx.search_grouped(parent, s, xq, nprobe, k, metric, cols[card], timing=True, group_size=1)
                assert tuple(new[0].shape) == (33, k, 1)
                _eq((_np(new[0])[:, :, 0], _np(new[1])[:, :, 0], new[2]), tuple(_np(a) for a in old[:3]), (card, "m = 1"))
                assert new[3]["n_items"] == old[3]["n_items"] == 1
                # member 0 at m = 16 is the old entry's row
                wide = ctx.search_grouped(parent, s, xq, nprobe, k, metric, cols[card], group_size=16)
                _eq((_np(wide[0])[:, :, 0], _np(wide[1])[:, :, 0], wide[2]), tuple(_np(a) for a in old[:3]), (card, "m = 16"))
            gp, _ = ctx.coarse(parent, q, nprobe, metric)
            old = ctx.scan_grouped(s, q, gp, k, metric, cols[card])
            new = ctx.scan_grouped(s, q, gp, k, metric, cols[card], group_size=1)
            _eq((new[0][:, :, 0], new[1][:, :, 0], new[2]), old, (card, "scan, m = 1"))
    finally:
        ctx.set_timing(0)
    # one group, k = 1, m = 16: the scan with k = 16 over the same lists
    gp, _ = ctx.coarse(parent, q, 4, metric)
    gi, gd, gg = ctx.scan_grouped(s, q, gp, 1, metric, cols["one"], group_size=16)
    si, sd = ctx.scan(s, q, gp, 16, metric)
    ctx.synchronize()
    np.testing.assert_array_equal(gi[:, 0, :], _np(si))
    np.testing.assert_array_equal(gd[:, 0, :].view(np.uint32), _np(sd).view(np.uint32))
    assert (gi >= 0).all() and (gg == 42).all()
    # every id its own group: member 0 is search(), the rest is padding
    gi, gd, gg = ctx.search_grouped(parent, s, q, 4, 10, metric, cols["own"], group_size=3)
    pi, pd = ctx.search(parent, s, q, 4, 10, metric)
    ctx.synchronize()
    np.testing.assert_array_equal(gi[:, :, 0], _np(pi))
    np.testing.assert_array_equal(gd[:, :, 0].view(np.uint32), _np(pd).view(np.uint32))
    assert (gi[:, :, 0] >= 0).all() and (gi[:, :, 1:] == -1).all()
    assert (gd[:, :, 1:] == (-np.inf if metric == "ip" else np.inf)).all()


# ---- 3. ties at the floor, ids beyond 2^32 -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_ids(ctx):
    """a small store whose ids lie beyond 2^40 (the column is in the sorted layout).  One vector sits under three ids of group
    1000001 -- rows t1, t2 in list 5, t3 in list 6; the ids agree in their low 32 bits -- and under a fourth id, t4 in list 7, of
    group 1000002.  Five ordinary rows belong to group 1000001 too."""
    c = RY.corpus(32, 12, 3000, "l2", seed=231)
    ids = c["ids"] + (1 << 40)
    off = c["offsets"]
    assert off[6] - off[5] > 60 and off[7] - off[6] > 30 and off[8] - off[7] > 10
    t1, t2, t3, t4 = off[5] + 3, off[5] + 40, off[6] + 20, off[7] + 1
    for t in (t2, t3, t4):
        c["vecs"][t] = c["vecs"][t1]
    ids[t1], ids[t2], ids[t3], ids[t4] = (1 << 42) + 9, (1 << 41) + 9, (1 << 40) + (1 << 33) + 9, (1 << 43) + 9
    assert np.unique(ids).shape[0] == ids.shape[0]
    c["ids"] = ids
    vals = ids % 50
    vals[[t1, t2, t3]] = 1000001
    vals[off[8]:off[8] + 5] = 1000001
    vals[t4] = 1000002
    s, parent = _stores(ctx, c)
    col = _attr(s, ids, vals)
    assert col.info()["layout"] == "sorted"
    yield dict(c=c, s=s, parent=parent, col=col, vals=vals, planted=(t1, t2, t3, t4))
    col.close()
    s.close()
    parent.close()


def test_ties_at_the_floor(ctx, big_ids):
    c, s, parent, col, vals = (big_ids[n] for n in ("c", "s", "parent", "col", "vals"))
    t1, t2, t3, t4 = big_ids["planted"]
    ids = c["ids"]
    q = np.ascontiguousarray(np.stack([c["vecs"][t1]] + list(RY.queries(c, 6, seed=232))))
    # the tie exists in the yardstick: the four copies are candidates at one canonical value, the smallest of the query
    lims, rows, val = GY.candidates(q, c["vecs"], ids, c["offsets"], GY.probed(q, c["cent"], c["offsets"], 12, "l2"), "l2")
    v0 = {int(r): v for r, v in zip(rows[lims[0]:lims[1]], val[lims[0]:lims[1]])}
    assert v0[int(t1)] == v0[int(t2)] == v0[int(t3)] == v0[int(t4)] == min(v0.values())
    assert len({int(ids[t]) & 0xFFFFFFFF for t in (t1, t2, t3, t4)}) == 1 and min(ids[[t1, t2, t3, t4]]) >= 1 << 32
    assert ids[t3] < ids[t2] < ids[t1] < ids[t4]
    w2 = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 12, 5, 2, "l2", ids, vals)
    w3 = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 12, 5, 3, "l2", ids, vals)
    # m = 2: the tie straddles the cut -- the two smallest ids are in, the third is out; m = 3: all three in id order
    assert list(w2[0][0, 0]) == [ids[t3], ids[t2]] and ids[t1] not in w2[0][0] and w2[2][0, 0] == 1000001
    assert list(w3[0][0, 0]) == [ids[t3], ids[t2], ids[t1]] and len(set(w3[1][0, 0].view(np.uint32).tolist())) == 1
    # the copy in the other group leads its own group, at the same distance
    assert w3[0][0, 1, 0] == ids[t4] and w3[2][0, 1] == 1000002 and w3[1][0, 1, 0] == w3[1][0, 0, 0] and w3[0][0, 1, 1] == -1
    for xq in (q, torch.from_numpy(q).cuda()):
        _eq(ctx.search_grouped(parent, s, xq, 12, 5, "l2", col, group_size=2), w2, "ties, m = 2")
        _eq(ctx.search_grouped(parent, s, xq, 12, 5, "l2", col, group_size=3), w3, "ties, m = 3")
    gp, _ = ctx.coarse(parent, q, 12, "l2")
    _eq(ctx.scan_grouped(s, q, np.ascontiguousarray(gp[:, ::-1]), 5, "l2", col, group_size=3), w3, "ties, lists reversed")


# ---- 4. hostile values -------------------------------------------------------------------------------------------------------------
def test_hostile_values(ctx, corpora):
    c, s, parent, cols = corpora(64, "l2")
    ids = c["ids"]
    # 4 extreme values and 400 values that agree in their low 40 bits, dealt round-robin: 404 groups, every one in every long list
    pool = np.concatenate([np.array([I64MIN, I64MAX, -1, 0], np.int64), np.arange(400, dtype=np.int64) * (1 << 40) + 12345])
    vals = pool[ids % pool.shape[0]]
    a = _attr(s, ids, vals)
    q = RY.queries(c, 17, seed=241)
    G = pool.shape[0]
    for k in (G - 1, G + 1):
        want = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 64, k, 3, "l2", ids, vals)
        assert (want[0][:, :min(k, G)] >= 0).all()    # every group has at least 3 rows among all lists: no padding inside
        if k == G + 1:
            assert (want[0][:, G] == -1).all()
            for v in (I64MIN, I64MAX, -1, 0):
                assert (want[2][:, :G] == v).sum(axis=1).min() == 1
        _eq(ctx.search_grouped(parent, s, q, 64, k, "l2", a, group_size=3), want, ("hostile", k))
    # one list: the slot-T group (-1) among groups with one or two candidates
    want = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 1, 449, 3, "l2", ids, vals)
    assert (want[2][want[0][:, :, 0] >= 0] == -1).any()
    _eq(ctx.search_grouped(parent, s, q, 1, 449, "l2", a, group_size=3), want, ("hostile", "nprobe 1"))
    a.close()


# ---- 5. rows without a value, the sorted layout ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["table", "sorted"])
def test_rows_without_value(ctx, corpora, big_ids, layout):
    if layout == "table":
        c, s, parent, _ = corpora(64, "l2")
    else:
        c, s, parent = big_ids["c"], big_ids["s"], big_ids["parent"]
    ids, off = c["ids"], c["offsets"]
    sizes = np.diff(off)
    bare = int(np.argsort(sizes)[-3])          # a long list none of whose ids gets a value
    in_bare = np.zeros(ids.shape[0], bool)
    in_bare[off[bare]:off[bare + 1]] = True
    has = (ids % 2 == 0) & ~in_bare
    vals = ids % 97
    a = _attr(s, ids[has], vals[has])
    assert a.info()["layout"] == layout
    q = RY.queries(c, 17, seed=251)
    q[0] = c["cent"][bare]
    for nprobe, k in ((1, 10), (4, 120)):
        want = GMY.search(q, c["cent"], c["vecs"], ids, off, nprobe, k, 3, "l2", ids[has], vals[has])
        if nprobe == 1:
            assert GY.probed(q[:1], c["cent"], off, 1, "l2")[0, 0] == bare and (want[0][0] == -1).all()   # nothing but padding
            assert (want[0][1:, 0, 0] >= 0).any()
        got = ctx.search_grouped(parent, s, q, nprobe, k, "l2", a, group_size=3)
        _eq(got, want, (layout, nprobe, k))
        live = got[0][got[0] >= 0]
        assert np.isin(live, ids[has]).all() and live.shape[0] > 0   # directly: only ids that have a value
    a.close()


# ---- 6. non-finite -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", ["nan", "inf"])
def test_nonfinite(ctx, cls, metric):
    c = NFY.corpus(cls, metric, 6000, 16, 32, seed=61)
    c["cent"] = c["centroids"]
    s, parent = _stores(ctx, c)
    ids = c["ids"]
    q, special_q = NFY.queries(c, 12, seed=62)
    sp = c["special"]                       # 5 rows in one host list, 5 in another, 5 in the tiny list
    vals = ids % 37
    vals[sp[:5]] = 900                      # a group made of special rows only
    vals[sp[10:]] = 901                     # ... and another one (the tiny list)
    a = _attr(s, ids, vals)
    nprobe, k, m = 4, 45, 3                 # more than the 39 groups: every group that has a candidate appears
    pids = GY.probed(q, c["cent"], c["offsets"], nprobe, metric)
    want = GMY.scan(q, c["vecs"], ids, c["offsets"], pids, k, m, metric, ids, vals)
    lims, rows, val = GY.candidates(q, c["vecs"], ids, c["offsets"], pids, metric)
    seen_nan_only = seen_nan_member = 0
    for i in range(q.shape[0]):
        r, v = rows[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
        for g in (900, 901):
            mine = vals[r] == g
            if mine.any() and np.isnan(v[mine]).all():   # probed, and NaN against this query in every row: the group is absent
                seen_nan_only += 1
                assert g not in want[2][i][want[0][i, :, 0] >= 0]
        nan_ids = ids[r[np.isnan(v)]]
        seen_nan_member += int(nan_ids.shape[0] > 0)
        assert not np.isin(want[0][i], nan_ids).any()    # a NaN row is never a member
    if cls == "nan":
        assert seen_nan_only > 0 and seen_nan_member > 0
    else:
        live = want[0] >= 0
        assert np.isinf(want[1][live]).any() and np.isin(ids[sp], want[0][live]).any()   # infinite rows are members, in order
        inf_member = np.isinf(want[1]) & live
        assert inf_member[:, :, 1:].any()                                                  # ... behind member 0 too
    got = ctx.scan_grouped(s, q, pids, k, metric, a, group_size=m)
    _eq(got, want, (cls, metric))
    NFY.assert_no_nan_pair(c, q, special_q, got[0].reshape(q.shape[0], -1))
    _eq(ctx.search_grouped(parent, s, torch.from_numpy(q).cuda(), nprobe, k, metric, a, group_size=m), want, (cls, metric, "search, device"))
    a.close()
    s.close()
    parent.close()


# ---- 7. filters --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filters(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent, cols = corpora(64, metric)
    ids = c["ids"]
    vals = (ids % 40) * 1000003 - 7   # 40 groups: a group that loses its best row is still among the k best
    col = _attr(s, ids, vals)
    q = RY.queries(c, 33, seed=271)
    nprobe, k, m = 8, 10, 4
    plain = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], nprobe, k, m, metric, ids, vals)
    gone_group = plain[2][0, 0]                                     # every row of query 0's best group is disallowed
    deny = np.union1d(plain[0][:, 0, 0], ids[vals == gone_group])   # ... and every query's best row
    want = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], nprobe, k, m, metric, ids, vals, S=deny, mode="deny")
    assert gone_group not in want[2][0] and not np.isin(want[0], deny).any()
    # a group whose best row is disallowed stays, with its allowed rows: its former members 1 .. move up
    moved = 0
    for i in range(1, 33):
        g = plain[2][i, 0]
        if g == gone_group or g not in want[2][i]:
            continue
        j = int(np.nonzero(want[2][i] == g)[0][0])
        rest = [x for x in plain[0][i, 0, 1:] if x >= 0 and x not in deny]
        assert list(want[0][i, j, :len(rest)]) == rest
        moved += int(len(rest) > 0)
    assert moved >= 5
    f_ids = Filter(s, deny, "deny")
    flag = _attr(s, ids, np.isin(ids, deny).astype(np.int64))
    f_where = Filter.where(s, [(flag, "range", 0, 0), (col, "not_range", 1, 0)])
    xd = torch.from_numpy(q).cuda()
    for tag, f in (("ids", f_ids), ("where", f_where)):
        _eq(ctx.search_grouped(parent, s, q, nprobe, k, metric, col, filter=f, group_size=m), want, (metric, tag))
        gp, _ = ctx.coarse(parent, xd, nprobe, metric)
        _eq(ctx.scan_grouped(s, xd, gp, k, metric, col, filter=f, group_size=m), want, (metric, tag, "scan, device"))
    for f in (f_ids, f_where):
        f.close()
    flag.close()
    col.close()


# ---- 8. wide rows ------------------------------------------------------------------------------------------------------------------
def test_wide_rows(ctx):
    c = RY.corpus(3072, 8, 3000, "l2", seed=551)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 17, seed=552)
    vals = _card_values(c["ids"], "n8")
    a = _attr(s, c["ids"], vals)
    want = GMY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, 10, 3, "l2", c["ids"], vals)
    assert ((want[0][:, :, 0] >= 0) & (want[0][:, :, 2] < 0)).any() and (want[0][:, :, 1] >= 0).any()
    got = ctx.search_grouped(parent, s, q, 3, 10, "l2", a, group_size=3)
    assert ctx.last_scan_kernel() == "k_scan_wide (grouped)"
    _eq(got, want, "wide")
    a.close()
    s.close()
    parent.close()


# ---- 9. passes ---------------------------------------------------------------------------------------------------------------------
def test_passes(ctx):
    """The construction of tests/test_grouped_search.py::test_passes: one unprobed list of 300 000 rows makes a call with P = 32 run
    in several passes while the probed work stays tiny.  The pass count follows the workspace rule include/quake_hip.h documents
    for group_size > 1."""
    from quake_amd.capi import Store
    d, nsmall, big = 16, 48, 300000
    rng = np.random.default_rng(291)
    sizes = rng.integers(0, 60, size=nsmall)
    sizes[[3, 17]] = 0
    sizes = np.concatenate([sizes, [big]]).astype(np.int64)
    offsets = np.zeros(nsmall + 2, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    Q, P, k, m = 64, 32, 10, 4
    q = rng.standard_normal((Q, d)).astype(np.float32)
    pids = np.stack([rng.permutation(nsmall)[:P] for _ in range(Q)]).astype(np.int64)
    pids[rng.random((Q, P)) < 0.05] = -1
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    vals = ids % 40 - 20
    a = _attr(s, ids, vals)
    # the rule: per query 12 bytes per key it has room for, 24 per slot of a table of T + 1 slots, 12 per k and 4 per member word
    ub = P * big
    T = 16
    while T < 2 * min(ub, n):
        T *= 2
    qc = min((1 << 29) // ub, (1 << 31) // (12 * ub + 24 * (T + 1) + 12 * k + 4 * k * m))
    passes = -(-Q // qc)
    assert passes >= 2 and qc < (1 << 29) // ub
    want = GMY.scan(q, vecs, ids, offsets, pids, k, m, "l2", ids, vals)
    assert (want[0] >= 0).all()
    ctx.set_timing(1)
    try:
        gi, gd, gg, tm = ctx.scan_grouped(s, q, pids, k, "l2", a, timing=True, group_size=m)
        assert tm["n_items"] == passes
        _eq((gi, gd, gg), want, "passes")
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------------
def test_determinism(ctx, corpora):
    c, s, parent, cols = corpora(128, "l2")
    q = RY.queries(c, 33, seed=301)
    runs = [ctx.search_grouped(parent, s, q, 4, 10, "l2", cols["n8"], group_size=4) for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    rev = ctx.search_grouped(parent, s, np.ascontiguousarray(q[::-1]), 4, 10, "l2", cols["n8"], group_size=4)
    for x, y in zip(runs[0], rev):
        assert x.tobytes() == np.ascontiguousarray(y[::-1]).tobytes()
    want = GMY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, 4, "l2", c["ids"], _card_values(c["ids"], "n8"))
    assert (want[0][:, :, 1] >= 0).any()
    _eq(runs[0], want, "det")


# ---- 11. follows changes of the column and of the store ----------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = RY.corpus(32, 24, 6000, "l2", seed=81)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 33, seed=83)
    pids = GY.probed(q, c["cent"], c["offsets"], 6, "l2")
    col = {int(i): int(i) % 12 for i in c["ids"]}   # 12 groups, 13 after the first change: k = 14 shows every one
    a = _attr(s, np.array(list(col)), np.array(list(col.values())))

    def check(tag):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(24)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        ai, av = np.array(list(col), np.int64), np.array(list(col.values()), np.int64)
        want = GMY.scan(q, vecs, ids, offs, pids, 14, 3, "l2", ai, av)
        _eq(ctx.scan_grouped(s, q, pids, 14, "l2", a, group_size=3), want, tag)
        return want

    w0 = check("as built")
    assert (w0[0][:, 0, 1] >= 0).all()
    # member 1 of query 0's best group moves to a group of its own: member 2 moves up, the row leads the new group
    second, third, old = int(w0[0][0, 0, 1]), int(w0[0][0, 0, 2]), int(w0[2][0, 0])
    assert third >= 0
    col[second] = 777777
    a.set(np.array([second]), np.array([777777]))
    w1 = check("qk_attr_set")
    assert w1[2][0, 0] == old and w1[0][0, 0, 1] == third and 777777 in w1[2][0]
    j = list(w1[2][0]).index(777777)
    assert list(w1[0][0, j]) == [second, -1, -1]
    # a new row next to every query, in the group of the query's best row: it becomes a member of that group
    new_ids = np.arange(10 ** 6, 10 ** 6 + 33, dtype=np.int64)
    s.add_batch(new_ids, q + np.float32(1e-3), np.ascontiguousarray(pids[:, 0]))
    for i, g in zip(new_ids, w1[2][:, 0]):
        col[int(i)] = int(g)
    a.set(new_ids, np.ascontiguousarray(w1[2][:, 0]))
    w2 = check("add")
    assert (w2[2][:, 0] == w1[2][:, 0]).all() and all(new_ids[i] in w2[0][i, 0] for i in range(33))
    # ... and leaves with it
    s.remove_ids(new_ids[::2])
    w3 = check("remove")
    assert not np.isin(w3[0], new_ids[::2]).any() and np.isin(new_ids[1::2], w3[0]).all()
    a.close()
    s.close()
    parent.close()


# ---- 12. errors --------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, corpora):
    from quake_amd._lib import QK_MEM_HOST, QK_METRIC_L2 as L2, QuakeHipError
    from quake_amd.capi import Store
    c, s, parent, cols = corpora(64, "l2")
    q = RY.queries(c, 5, seed=311)
    col = cols["n8"]
    pids = GY.probed(q, c["cent"], c["offsets"], 4, "l2")
    out = (np.zeros((5, 10, 1), np.int64), np.zeros((5, 10, 1), np.float32), np.zeros((5, 10), np.int64))
    for m in (0, -2):
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*group_size"):
            ctx.search_grouped(parent, s, q, 4, 10, "l2", col, group_size=m, out=out)
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*group_size"):
            ctx.scan_grouped(s, q, pids, 10, "l2", col, group_size=m, out=out)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*group_size"):
        ctx.search_grouped(parent, s, q, 4, 10, "l2", col, group_size=17)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*group_size"):
        ctx.scan_grouped(s, q, pids, 10, "l2", col, group_size=17)
    # the existing checks stay
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*k="):
        ctx.search_grouped(parent, s, q, 4, 0, "l2", col, group_size=2, out=out)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*8192"):
        ctx.search_grouped(parent, s, q, 4, 8193, "l2", col, group_size=2)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.search_grouped(parent, s, q, 4, 10, "l2", None, group_size=2)
    # Q = 0: nothing is written
    P = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    oi, od, og = np.full((5, 10, 3), 77, np.int64), np.zeros((5, 10, 3), np.float32), np.zeros((5, 10), np.int64)
    assert ctx.lib.qk_search_grouped_n(ctx.h, parent.h, s.h, P(q), 0, 4, 10, 3, L2, col.h, None, P(oi), P(od), P(og), QK_MEM_HOST, None) == 0
    assert (oi == 77).all()
    got = ctx.search_grouped(parent, s, q[:0], 4, 10, "l2", col, group_size=3)
    assert tuple(got[0].shape) == (0, 10, 3) and tuple(got[2].shape) == (0, 10)
    # groups and distances may be NULL
    want = GMY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, 3, "l2", c["ids"], _card_values(c["ids"], "n8"))
    assert ctx.lib.qk_search_grouped_n(ctx.h, parent.h, s.h, P(q), 5, 4, 10, 3, L2, col.h, None, P(oi), None, None, QK_MEM_HOST, None) == 0
    np.testing.assert_array_equal(oi, want[0])
    # no lists: all padding, [Q, k, m]
    e = Store(ctx, 64)
    ea = _attr(e, np.array([1, 2, 3]), np.array([5, 5, 6]))
    for xq in (q, torch.from_numpy(q).cuda()):
        gi, gd, gg = ctx.search_grouped(None, e, xq, 1, 4, "l2", ea, group_size=3)
        ctx.synchronize()
        assert tuple(gi.shape) == (5, 4, 3) and tuple(gd.shape) == (5, 4, 3) and tuple(gg.shape) == (5, 4)
        assert (_np(gi) == -1).all() and (_np(gd) == np.inf).all() and (_np(gg) == 0).all()
    ea.close()
    e.close()
    # the context still answers
    _eq(ctx.search_grouped(parent, s, q, 4, 10, "l2", col, group_size=3), want, "after the errors")


# ---- 13. mirrors -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def test_mirrors(qb, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(321)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(33, d, generator=g)
    vals = ids % 1500 - 100   # four rows per group: some returned groups have a second candidate, few a third
    idx = quake.QuakeIndex()
    bp = quake.IndexBuildParams()
    bp.nlist, bp.metric = 20, "l2"
    idx.build(x, ids, bp)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    before = repr(quake.SearchParams())
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(322)))
    sps = []
    for mod, m in ((quake, idx), (qb, loaded)):
        m.set_attribute("doc", ids, vals)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 10, 5
        sps.append(sp)
    sp, spc = sps
    for exclude in (None, True):
        sp.filter = None if exclude is None else idx.make_filter(S, exclude)
        spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
        base = idx._ctx.search_grouped(idx.parent._store, idx._store, q.numpy(), 5, 10, "l2", idx._attributes()["doc"],
                                       filter=sp.filter._h if sp.filter is not None else None, group_size=3)
        assert (base[0][:, :, 1] >= 0).any() and (base[0][:, :, 2] == -1).any()
        for xq in (q, q.cuda()):
            r = idx.grouped_search(xq, "doc", sp, group_size=3)
            rc = loaded.grouped_search(xq, "doc", spc, group_size=3)
            for tag, res in (("python", r), ("compiled", rc)):
                assert tuple(res.ids.shape) == (33, 10, 3) and tuple(res.distances.shape) == (33, 10, 3) and tuple(res.groups.shape) == (33, 10)
                assert res.ids.is_cuda == xq.is_cuda and res.groups.is_cuda == xq.is_cuda and res.timing_info.n_queries == 33
                _eq((res.ids, res.distances, res.groups), base, (tag, exclude, xq.is_cuda))
        if exclude:
            assert not np.isin(base[0], S.numpy()).any()
        # group_size = None: today's rank-2 result, member 0 of the above
        for res in (idx.grouped_search(q, "doc", sp), loaded.grouped_search(q, "doc", spc), idx.grouped_search(q, "doc", sp, None),
                    loaded.grouped_search(q, "doc", spc, group_size=None)):
            assert tuple(res.ids.shape) == (33, 10) and tuple(res.distances.shape) == (33, 10)
            _eq((res.ids, res.distances, res.groups), (base[0][:, :, 0], base[1][:, :, 0], base[2]), ("rank 2", exclude))
    sp.filter = spc.filter = None
    assert "group" not in before and repr(quake.SearchParams()) == before and repr(qb.SearchParams()) == before
    # empty x
    for res in (idx.grouped_search(q[:0], "doc", sp, group_size=3), loaded.grouped_search(q[:0], "doc", spc, group_size=3)):
        assert tuple(res.ids.shape) == (0, 10, 3) and tuple(res.distances.shape) == (0, 10, 3) and tuple(res.groups.shape) == (0, 10)
    # the refusals: group_size out of range in the same words; the existing ones stay
    for m in (0, 17, -1):
        texts = []
        for index, p in ((idx, sp), (loaded, spc)):
            with pytest.raises(RuntimeError, match="group_size") as ei:
                index.grouped_search(q, "doc", p, group_size=m)
            texts.append(str(ei.value))
        assert texts[0] == texts[1]
    for index, p in ((idx, sp), (loaded, spc)):
        p.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            index.grouped_search(q, "doc", p, group_size=3)
        p.recall_target = -1.0
        with pytest.raises(RuntimeError, match="unknown attribute"):
            index.grouped_search(q, "nope", p, group_size=3)
        res = index.grouped_search(q, "doc", p, group_size=16)
        assert tuple(res.ids.shape) == (33, 10, 16)
