"""Grouped search (qk_search_grouped / qk_scan_grouped; Context.search_grouped / scan_grouped; QuakeIndex.grouped_search in both
mirrors): the k best groups of an attribute column per query, every group represented by its best row.

Every comparison is bit for bit -- ids, the uint32 view of the distances, groups -- against tests/grouped_yardstick.py (pinned on
the CPU by tests/test_grouped_oracle.py).  No assertion reads a clock.  Every test asserts on its own inputs that the situation it is
about occurs."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import filter_yardstick as FY
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


def _list_of(offsets, rows):
    return np.searchsorted(offsets, rows, side="right") - 1


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
AXES = dict(metric=["l2", "ip"], d=[64, 128], nprobe=[1, 4, 64], Q=[1, 17, 33], k=[1, 10, 449, "over"], card=list(CARDS),
            mem=["host", "device"], entry=["search_grouped", "coarse+scan_grouped"])
K_OVER = 3000  # more than the 2500 groups of "n8" (and than the one of "one")


def _grid():
    """every value of every axis, in combinations a fixed seed decides (the pruning of tests/test_range_search.py)"""
    rng = np.random.default_rng(20250611)
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
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, case):
    c, s, parent, cols = corpora(case["d"], case["metric"])
    metric, nprobe, Q, card = case["metric"], case["nprobe"], case["Q"], case["card"]
    k = K_OVER if case["k"] == "over" else case["k"]
    q = RY.queries(c, Q, seed=zlib.crc32(repr(sorted(case.items(), key=str)).encode()) % (1 << 30))
    pids = GY.probed(q, c["cent"], c["offsets"], nprobe, metric)
    vals = _card_values(c["ids"], card)
    want = GY.scan(q, c["vecs"], c["ids"], c["offsets"], pids, k, metric, c["ids"], vals)
    if case["k"] == "over" and card != "own":
        assert (want[0][:, -1] == -1).all() and (want[0][:, 0] >= 0).all()   # fewer groups than k: padding
    if card == "one":
        assert (want[0][:, 1:] == -1).all()
    dev = case["mem"] == "device"
    xq = torch.from_numpy(q).cuda() if dev else q
    if case["entry"] == "search_grouped":
        got = ctx.search_grouped(parent, s, xq, nprobe, k, metric, cols[card])
    else:
        gp, _ = ctx.coarse(parent, xq, nprobe, metric)
        got = ctx.scan_grouped(s, xq, gp, k, metric, cols[card])
    ctx.synchronize()
    assert ctx.last_scan_kernel() == "k_scan (grouped)"
    _eq(got, want, case)
    if card == "own":  # every row its own group: the plain search at the same k, on either side of QK_MAX_K
        pi, pd = ctx.search(parent, s, xq, nprobe, k, metric)
        ctx.synchronize()
        np.testing.assert_array_equal(_np(got[0]), _np(pi))
        np.testing.assert_array_equal(_np(got[1]).view(np.uint32), _np(pd).view(np.uint32))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    c = RY.corpus(3072, 8, 3000, metric, seed=551)
    s, parent = _stores(ctx, c)
    q = RY.queries(c, 17, seed=552)
    for card, k in (("n8", 10), ("own", 449), ("one", 3)):
        vals = _card_values(c["ids"], card)
        a = _attr(s, c["ids"], vals)
        got = ctx.search_grouped(parent, s, q, 3, k, metric, a)
        assert ctx.last_scan_kernel() == "k_scan_wide (grouped)"
        _eq(got, GY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, metric, c["ids"], vals), (metric, card))
        a.close()
    s.close()
    parent.close()


# ---- 2. a group that spans several probed lists -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_group_spans_lists(ctx, corpora, metric):
    c, s, parent, cols = corpora(64, metric)
    q = RY.queries(c, 33, seed=21)
    ids = c["ids"]
    vals = ids % 7 + 100   # seven groups: every one has rows in every probed list
    a = _attr(s, ids, vals)
    # the probed lists farthest first: a group's first rows in scan order are then in the farthest list, its best row is elsewhere
    pids = np.ascontiguousarray(GY.probed(q, c["cent"], c["offsets"], 4, metric)[:, ::-1])
    want = GY.scan(q, c["vecs"], ids, c["offsets"], pids, 7, metric, ids, vals)
    lims, rows, val = GY.candidates(q, c["vecs"], ids, c["offsets"], pids, metric)
    not_first = 0
    for i in range(q.shape[0]):
        r = rows[lims[i]:lims[i + 1]]
        mine = r[vals[r] == want[2][i, 0]]
        assert np.unique(_list_of(c["offsets"], mine)).shape[0] >= 2, "the winning group must have rows in two probed lists"
        # a per-list best would differ: the representative is not in the list the group's first rows are in
        for j in range(7):
            rep_row = np.nonzero(ids == want[0][i, j])[0][0]
            g_rows = r[vals[r] == want[2][i, j]]
            not_first += int(_list_of(c["offsets"], rep_row) != _list_of(c["offsets"], g_rows[0]))
    assert not_first > 100
    _eq(ctx.scan_grouped(s, q, pids, 7, metric, a), want, (metric, "farthest first"))
    _eq(ctx.search_grouped(parent, s, q, 4, 7, metric, a), want, metric)
    a.close()


# ---- 3. exact ties, ids beyond 2^40 ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_ids(ctx):
    """a small store whose ids lie beyond 2^40 (the column is in the sorted layout), with two planted pairs of duplicate vectors:
    rows A1 / A2 (lists 5 and 6) in one group of their own -- A2 has the smaller id, and the two ids differ above bit 32 only;
    rows B1 / B2 (lists 5 and 7) in two groups of their own -- equal low 32 bits again"""
    c = RY.corpus(32, 12, 3000, "l2", seed=31)
    ids = c["ids"] + (1 << 40)
    off = c["offsets"]
    a1, a2, b1, b2 = off[5] + 3, off[6] + 20, off[5] + 17, off[7] + 1
    c["vecs"][a2] = c["vecs"][a1]
    c["vecs"][b2] = c["vecs"][b1]
    ids[a1], ids[a2], ids[b1], ids[b2] = (1 << 42) + 9, (1 << 40) + 9 + (1 << 33), (1 << 41) + 5, (1 << 40) + 5 + (1 << 34)
    assert np.unique(ids).shape[0] == ids.shape[0]
    c["ids"] = ids
    vals = ids % 50
    vals[[a1, a2]] = 1000001
    vals[b1], vals[b2] = 1000002, 1000003
    s, parent = _stores(ctx, c)
    col = _attr(s, ids, vals)
    assert col.info()["layout"] == "sorted"
    yield dict(c=c, s=s, parent=parent, col=col, vals=vals, planted=(a1, a2, b1, b2))
    col.close()
    s.close()
    parent.close()


def test_ties(ctx, big_ids):
    c, s, parent, col, vals = (big_ids[n] for n in ("c", "s", "parent", "col", "vals"))
    a1, a2, b1, b2 = big_ids["planted"]
    ids = c["ids"]
    q = np.ascontiguousarray(np.stack([c["vecs"][a1], c["vecs"][b1]] + list(RY.queries(c, 6, seed=32))))
    want = GY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 12, 20, "l2", ids, vals)
    # the ties exist in the yardstick: both duplicates are candidates at the same canonical value
    lims, rows, val = GY.candidates(q, c["vecs"], ids, c["offsets"], GY.probed(q, c["cent"], c["offsets"], 12, "l2"), "l2")
    v0 = {int(r): v for r, v in zip(rows[lims[0]:lims[1]], val[lims[0]:lims[1]])}
    v1 = {int(r): v for r, v in zip(rows[lims[1]:lims[2]], val[lims[1]:lims[2]])}
    assert v0[int(a1)] == v0[int(a2)] == min(v0.values()) and v1[int(b1)] == v1[int(b2)] == min(v1.values())
    # one group: the smaller id wins, the other row is nowhere; two groups: both, in id order
    assert want[0][0, 0] == ids[a2] < ids[a1] and ids[a1] not in want[0][0] and want[2][0, 0] == 1000001
    assert list(want[0][1, :2]) == sorted([ids[b1], ids[b2]]) and want[1][1, 0] == want[1][1, 1]
    assert (ids[a1] & 0xFFFFFFFF) == (ids[a2] & 0xFFFFFFFF) and (ids[b1] & 0xFFFFFFFF) == (ids[b2] & 0xFFFFFFFF)
    for xq in (q, torch.from_numpy(q).cuda()):
        _eq(ctx.search_grouped(parent, s, xq, 12, 20, "l2", col), want, "ties")
    _eq(ctx.search_grouped(parent, s, q, 12, 1, "l2", col), tuple(w[:, :1] for w in want), "ties, k = 1")


# ---- 4. hostile values ------------------------------------------------------------------------------------------------------------------
def test_hostile_values(ctx, corpora):
    c, s, parent, cols = corpora(64, "l2")
    ids = c["ids"]
    # 4 extreme values and 400 values that agree in their low 40 bits, dealt round-robin: 404 groups, every one in every long list
    pool = np.concatenate([np.array([I64MIN, I64MAX, -1, 0], np.int64), np.arange(400, dtype=np.int64) * (1 << 40) + 12345])
    vals = pool[ids % pool.shape[0]]
    a = _attr(s, ids, vals)
    q = RY.queries(c, 17, seed=41)
    G = pool.shape[0]
    for k in (G - 1, G + 1, 449):
        want = GY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 64, k, "l2", ids, vals)
        assert np.unique(want[2][0][want[0][0] >= 0]).shape[0] == min(k, G)
        if k == G - 1:   # one group more than k: a full row that leaves exactly one group out
            assert (want[0] >= 0).all()
        if k == G + 1:   # one group fewer than k: exactly one padding entry
            assert (want[0][:, :G] >= 0).all() and (want[0][:, G] == -1).all()
            for v in (I64MIN, I64MAX, -1, 0):
                assert (want[2][:, :G] == v).sum(axis=1).min() == 1
        _eq(ctx.search_grouped(parent, s, q, 64, k, "l2", a), want, ("hostile", k))
    a.close()


# ---- 5. rows without a value ------------------------------------------------------------------------------------------------------------
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
    q = RY.queries(c, 17, seed=51)
    q[0] = c["cent"][bare]
    want = GY.search(q, c["cent"], c["vecs"], ids, off, 1, 10, "l2", ids[has], vals[has])
    assert GY.probed(q[:1], c["cent"], off, 1, "l2")[0, 0] == bare and (want[0][0] == -1).all()   # nothing but padding
    assert (want[0][1:, 0] >= 0).any()
    for nprobe, k in ((1, 10), (4, 120)):
        want = GY.search(q, c["cent"], c["vecs"], ids, off, nprobe, k, "l2", ids[has], vals[has])
        got = ctx.search_grouped(parent, s, q, nprobe, k, "l2", a)
        _eq(got, want, (layout, nprobe, k))
        live = got[0][got[0] >= 0]
        assert np.isin(live, ids[has]).all() and live.shape[0] > 0   # directly: only ids that have a value
    a.close()


# ---- 6. non-finite ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", ["nan", "inf"])
def test_nonfinite(ctx, cls, metric):
    c = NFY.corpus(cls, metric, 6000, 16, 32, seed=61)
    c["cent"] = c["centroids"]
    s, parent = _stores(ctx, c)
    ids = c["ids"]
    q, special_q = NFY.queries(c, 12, seed=62)
    h0, h1 = c["hosts"]
    sp = c["special"]                       # 5 rows in h0, 5 in h1, 5 in the tiny list
    vals = ids % 37
    vals[sp[:5]] = 900                      # a group made of special rows only
    vals[sp[10:]] = 901                     # ... and another one (the tiny list)
    shared = vals[sp[5:10]].copy()          # the specials of h1 share their groups with ordinary rows
    a = _attr(s, ids, vals)
    nprobe, k = 4, 45                       # more than the 39 groups: every group that has a candidate appears
    pids = GY.probed(q, c["cent"], c["offsets"], nprobe, metric)
    want = GY.scan(q, c["vecs"], ids, c["offsets"], pids, k, metric, ids, vals)
    lims, rows, val = GY.candidates(q, c["vecs"], ids, c["offsets"], pids, metric)
    seen_nan_only = seen_nan_shared = 0
    for i in range(q.shape[0]):
        r, v = rows[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
        for g in (900, 901):
            m = vals[r] == g
            if m.any() and np.isnan(v[m]).all():   # probed, and NaN against this query in every row: the group is absent
                seen_nan_only += 1
                assert g not in want[2][i][want[0][i] >= 0]
        for row, g in zip(sp[5:10], shared):
            m = r == row
            if m.any() and np.isnan(v[m]).all() and (~np.isnan(v[vals[r] == g])).any():
                seen_nan_shared += 1
                assert ids[row] not in want[0][i] and g in want[2][i]   # a finite row represents the group, never the NaN row
    if cls == "nan":
        assert seen_nan_only > 0 and seen_nan_shared > 0
    else:
        live = want[0] >= 0
        assert np.isinf(want[1][live]).any() and np.isin(ids[sp], want[0][live]).any()   # infinite rows compete and appear
    got = ctx.scan_grouped(s, q, pids, k, metric, a)
    _eq(got, want, (cls, metric))
    NFY.assert_no_nan_pair(c, q, special_q, got[0])
    _eq(ctx.search_grouped(parent, s, torch.from_numpy(q).cuda(), nprobe, k, metric, a), want, (cls, metric, "search, device"))
    a.close()
    s.close()
    parent.close()


# ---- 7. filters ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filters(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent, cols = corpora(64, metric)
    ids = c["ids"]
    vals = (ids % 40) * 1000003 - 7   # 40 groups: a group that loses its best row is still among the k best
    col = _attr(s, ids, vals)
    q = RY.queries(c, 33, seed=71)
    nprobe, k = 8, 10
    plain = GY.search(q, c["cent"], c["vecs"], ids, c["offsets"], nprobe, k, metric, ids, vals)
    gone_group = plain[2][0, 0]                                  # every row of query 0's best group is disallowed
    deny = np.union1d(plain[0][:, 0], ids[vals == gone_group])   # ... and every query's best row
    want = GY.search(q, c["cent"], c["vecs"], ids, c["offsets"], nprobe, k, metric, ids, vals, S=deny, mode="deny")
    assert gone_group not in want[2][0] and not np.isin(want[0], deny).any()
    # the best row of a group is disallowed and the next one represents it
    moved = [i for i in range(1, 33) if plain[2][i, 0] in want[2][i] and plain[2][i, 0] != gone_group]
    assert len(moved) >= 5
    for i in moved:
        j = int(np.nonzero(want[2][i] == plain[2][i, 0])[0][0])
        assert want[0][i, j] != plain[0][i, 0]
    f_ids = Filter(s, deny, "deny")
    flag = _attr(s, ids, np.isin(ids, deny).astype(np.int64))
    f_where = Filter.where(s, [(flag, "range", 0, 0), (col, "not_range", 1, 0)])
    for tag, f in (("ids", f_ids), ("where", f_where)):
        _eq(ctx.search_grouped(parent, s, q, nprobe, k, metric, col, filter=f), want, (metric, tag))
        gp, _ = ctx.coarse(parent, torch.from_numpy(q).cuda(), nprobe, metric)
        _eq(ctx.scan_grouped(s, torch.from_numpy(q).cuda(), gp, k, metric, col, filter=f), want, (metric, tag, "scan, device"))
    # an allow filter over a few ids: results come from it alone
    allow = FY.draw_set(ids, 0.001, np.random.default_rng(72))
    f_allow = Filter(s, allow, "allow")
    got = ctx.search_grouped(parent, s, q, nprobe, k, metric, col, filter=f_allow)
    _eq(got, GY.search(q, c["cent"], c["vecs"], ids, c["offsets"], nprobe, k, metric, ids, vals, S=allow, mode="allow"), "allow")
    assert np.isin(got[0][got[0] >= 0], allow).all() and (got[0] == -1).any()
    for f in (f_ids, f_where, f_allow):
        f.close()
    flag.close()
    col.close()


# ---- 8. follows changes of the column and of the store -----------------------------------------------------------------------------------
def test_follows_changes(ctx):
    c = RY.corpus(32, 24, 6000, "l2", seed=81)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(82)
    q = RY.queries(c, 33, seed=83)
    pids = GY.probed(q, c["cent"], c["offsets"], 6, "l2")
    col = {int(i): int(i) % 300 for i in c["ids"]}
    a = _attr(s, np.array(list(col)), np.array(list(col.values())))

    def check(tag, builds):
        lists = [s.get_list(p) if p in set(s.list_ids()) else (np.zeros((0, 32), np.float32), np.zeros(0, np.int64)) for p in range(24)]
        vecs, ids, offs = O.csr_from_partitions([l[0] for l in lists], [l[1] for l in lists], 32)
        ai, av = np.array(list(col), np.int64), np.array(list(col.values()), np.int64)
        want = GY.scan(q, vecs, ids, offs, pids, 10, "l2", ai, av)
        got = ctx.scan_grouped(s, q, pids, 10, "l2", a)
        _eq(got, want, tag)
        assert a.group_info()["builds"] == builds, tag
        return want

    w0 = check("as built", 1)
    check("nothing changed", 1)
    # the best row of query 0 moves to a group of its own: it now represents that group, its old group is represented by another row
    best, old = int(w0[0][0, 0]), int(w0[2][0, 0])
    col[best] = 777777
    a.set(np.array([best]), np.array([777777]))
    w1 = check("set_attribute", 2)
    assert w1[0][0, 0] == best and w1[2][0, 0] == 777777 and (old not in w1[2][0] or w1[0][0][list(w1[2][0]).index(old)] != best)
    del col[best]
    a.unset(np.array([best]))
    w2 = check("unset_attribute", 3)
    assert best not in w2[0]
    na = 500
    new_ids = np.arange(10 ** 6, 10 ** 6 + na, dtype=np.int64)
    lists = rng.integers(4, 24, size=na).astype(np.int64)
    new_vecs = (c["cent"][lists] + 0.3 * rng.standard_normal((na, 32))).astype(np.float32)
    lists[:33] = pids[:, 0]                 # the first 33 sit next to the queries, in a list the query probes
    new_vecs[:33] = q + np.float32(1e-3)
    s.add_batch(new_ids, new_vecs, lists)
    check("add (no values yet)", 4)
    for i in new_ids[::2]:
        col[int(i)] = 555000 + int(i) % 3
    a.set(new_ids[::2], np.array([col[int(i)] for i in new_ids[::2]]))
    w3 = check("values for the added rows", 5)
    assert (w3[0][0::2, 0] == new_ids[0:33:2]).all() and not np.isin(w3[0], new_ids[1::2]).any()
    s.remove_ids(np.unique(w3[0][w3[0] >= 0])[::2])
    w4 = check("remove", 6)
    assert not (w4[0] == w3[0]).all()
    check("nothing changed again", 6)
    a.close()
    s.close()
    parent.close()


# ---- 9. passes ------------------------------------------------------------------------------------------------------------------------------
def test_passes(ctx):
    """The construction of tests/test_range_search.py::test_passes: one unprobed list of 300 000 rows makes a call with P = 32 run in
    many passes while the probed work stays tiny.  The pass count follows the documented workspace rule (include/quake_hip.h)."""
    from quake_amd.capi import Store
    d, nsmall, big = 16, 48, 300000
    rng = np.random.default_rng(91)
    sizes = rng.integers(0, 60, size=nsmall)
    sizes[[3, 17]] = 0
    sizes = np.concatenate([sizes, [big]]).astype(np.int64)
    offsets = np.zeros(nsmall + 2, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    Q, P, k = 1024, 32, 10
    q = rng.standard_normal((Q, d)).astype(np.float32)
    pids = np.stack([rng.permutation(nsmall)[:P] for _ in range(Q)]).astype(np.int64)
    pids[rng.random((Q, P)) < 0.05] = -1
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    vals = ids % 40 - 20
    a = _attr(s, ids, vals)
    # the rule: per query 8 bytes per key it has room for and 20 per slot of a table of T + 1 slots
    ub = P * big
    T = 16
    while T < 2 * min(ub, n):
        T *= 2
    qc = min((1 << 29) // ub, (1 << 31) // (ub * 8 + (T + 1) * 20))
    passes = -(-Q // qc)
    assert passes == 49 and qc < (1 << 29) // ub
    want = GY.scan(q, vecs, ids, offsets, pids, k, "l2", ids, vals)
    assert (want[0] >= 0).all()
    ctx.set_timing(1)
    try:
        gi, gd, gg, tm = ctx.scan_grouped(s, q, pids, k, "l2", a, timing=True)
        assert tm["n_items"] == passes
        _eq((gi, gd, gg), want, "passes")
    finally:
        ctx.set_timing(0)
        a.close()
        s.close()


# ---- 10. determinism --------------------------------------------------------------------------------------------------------------------------
def test_determinism(ctx, corpora):
    c, s, parent, cols = corpora(128, "l2")
    q = RY.queries(c, 33, seed=101)
    runs = [ctx.search_grouped(parent, s, q, 4, 10, "l2", cols["n8"]) for _ in range(2)]
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    rev = ctx.search_grouped(parent, s, np.ascontiguousarray(q[::-1]), 4, 10, "l2", cols["n8"])
    for x, y in zip(runs[0], rev):
        assert x.tobytes() == np.ascontiguousarray(y[::-1]).tobytes()
    _eq(runs[0], GY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", c["ids"], _card_values(c["ids"], "n8")), "det")


# ---- 11. errors, refusals, mirrors ------------------------------------------------------------------------------------------------------------
def test_errors(ctx, corpora):
    from quake_amd._lib import QK_MEM_HOST, QK_METRIC_L2 as L2, QuakeHipError
    from quake_amd.capi import Filter
    c, s, parent, cols = corpora(64, "l2")
    c2, s2, parent2, cols2 = corpora(128, "l2")
    q = RY.queries(c, 5, seed=111)
    col = cols["n8"]
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.search_grouped(parent, s, q, 4, 10, "l2", None)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search_grouped(parent, s, q, 4, 10, "l2", cols2["n8"])
    f2 = Filter(s2, c2["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search_grouped(parent, s, q, 4, 10, "l2", col, filter=f2)
    f2.close()
    for k in (0, -3):
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*k="):
            ctx.search_grouped(parent, s, q, 4, k, "l2", col, out=(np.zeros((5, 1), np.int64), np.zeros((5, 1), np.float32), np.zeros((5, 1), np.int64)))
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*8192"):
        ctx.search_grouped(parent, s, q, 4, 8193, "l2", col)
    pids = GY.probed(q, c["cent"], c["offsets"], 4, "l2")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.scan_grouped(s, q, pids, 10, "l2", None)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*8192"):
        ctx.scan_grouped(s, q, pids, 9000, "l2", col)
    P = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    oi, od, og = np.zeros((5, 10), np.int64), np.zeros((5, 10), np.float32), np.zeros((5, 10), np.int64)
    assert ctx.lib.qk_search_grouped(ctx.h, parent.h, s.h, P(q), 5, 0, 10, L2, col.h, None, P(oi), P(od), P(og), QK_MEM_HOST, None) == 1  # nprobe
    assert ctx.lib.qk_scan_grouped(ctx.h, s.h, P(q), 5, None, 4, 10, L2, col.h, None, P(oi), P(od), P(og), QK_MEM_HOST, None) == 1      # no pids
    # k = 8192 is served; groups may be NULL
    vals = _card_values(c["ids"], "n8")
    want = GY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 8192, "l2", c["ids"], vals)
    _eq(ctx.search_grouped(parent, s, q, 4, 8192, "l2", col), want, "k = 8192")
    assert ctx.lib.qk_search_grouped(ctx.h, parent.h, s.h, P(q), 5, 4, 10, L2, col.h, None, P(oi), P(od), None, QK_MEM_HOST, None) == 0
    np.testing.assert_array_equal(oi, want[0][:, :10])
    # pids edge cases as qk_range_scan: -1, out of range and empty lists contribute nothing
    sizes = np.diff(c["offsets"])
    empty = int(np.nonzero(sizes == 0)[0][0])
    edge = np.array([[5, -1, 9], [-1, -1, -1], [10 ** 6, 7, empty], [-1, 6, -1], [64, 65, 10 ** 12]], np.int64)
    want = GY.scan(q, c["vecs"], c["ids"], c["offsets"], np.where(edge >= 64, -1, edge), 10, "l2", c["ids"], vals)
    assert (want[0][[1, 4]] == -1).all() and (want[0][[0, 2, 3]] >= 0).all()
    _eq(ctx.scan_grouped(s, q, edge, 10, "l2", col), want, "edge pids")
    _eq(ctx.scan_grouped(s, torch.from_numpy(q).cuda(), torch.from_numpy(edge).cuda(), 10, "l2", col), want, "edge pids, device")
    # parent == None: every list
    _eq(ctx.search_grouped(None, s, q[:2], 1, 10, "l2", col),
        GY.search(q[:2], None, c["vecs"], c["ids"], c["offsets"], 1, 10, "l2", c["ids"], vals), "all lists")
    # the context still answers
    gi, gd = ctx.search(parent, s, q, 4, 10, "l2")
    oi2, od2 = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", batched_scan=True)
    np.testing.assert_array_equal(gi, oi2)
    np.testing.assert_array_equal(gd.view(np.uint32), od2.view(np.uint32))


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


@pytest.mark.parametrize("nlist", [0, 20])
def test_mirrors(qb, nlist, tmp_path):
    import quake_amd as quake
    g = torch.Generator().manual_seed(121)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(33, d, generator=g)
    vals = ids % 200 - 100
    S = torch.from_numpy(FY.draw_set(ids.numpy(), 0.3, np.random.default_rng(122)))
    idx = _build(quake, x, ids, nlist)
    path = str(tmp_path / "index")
    idx.save(path)
    loaded = qb.QuakeIndex()
    loaded.load(path)
    before = repr(quake.SearchParams())
    for m in (idx, loaded):
        m.set_attribute("doc", ids, vals)
    sps = []
    for mod in (quake, qb):
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 10, 5
        sps.append(sp)
    sp, spc = sps

    def compare(tag):
        for exclude in (None, True):
            sp.filter = None if exclude is None else idx.make_filter(S, exclude)
            spc.filter = None if exclude is None else loaded.make_filter(S, exclude)
            r = idx.grouped_search(q, "doc", sp)
            # the Python mirror is Context.search_grouped on the index's own stores
            base = idx._ctx.search_grouped(idx.parent._store if idx.parent is not None else None, idx._store, q.numpy(), 5, 10, "l2",
                                           idx._attributes()["doc"], filter=sp.filter._h if sp.filter is not None else None)
            _eq((r.ids, r.distances, r.groups), base, ("python", tag, exclude))
            assert r.ids.shape == (33, 10) and r.timing_info.n_queries == 33 and (r.ids >= 0).all()
            for row_i, row_g in zip(r.ids.numpy(), r.groups.numpy()):
                assert len(set(row_g.tolist())) == 10                      # distinct by the attribute
            if exclude:
                assert not np.isin(r.ids.numpy(), S.numpy()).any()
            rd = idx.grouped_search(q.cuda(), "doc", sp)
            assert rd.ids.is_cuda and rd.groups.is_cuda and rd.distances.is_cuda
            _eq((rd.ids, rd.distances, rd.groups), base, ("python, device", tag, exclude))
            for xq in (q, q.cuda()):
                rc = loaded.grouped_search(xq, "doc", spc)
                assert rc.ids.is_cuda == xq.is_cuda and rc.groups.is_cuda == xq.is_cuda
                _eq((rc.ids, rc.distances, rc.groups), base, ("compiled", tag, exclude, xq.is_cuda))
        sp.filter = spc.filter = None

    compare("as built")
    xa = torch.randn(300, d, generator=g)
    ia = torch.arange(300) + 10 ** 6
    for m in (idx, loaded):
        m.add(xa, ia)
        m.set_attribute("doc", ia, ia % 7 + 5000)
    compare("add")
    gone = ids[:1500]
    for m in (idx, loaded):
        m.remove(gone)
    compare("remove")
    r = idx.grouped_search(q, "doc", sp)
    assert not np.isin(r.ids.numpy(), gone.numpy()).any()
    assert "group" not in before and repr(quake.SearchParams()) == before
    empty = idx.grouped_search(q[:0], "doc", sp)
    assert tuple(empty.ids.shape) == (0, 10) and tuple(empty.groups.shape) == (0, 10)
    emptyc = loaded.grouped_search(q[:0], "doc", spc)
    assert tuple(emptyc.ids.shape) == (0, 10)


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(131)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        other = _build(mod, x, ids, 16)
        idx.set_attribute("doc", ids, ids % 50)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        plain = idx.grouped_search(qq, "doc", sp)
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.grouped_search(qq, "doc", sp)
        sp.recall_target = -1.0
        sp.filters = [idx.make_filter(ids[:1000])]
        sp.query_filter = torch.zeros(10, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="query_filter"):
            idx.grouped_search(qq, "doc", sp)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        with pytest.raises(RuntimeError, match="unknown attribute"):
            idx.grouped_search(qq, "nope", sp)
        sp.filter = other.make_filter(ids[:1000])
        with pytest.raises(RuntimeError, match="another index"):
            idx.grouped_search(qq, "doc", sp)
        sp.filter = None
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.grouped_search(qq, "doc", sp)
        again = idx.grouped_search(qq, "doc", sp)
        assert torch.equal(again.ids, plain.ids) and torch.equal(again.distances, plain.distances) and torch.equal(again.groups, plain.groups)
