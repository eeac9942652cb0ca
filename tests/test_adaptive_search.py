"""Adaptive probing under a filter (qk_search_filtered_adaptive; capi.Context.search_adaptive; SearchParams.max_nprobe /
filter_min_candidates and SearchResult.nprobed in both mirrors): every query probes the shortest prefix of its ranked lists that
holds min_candidates candidates of its filter, cut on the device between the coarse step and the scan (k_filter_list_counts,
k_probe_trim).

Expected values come from tests/adaptive_yardstick.py -- the definition, one query at a time, pinned on the CPU by
tests/test_adaptive_oracle.py -- and every comparison is exact: ids, the uint32 view of the distances, nprobed, the probed rows.
No test reads a clock."""
import zlib

import numpy as np
import pytest
import torch

import adaptive_yardstick as A
import attr_yardstick as AY
import filter_yardstick as Y
import oracle as O
from test_filtered_search import _build, _eq, _index_csr, _np

pytestmark = pytest.mark.gpu

QK_MAX_K = 448
QK_MAX_NPROBE = 8192
NLIST = 130
SIZES = [0, 0, 1, 15, 16, 17, 255, 256, 257, 5003]  # list 0 is taken out of the store again: absent, its centroid stays ranked


def _corpus(d, metric, seed):
    """130 lists: an absent one, an empty one, lists around one tile and around 16 tiles, one of ~5000 rows, the rest 20..120 rows"""
    rng = np.random.default_rng(seed)
    sizes = np.array(SIZES + list(rng.integers(20, 120, size=NLIST - len(SIZES))), np.int64)
    offsets = np.zeros(NLIST + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    assign = np.repeat(np.arange(NLIST), sizes)
    cent = rng.standard_normal((NLIST, d)).astype(np.float32)
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) * 3 + 7
    return dict(cent=cent, vecs=np.ascontiguousarray(x), ids=ids, offsets=offsets, d=d, metric=metric)


def _queries(c, Q, seed):
    rng = np.random.default_rng(seed)
    n = c["vecs"].shape[0]
    q = (c["vecs"][rng.integers(0, n, size=Q)] + 0.05 * rng.standard_normal((Q, c["d"]))).astype(np.float32)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q)


def _stores(ctx, c, cent=None):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    s.remove_list(0)  # absent: no rows, no entry in the table -- the parent still ranks its centroid
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, NLIST], np.int64), np.arange(NLIST, dtype=np.int64), c["cent"] if cent is None else cent)
    return s, parent


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c = _corpus(d, metric, seed=300 + d + (1 if metric == "ip" else 0))
            s, parent = _stores(ctx, c)
            assert 0 not in [int(p) for p in s.list_ids()] and s.list_size(1) == 0
            cache[(d, metric)] = (c, s, parent)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


class _Filters:
    """the filter family over one corpus: id allow-sets of selectivity 1 / 0.1 / 0.01 / 0, a deny-set, a predicate -- as
    yardstick filters (`spec`) and as handles of the store (`h`), in the same order"""
    NAMES = ["allow1", "allow0.1", "allow0.01", "allow0", "deny0.3", "where"]

    def __init__(self, s, c, seed):
        from quake_amd.capi import Attr, Filter
        rng = np.random.default_rng(seed)
        ids = c["ids"]
        self.spec = [(Y.draw_set(ids, 1, rng), "allow"), (Y.draw_set(ids, 0.1, rng), "allow"), (Y.draw_set(ids, 0.01, rng), "allow"),
                     (np.zeros(0, np.int64), "allow"), (Y.draw_set(ids, 0.3, rng), "deny")]
        self.h = [Filter(s, S, mode) for S, mode in self.spec]
        # a column `tenant` over 90 % of the ids, values 0 .. 19; the predicate: 3 <= tenant <= 4 (~9 % of the rows)
        have = rng.permutation(ids)[: int(0.9 * ids.shape[0])]
        self.column = {int(i): int(v) for i, v in zip(have, rng.integers(0, 20, size=have.shape[0]))}
        self.attr = Attr(s)
        self.attr.set(np.fromiter(self.column.keys(), np.int64), np.fromiter(self.column.values(), np.int64))
        self.clauses = [("tenant", "range", 3, 4)]
        self.spec.append(AY.eval_clauses(self.clauses, ids, {"tenant": self.column}))
        self.h.append(Filter.where(s, [(self.attr, "range", 3, 4)]))

    def close(self):
        for f in self.h:
            f.close()
        self.attr.close()


@pytest.fixture(scope="module")
def families(corpora):
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c, s, parent = corpora(d, metric)
            cache[(d, metric)] = _Filters(s, c, seed=17 + d)
        return cache[(d, metric)]

    yield get
    for f in cache.values():
        f.close()


def _yard(c, q, nprobe, max_nprobe, minc, k, spec, qf=None, cent=None):
    return A.search(q, c["cent"] if cent is None else cent, c["vecs"], c["ids"], c["offsets"], nprobe, max_nprobe, minc, k, c["metric"],
                    spec, qf)


def _pairs_scanned(probed, offsets):
    """the (query, list) pairs of the prefixes that reach a present, non-empty list: qk_timing::partitions_scanned"""
    sizes = np.diff(np.asarray(offsets, np.int64))
    pr = np.asarray(probed)
    return int((sizes[pr[pr >= 0]] > 0).sum())


def _same(got, want, tag):
    gi, gd, gn, gp = got[:4]
    oi, od, on, op = want
    np.testing.assert_array_equal(_np(gn), on, err_msg=str(tag))
    np.testing.assert_array_equal(_np(gp), op, err_msg=str(tag))
    _eq(gi, gd, oi, od, tag)
    assert _np(gn).dtype == np.int32 and _np(gp).dtype == np.int64


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[8, 128], Q=[1, 17, 33], k=[1, 10, 100],
            probes=[(1, 1), (1, 2), (4, 63), (4, 64), (4, 65), (8, 130), (8, 500)], minc=["1", "k", "4k", "1e9"],
            flt=_Filters.NAMES + ["mixed"], mem=["host", "device"])


def _grid():
    """Case i takes, on every axis, element i of a seeded shuffle of that axis repeated: every value of every axis appears (the
    longest axis has 7 values, there are 28 cases) in combinations the seed decides."""
    rng = np.random.default_rng(20250311)
    n = 28
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


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v).replace(" ", "") for v in c.values()))
def test_grid(ctx, corpora, families, case):
    c, s, parent = corpora(case["d"], case["metric"])
    fam = families(case["d"], case["metric"])
    metric, k, Q = case["metric"], case["k"], case["Q"]
    nprobe, max_nprobe = case["probes"]
    minc = {"1": 1, "k": k, "4k": 4 * k, "1e9": 10 ** 9}[case["minc"]]
    rng = np.random.default_rng(zlib.crc32(repr(sorted(case.items())).encode()))
    q = _queries(c, Q, seed=int(rng.integers(1 << 30)))
    if case["flt"] == "mixed":
        spec, kw = fam.spec, dict(filters=fam.h, query_filter=rng.integers(0, len(fam.h), size=Q).astype(np.int32))
        qf = kw["query_filter"]
    else:
        i = _Filters.NAMES.index(case["flt"])
        spec, qf, kw = [fam.spec[i]], None, dict(filter=fam.h[i])
    want = _yard(c, q, nprobe, max_nprobe, minc, k, spec, qf)
    if case["mem"] == "device":
        xq = torch.from_numpy(q).cuda()
        if "query_filter" in kw:
            kw["query_filter"] = torch.from_numpy(kw["query_filter"]).cuda()
    else:
        xq = q
    got = ctx.search_adaptive(parent, s, xq, nprobe, max_nprobe, k, metric, min_candidates=minc, **kw)
    _same(got, want, case)
    M, n0 = min(max_nprobe, NLIST), min(nprobe, NLIST)
    assert _np(got[3]).shape == (Q, M)
    if minc == 10 ** 9:
        assert (_np(got[2]) == M).all()  # never reached
    if case["flt"] == "allow1" and minc == 1 and nprobe >= 4:
        assert (_np(got[2]) == n0).all()  # reached inside the first nprobe lists
    assert got[4]["partitions_scanned"] == _pairs_scanned(want[3], c["offsets"])  # the pairs actually scanned, not Q * M
    # the NULL forms of the two extra outputs answer the same
    gi, gd, gn, gp, _ = ctx.search_adaptive(parent, s, xq, nprobe, max_nprobe, k, metric, min_candidates=minc, probed=False,
                                            nprobed=False, **kw)
    assert gn is None and gp is None
    _eq(gi, gd, want[0], want[1], (case, "NULL outputs"))


# ---- 2. constructed cuts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_cut_falls_on_the_chunk_boundary(ctx, corpora, metric):
    """One allowed id in every non-empty list of the first 65 ranked lists of query 0: with m of the first 63 non-empty,
    min_candidates = m + 1 is reached exactly at t = 64 -- the last lane of the first chunk of k_probe_trim -- and m + 2 exactly
    at t = 65, the first lane of the second chunk with the whole first chunk carried."""
    from quake_amd.capi import Filter
    c, s, parent = corpora(8, metric)
    sizes = np.diff(c["offsets"])
    cand = _queries(c, 64, seed=909)
    rank, _ = O.coarse(cand, c["cent"], None, NLIST, metric)
    pick = [i for i in range(64) if sizes[rank[i, 63]] > 0 and sizes[rank[i, 64]] > 0 and (sizes[rank[i, :63]] == 0).any()]
    assert pick
    q = np.ascontiguousarray(np.concatenate([cand[pick[0]:pick[0] + 1], cand[:16]]))
    r = rank[pick[0]]
    S = np.array([c["ids"][c["offsets"][p]] for p in r[:65] if sizes[p] > 0], np.int64)
    m = int((sizes[r[:63]] > 0).sum())
    assert m < 63  # lists with 0 candidates lie in the middle of the ranking (the absent and the empty one)
    f = Filter(s, S, "allow")
    for minc, t in [(m + 1, 64), (m + 2, 65)]:
        want = _yard(c, q, 4, NLIST, minc, 10, [(S, "allow")])
        assert want[2][0] == t
        _same(ctx.search_adaptive(parent, s, q, 4, NLIST, 10, metric, min_candidates=minc, filter=f), want, (minc, t))
        for M in (63, 64, 65):  # ... and with the row ending around the boundary
            _same(ctx.search_adaptive(parent, s, q, 4, M, 10, metric, min_candidates=minc, filter=f),
                  _yard(c, q, 4, M, minc, 10, [(S, "allow")]), (minc, t, M))
    f.close()


def test_lists_without_candidates_in_the_middle(ctx, corpora, families):
    c, s, parent = corpora(128, "l2")
    fam = families(128, "l2")
    q = _queries(c, 33, seed=911)
    i = _Filters.NAMES.index("allow0.01")
    want = _yard(c, q, 2, 40, 5, 10, [fam.spec[i]])
    cnt = A.list_counts(A.keep_of(fam.spec[i], c["ids"]), c["offsets"])
    inner = [(cnt[want[3][j, :want[2][j] - 1]] == 0).any() for j in range(33)]
    assert any(inner) and ((want[2] > 2) & (want[2] < 40)).any()
    _same(ctx.search_adaptive(parent, s, q, 2, 40, 10, "l2", min_candidates=5, filter=fam.h[i]), want, "zeros inside")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_a_nan_centroid_leaves_padding_in_the_ranking(ctx, corpora, families, metric):
    c, s, _ = corpora(8, metric)
    fam = families(8, metric)
    cent = c["cent"].copy()
    cent[20, 3] = np.nan
    from quake_amd.capi import Store
    parent = Store(ctx, 8)
    parent.build_csr(np.array([0, NLIST], np.int64), np.arange(NLIST, dtype=np.int64), cent)
    q = _queries(c, 17, seed=913)
    i = _Filters.NAMES.index("allow0.01")
    for minc in (3, 10 ** 9):
        want = _yard(c, q, 8, NLIST, minc, 10, [fam.spec[i]], cent=cent)
        if minc == 10 ** 9:
            assert (want[2] == NLIST).all() and (want[3][:, -1] == -1).all() and not (want[3] == 20).any()
        _same(ctx.search_adaptive(parent, s, q, 8, NLIST, 10, metric, min_candidates=minc, filter=fam.h[i]), want, minc)
    parent.close()


def test_a_device_qfilter_out_of_range(ctx, corpora, families):
    c, s, parent = corpora(8, "l2")
    fam = families(8, "l2")
    Q = 17
    q = _queries(c, Q, seed=915)
    F = len(fam.h)
    qf = (np.arange(Q) % F).astype(np.int32)
    qf[[2, 9]] = [F, -1]
    want = _yard(c, q, 4, 65, 10, 10, fam.spec, qf)
    assert (want[2][[2, 9]] == 0).all() and (want[0][[2, 9]] == -1).all() and (want[3][[2, 9]] == -1).all()
    got = ctx.search_adaptive(parent, s, torch.from_numpy(q).cuda(), 4, 65, 10, "l2", min_candidates=10, filters=fam.h,
                              query_filter=torch.from_numpy(qf).cuda())
    _same(got, want, "device qfilter")
    from quake_amd._lib import QuakeHipError
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*outside"):  # the host reads a host qfilter
        ctx.search_adaptive(parent, s, q, 4, 65, 10, "l2", min_candidates=10, filters=fam.h, query_filter=qf)


# ---- 3. wide rows --------------------------------------------------------------------------------------------------------------
def test_wide_rows(ctx):
    from quake_amd.capi import Filter, Store
    d, nlist, per = 2600, 8, 40
    rng = np.random.default_rng(921)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    vecs = (cent[:, None, :] + 0.4 * rng.standard_normal((nlist, per, d))).astype(np.float32).reshape(-1, d)
    ids = rng.permutation(nlist * per).astype(np.int64)
    offsets = np.arange(nlist + 1, dtype=np.int64) * per
    c = dict(cent=cent, vecs=np.ascontiguousarray(vecs), ids=ids, offsets=offsets, d=d, metric="l2")
    s = Store(ctx, d)
    s.build_csr(offsets, ids, c["vecs"])
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
    q = _queries(c, 17, seed=922)
    S = Y.draw_set(ids, 0.05, rng)
    f = Filter(s, S, "allow")
    for minc in (1, 5, 10 ** 9):
        got = ctx.search_adaptive(parent, s, q, 1, 8, 10, "l2", min_candidates=minc, filter=f)
        assert ctx.last_scan_kernel() == "k_scan_wide (filtered)"
        _same(got, _yard(c, q, 1, 8, minc, 10, [(S, "allow")]), minc)
    f.close()
    s.close()
    parent.close()


# ---- 4. equivalences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_max_nprobe_equal_to_nprobe_is_the_filtered_call(ctx, corpora, families, metric):
    c, s, parent = corpora(128, metric)
    fam = families(128, metric)
    q = _queries(c, 33, seed=931)
    qf = (np.arange(33) % len(fam.h)).astype(np.int32)
    for nprobe in (1, 8, 500):
        for k in (1, 100):
            for minc in (1, 10 ** 9):
                for f in (fam.h[1], fam.h[5]):
                    gi, gd, gn, gp, _ = ctx.search_adaptive(parent, s, q, nprobe, nprobe, k, metric, min_candidates=minc, filter=f)
                    oi, od, op = ctx.search_tracked(parent, s, q, nprobe, k, metric, filter=f)
                    _eq(gi, gd, oi, od, (nprobe, k, minc))
                    np.testing.assert_array_equal(gp, op)
                    assert (gn == min(nprobe, NLIST)).all()
                gi, gd, gn, gp, _ = ctx.search_adaptive(parent, s, q, nprobe, nprobe, k, metric, min_candidates=minc, filters=fam.h,
                                                        query_filter=qf)
                oi, od = ctx.search(parent, s, q, nprobe, k, metric, filters=fam.h, query_filter=qf)
                _eq(gi, gd, oi, od, ("per query", nprobe, k, minc))


def test_row_i_of_a_batch_is_the_single_query_call(ctx, corpora, families):
    c, s, parent = corpora(128, "l2")
    fam = families(128, "l2")
    Q = 33
    q = _queries(c, Q, seed=933)
    qf = ((np.arange(Q) * 5) % len(fam.h)).astype(np.int32)
    gi, gd, gn, gp, _ = ctx.search_adaptive(parent, s, q, 4, 65, 10, "l2", min_candidates=40, filters=fam.h, query_filter=qf)
    assert len(set(gn.tolist())) > 2
    for i in range(Q):
        one = ctx.search_adaptive(parent, s, q[i:i + 1], 4, 65, 10, "l2", min_candidates=40, filter=fam.h[qf[i]])
        _same(one, (gi[i:i + 1], gd[i:i + 1], gn[i:i + 1], gp[i:i + 1]), i)
        # ... and the scan of its prefix
        t = int(gn[i])
        if t:
            si, sd = ctx.scan(s, q[i:i + 1], gp[i:i + 1, :t][:, gp[i, :t] != 0], 10, "l2", filter=fam.h[qf[i]])  # (list 0 is absent)
            _eq(si, sd, gi[i:i + 1], gd[i:i + 1], ("scan", i))


# ---- 5. liveness ---------------------------------------------------------------------------------------------------------------
def _csr_of(s, d):
    """the store's lists 0 .. NLIST-1 as a CSR (an absent list: no rows)"""
    present = {int(p) for p in s.list_ids()}
    vs, is_ = [], []
    for p in range(NLIST):
        v, i = s.get_list(p) if p in present else (np.zeros((0, d), np.float32), np.zeros(0, np.int64))
        vs.append(np.asarray(v, np.float32).reshape(-1, d))
        is_.append(np.asarray(i, np.int64))
    offsets = np.zeros(NLIST + 1, np.int64)
    offsets[1:] = np.cumsum([v.shape[0] for v in vs])
    return np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(is_)), offsets


def test_the_counts_follow_the_store_and_the_columns(ctx):
    from quake_amd.capi import Attr, Filter
    d, metric = 8, "l2"
    c = _corpus(d, metric, seed=941)
    s, parent = _stores(ctx, c)
    rng = np.random.default_rng(942)
    q = _queries(c, 17, seed=943)
    S = Y.draw_set(c["ids"], 0.05, rng)
    new_ids = np.arange(10 ** 6, 10 ** 6 + 700, dtype=np.int64)
    S = np.concatenate([S, new_ids[::2]])  # ids that arrive later
    column = {int(i): int(v) for i, v in zip(c["ids"], rng.integers(0, 10, size=c["ids"].shape[0]))}
    attr = Attr(s)
    attr.set(np.fromiter(column.keys(), np.int64), np.fromiter(column.values(), np.int64))
    f_ids = Filter(s, S, "allow")
    f_where = Filter.where(s, [(attr, "range", 7, 7)])
    fs = [f_ids, f_where]
    qf = (np.arange(17) % 2).astype(np.int32)

    def check(tag):
        vecs, ids, offsets = _csr_of(s, d)
        cc = dict(c, vecs=vecs, ids=ids, offsets=offsets)
        spec = [(S, "allow"), AY.eval_clauses([("t", "range", 7, 7)], ids, {"t": column})]
        for minc in (3, 25):
            _same(ctx.search_adaptive(parent, s, q, 2, 65, 10, metric, min_candidates=minc, filter=f_ids),
                  _yard(cc, q, 2, 65, minc, 10, spec[:1]), (tag, "ids", minc))
            _same(ctx.search_adaptive(parent, s, q, 2, 65, 10, metric, min_candidates=minc, filter=f_where),
                  _yard(cc, q, 2, 65, minc, 10, spec[1:]), (tag, "where", minc))
            _same(ctx.search_adaptive(parent, s, q, 2, 65, 10, metric, min_candidates=minc, filters=fs, query_filter=qf),
                  _yard(cc, q, 2, 65, minc, 10, spec, qf), (tag, "per query", minc))

    # the counts are derived by the first adaptive call, not by a filtered one
    b0 = [f.info()["device_bytes"] for f in fs]
    ctx.search(parent, s, q, 4, 10, metric, filter=f_ids)
    ctx.search(parent, s, q, 4, 10, metric, filters=fs, query_filter=qf)
    assert [f.info()["device_bytes"] for f in fs] == b0
    check("as built")
    b1 = [f.info()["device_bytes"] for f in fs]
    assert all(b > a for a, b in zip(b0, b1))
    # remove: allowed and other ids (rows swap inside their lists)
    s.remove_ids(np.concatenate([S[:150], c["ids"][::7]]))
    ctx.search(parent, s, q, 4, 10, metric, filter=f_ids)  # a filtered call in between rebuilds the mask only
    check("remove_ids")
    # add_entries that relocates a list: the 17-row list outgrows its extent
    nv = (c["cent"][5] + 0.4 * rng.standard_normal((700, d))).astype(np.float32)
    relocs = s.counters()["list_relocations"]
    s.add_entries(5, new_ids, nv)
    assert s.counters()["list_relocations"] > relocs
    for i in new_ids:
        column.pop(int(i), None)
    check("add_entries")
    # a column update under an unchanged store
    upd = np.concatenate([new_ids[:300], c["ids"][1::11]])
    attr.set(upd, np.full(upd.shape[0], 7, np.int64))
    column.update({int(i): 7 for i in upd})
    check("set_attribute")
    assert f_ids.info()["device_bytes"] >= b1[0]
    for f in fs:
        f.close()
    attr.close()
    s.close()
    parent.close()


# ---- 6. both mirrors -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def test_both_mirrors(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(951)
    n, d, nlist, Q = 6000, 32, 40, 33
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(Q, d, generator=g)
    rng = np.random.default_rng(952)
    sets = [(Y.draw_set(ids.numpy(), 0.2, rng), "allow"), (Y.draw_set(ids.numpy(), 0.01, rng), "allow"), (Y.draw_set(ids.numpy(), 0.5, rng), "deny")]
    qf = torch.from_numpy((np.arange(Q) % 3).astype(np.int64))
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, nlist)
        fl = [idx.make_filter(torch.from_numpy(S), mode == "deny") for S, mode in sets]
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 10, 2
        sp.filter = fl[1]
        r = idx.search(q, sp)
        assert r.nprobed is None  # off by default
        sp.max_nprobe = 2
        assert idx.search(q, sp).nprobed is None and torch.equal(idx.search(q, sp).ids, r.ids)  # max_nprobe == nprobe: the fixed call
        for track in (False, True):
            if name == "python":
                idx.track_hits = track
            else:
                idx.set_track_hits(track)
            for form in ("one", "per query"):
                sp.filter, sp.filters, sp.query_filter = (fl[1], [], None) if form == "one" else (None, fl, qf)
                for mc in (0, 40):
                    sp.max_nprobe, sp.filter_min_candidates = 33, mc
                    r = idx.search(q, sp)
                    rd = idx.search(q.cuda(), sp)
                    assert r.nprobed.dtype == torch.int32 and tuple(r.nprobed.shape) == (Q,) and not r.nprobed.is_cuda and rd.nprobed.is_cuda
                    assert torch.equal(rd.ids.cpu(), r.ids) and torch.equal(rd.distances.cpu(), r.distances)
                    assert torch.equal(rd.nprobed.cpu(), r.nprobed)
                    out[(name, form, mc)] = (r.ids.numpy(), r.distances.numpy(), r.nprobed.numpy(), int(r.timing_info.partitions_scanned))
        if name == "python":
            assert idx._pending_hits and tuple(idx._pending_hits[-1].shape) == (Q, 33) and (idx._pending_hits[-1] == -1).any()
            cent, cids, cv, ci, co = _index_csr(idx)
            for form in ("one", "per query"):
                for mc in (0, 40):
                    oi, od, on, op = A.search(q.numpy(), cent, cv, ci, co, 2, 33, mc or 10, 10, "l2", sets[1:2] if form == "one" else sets,
                                              None if form == "one" else qf.numpy(), centroid_ids=cids)
                    gi, gd, gn, gs = out[(name, form, mc)]
                    _eq(gi, gd, oi, od, (form, mc))
                    np.testing.assert_array_equal(gn, on)
                    assert gs == _pairs_scanned(op, co), (form, mc)  # (no centroid ids given: the yardstick's probed rows are CSR lists)
        idx.maintenance()  # the hit tracker took rows that end in -1
        if name == "python":
            idx.track_hits = False
        else:
            idx.set_track_hits(False)
        # refusals, worded like the filtered ones
        sp.filter, sp.filters, sp.query_filter = None, [], None
        with pytest.raises(RuntimeError, match="max_nprobe needs a filter"):
            idx.search(q, sp)
        sp.filter = fl[0]
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="recall_target"):
            idx.search(q, sp)
        sp.recall_target = -1.0
        sp.nprobe, sp.max_nprobe = 8, 4
        with pytest.raises(RuntimeError, match="max_nprobe=4 is below nprobe=8"):
            idx.search(q, sp)
        sp.nprobe, sp.max_nprobe = 2, 33
        grp = _build(mod, x, ids, nlist, workers=2)
        with pytest.raises(RuntimeError, match="num_workers"):
            grp.search(q, sp)
        sp.filter = None
        with pytest.raises(RuntimeError, match="max_nprobe"):
            grp.search(q, sp)
        sp.max_nprobe = 0
        assert tuple(idx.search(q, sp).ids.shape) == (Q, 10)
    for key in [k for k in out if k[0] == "python"]:
        a, b = out[key], out[("compiled",) + key[1:]]
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        np.testing.assert_array_equal(a[2], b[2])
        assert a[3] == b[3], key  # partitions_scanned: the same quantity in both mirrors


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(ctx, corpora, families):
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Store
    c, s, parent = corpora(8, "l2")
    fam = families(8, "l2")
    q = _queries(c, 4, seed=961)
    f = fam.h[1]
    for kw, code in [(dict(min_candidates=0), "QK_ERR_INVALID.*min_candidates"), (dict(min_candidates=-5), "QK_ERR_INVALID.*min_candidates"),
                     (dict(nprobe=9, max_nprobe=8), "QK_ERR_INVALID.*max_nprobe"), (dict(nprobe=0, max_nprobe=8), "QK_ERR_INVALID.*nprobe"),
                     (dict(k=QK_MAX_K + 1), "QK_ERR_UNSUPPORTED.*QK_MAX_K")]:
        a = dict(nprobe=4, max_nprobe=8, k=10, min_candidates=10)
        a.update(kw)
        with pytest.raises(QuakeHipError, match=code):
            ctx.search_adaptive(parent, s, q, a["nprobe"], a["max_nprobe"], a["k"], "l2", min_candidates=a["min_candidates"], filter=f)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*flat index"):
        ctx.search_adaptive(None, s, q, 4, 8, 10, "l2", filter=f)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID"):
        ctx.search_adaptive(parent, s, q, 4, 8, 10, "l2")  # no filter at all
    # M > QK_MAX_NPROBE: a parent of 8200 lists
    rng = np.random.default_rng(962)
    big = Store(ctx, 8)
    nb = QK_MAX_NPROBE + 8
    big.build_csr(np.array([0, nb], np.int64), np.arange(nb, dtype=np.int64), rng.standard_normal((nb, 8)).astype(np.float32))
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_NPROBE"):
        ctx.search_adaptive(big, s, q, 4, nb, 10, "l2", filter=f)
    big.close()
    want = _yard(c, q, 4, 8, 10, 10, [fam.spec[1]])
    _same(ctx.search_adaptive(parent, s, q, 4, 8, 10, "l2", filter=f), want, "after the refusals")  # (min_candidates defaults to k)
