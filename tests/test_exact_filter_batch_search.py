"""Exact filtered search with one filter per query (qk_search_filtered_exact_batch, qk_store_exact_pool_info,
qk_store_exact_pool_drop; capi.Context.search_exact_batch, capi.Store.exact_pool_info / exact_pool_drop): the candidates of every
filter of a call are a list of the store's candidate pool (k_pool_block_counts, k_pool_block_scan, k_pool_gather), and query i
scans the list of its own filter.

Expected values come from tests/exact_filter_batch_yardstick.py -- the single-filter yardstick under filter qfilter[i], pinned on
the CPU by tests/test_exact_filter_batch_oracle.py -- and every comparison is exact: ids and the uint32 view of the distances.
Every answer is also compared with the single-filter call of each query alone and, for k <= QK_MAX_K, with the all-lists
per-query route qk_search_filtered_batch(parent = NULL).  No test reads a clock."""
import itertools

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import exact_filter_batch_yardstick as B
import filter_yardstick as Y
import nonfinite_yardstick as NF
import oracle as O
from test_adaptive_search import _corpus, _queries, _stores
from test_exact_filter_search import _Filters
from test_filtered_search import _eq, _np
from test_filtered_search import _corpus as _skewed_corpus
from test_filtered_search import _stores as _skewed_stores

pytestmark = pytest.mark.gpu

QK_MAX_K = 448
ZERO = dict(slots=0, rows=0, cap_rows=0, builds=0, evictions=0, device_bytes=0)


def _r16(n):
    return (int(n) + 15) // 16 * 16


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
            c = _corpus(d, metric, seed=700 + d + (1 if metric == "ip" else 0))
            s, parent = _stores(ctx, c)
            cache[(d, metric)] = (c, s, parent)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


@pytest.fixture(scope="module")
def families(corpora):
    cache = {}

    def get(d, metric):
        if (d, metric) not in cache:
            c, s, parent = corpora(d, metric)
            cache[(d, metric)] = _Filters(s, c, seed=29 + d)
        return cache[(d, metric)]

    yield get
    for f in cache.values():
        f.close()


def _check(ctx, s, c, q, k, handles, specs, qf, tag, mem="host", finite=True, single=True, all_lists=True, **kw):
    """the per-query exact call against the yardstick, against the single-filter call of every query alone and, for
    k <= QK_MAX_K, against qk_search_filtered_batch(parent = NULL)"""
    metric = c["metric"]
    qf = np.asarray(qf, np.int32)
    dev = mem == "device"
    x = torch.from_numpy(q).cuda() if dev else q
    qfx = torch.from_numpy(qf).cuda() if dev else qf
    gi, gd = ctx.search_exact_batch(s, x, k, metric, handles, qfx, **kw)
    ctx.synchronize()  # (device buffers are complete behind the context's stream)
    assert "filtered" not in ctx.last_scan_kernel() and "filt" not in ctx.last_scan_kernel(), (tag, ctx.last_scan_kernel())
    oi, od = B.search(q, c["vecs"], c["ids"], c["offsets"], k, metric, specs, qf)
    _eq(gi, gd, oi, od, tag)
    counts = B.candidates(c["ids"], specs)
    if finite:  # (a pair whose value is NaN is no candidate: such a row is shorter)
        want = np.array([min(k, counts[f]) if 0 <= f < len(specs) else 0 for f in qf])
        assert ((_np(gi) >= 0).sum(axis=1) == want).all(), tag
    if single:
        for i, f in enumerate(qf):
            if 0 <= f < len(specs):
                si, sd = ctx.search_exact(s, np.ascontiguousarray(q[i:i + 1]), k, metric, handles[f])
                _eq(_np(gi)[i:i + 1], _np(gd)[i:i + 1], si, sd, (tag, "query alone", i))
    if k <= QK_MAX_K and all_lists:
        ai, ad = ctx.search(None, s, x, 1, k, metric, filters=handles, query_filter=qfx)
        ctx.synchronize()
        _eq(gi, gd, _np(ai), _np(ad), (tag, "all lists"))
    return _np(gi), _np(gd)


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[8, 20, 128], Q=[1, 17, 33], k=[1, 10, 100, 1000], mem=["host", "device"])


def _grid():
    """The full product k x d, three times; metric, Q and the queries' memory rotate over it as in
    test_exact_filter_search.py::_grid (the repetition number in the place of the filter number), so that every pair of values
    of every two axes occurs (checked below)."""
    cases = []
    for rep in range(3):
        for j, (k, d) in enumerate(itertools.product(AXES["k"], AXES["d"])):
            cases.append(dict(metric=AXES["metric"][(j + rep) % 2], d=d, Q=AXES["Q"][(j + rep) % 3], k=k,
                              mem=AXES["mem"][(j // 2 + rep) % 2], n=len(cases)))
    for a, b in itertools.combinations(AXES, 2):
        assert {(c[a], c[b]) for c in cases} == set(itertools.product(AXES[a], AXES[b])), (a, b)
    return cases


def _draw_qfilter(Q, F, n):
    """every filter named when Q allows it; a single query takes the filters in turn with the case number"""
    if Q < F:
        return (np.arange(Q) + n) % F
    rng = np.random.default_rng(n)
    return rng.permutation(np.concatenate([np.arange(F), rng.integers(0, F, size=Q - F)]))


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, families, case):
    c, s, parent = corpora(case["d"], case["metric"])
    fam = families(case["d"], case["metric"])
    q = _queries(c, case["Q"], seed=7 + case["Q"])
    qf = _draw_qfilter(case["Q"], len(fam.h), case["n"])
    if case["Q"] >= len(fam.h):
        assert set(qf) == set(range(len(fam.h)))
    _check(ctx, s, c, q, case["k"], fam.h, fam.spec, qf, tag=case, mem=case["mem"])
    assert s.exact_pool_info()["slots"] == len(fam.h)  # every filter of the call is admitted, named or not


# ---- 2. the gather's edges, all in one admission -------------------------------------------------------------------------------
def _flat_corpus(sizes, d, seed, metric="l2"):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    offsets = np.zeros(sizes.shape[0] + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 2 + 1
    return dict(vecs=vecs, ids=ids, offsets=offsets, d=d, metric=metric)


def _store_of(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    return s


def _csr_of(s, d):
    lists = sorted(int(p) for p in s.list_ids())
    pv, pi = zip(*[s.get_list(p) for p in lists])
    return O.csr_from_partitions(pv, pi, d)


def test_gather_edges(ctx):
    """1, 15, 16, 17 and 1025 candidates; candidates on both sides of a 1024-row scan block boundary; candidates only in the
    last, partial tile of the arena; a whole list of exactly 16 rows; two filters with the same id set (two slots); one handle
    listed twice (one slot); a filter without candidates -- F = 12 in ONE admission, k = 20 longer than some slots"""
    from quake_amd.capi import Filter
    # lists in arena order (every extent is the list rounded up to a tile): rows 0 .. 1007, 1008 .. 1023, 1024 .. 1063, ...
    c = _flat_corpus([1000, 16, 40, 2000, 7], 20, seed=31)
    s = _store_of(ctx, c)
    o, ids = c["offsets"], c["ids"]
    rng = np.random.default_rng(32)
    sets = [rng.permutation(ids)[:m] for m in (1, 15, 16, 17, 1025)]
    sets.append(np.concatenate([ids[o[1] + 12:o[2]], ids[o[2]:o[2] + 4]]))  # arena rows 1020 .. 1027
    sets.append(ids[o[4]:o[5]])                                            # the last tile of the arena, 7 of 16 rows
    sets.append(ids[o[1]:o[2]])                                            # a whole list of one full tile
    twin = rng.permutation(ids)[:100]
    sets += [twin, twin.copy()]
    handles = [Filter(s, S, "allow") for S in sets]
    handles.append(handles[3])  # the same handle again
    sets.append(sets[3])
    handles.append(Filter(s, np.zeros(0, np.int64), "allow"))
    sets.append(np.zeros(0, np.int64))
    assert len(handles) == 12
    specs = [(S, "allow") for S in sets]
    q = rng.standard_normal((24, 20)).astype(np.float32)
    qf = np.arange(24) % 12
    assert s.exact_pool_info() == ZERO
    gi, gd = _check(ctx, s, c, q, 20, handles, specs, qf, "edges")
    info = s.exact_pool_info()
    assert info["slots"] == 11 and info["builds"] == 11 and info["evictions"] == 0, info
    assert info["rows"] == sum(_r16(S.shape[0]) for S in sets[:10]) and info["cap_rows"] >= info["rows"], info
    # the twins answer alike: the same queries under either
    a = _check(ctx, s, c, q, 20, handles, specs, np.full(24, 8), "twin a", mem="device")
    b = _check(ctx, s, c, q, 20, handles, specs, np.full(24, 9), "twin b", mem="device")
    _eq(a[0], a[1], b[0], b[1], "twins")
    assert s.exact_pool_info() == info  # nothing was gathered again
    for f in handles[:10] + handles[11:]:
        f.close()
    assert s.exact_pool_info()["slots"] == 0
    s.close()


# ---- 3. many filters -----------------------------------------------------------------------------------------------------------
def test_many_filters(ctx, corpora):
    """F = 130 predicates tenant == t in ONE admission: some tenants are empty, a tenth of the ids carry no value"""
    from quake_amd.capi import Attr, Filter
    c, s, parent = corpora(20, "l2")
    s.exact_pool_drop()
    rng = np.random.default_rng(41)
    ids = c["ids"]
    have = rng.permutation(ids)[: int(0.9 * ids.shape[0])]
    tenants = rng.permutation(130)[:115]  # 15 tenants without a row
    column = {int(i): int(v) for i, v in zip(have, rng.choice(tenants, size=have.shape[0]))}
    attr = Attr(s)
    attr.set(np.fromiter(column.keys(), np.int64), np.fromiter(column.values(), np.int64))
    handles = [Filter.where(s, [(attr, "range", t, t)]) for t in range(130)]
    specs = [(ids[AY.eval_clauses([("tenant", "range", t, t)], ids, {"tenant": column})], "allow") for t in range(130)]
    counts = B.candidates(ids, specs)
    assert counts.count(0) == 15 and sum(counts) == have.shape[0]
    q = _queries(c, 64, seed=42)
    qf = rng.integers(0, 130, size=64)
    qf[:3] = [int(np.argmin(counts)), int(np.argmax(counts)), 129]
    _check(ctx, s, c, q, 10, handles, specs, qf, "130 tenants", single=False)
    info = s.exact_pool_info()
    assert info["slots"] == 130 and info["builds"] == 130, info  # `builds` counts slots gathered: one per filter admitted
    assert info["rows"] == sum(_r16(n) for n in counts)
    _check(ctx, s, c, q, 10, handles, specs, qf, "130 tenants, device", mem="device", all_lists=False)
    assert s.exact_pool_info() == info
    for f in handles:
        f.close()
    attr.close()
    assert s.exact_pool_info()["slots"] == 0
    s.exact_pool_drop()


# ---- 4. wide rows ----------------------------------------------------------------------------------------------------------------
def test_wide_rows(ctx):
    """the smallest d whose scan reads the queries from global memory (k_scan_wide)"""
    from quake_amd.capi import Filter
    d = 2560
    c = _skewed_corpus(d, 24, 2000, "l2", seed=51)
    s, parent = _skewed_stores(ctx, c)
    q = np.ascontiguousarray(c["x"][:5] + 0.01)
    rng = np.random.default_rng(53)
    specs = [(Y.draw_set(c["ids"], sel, rng), "allow") for sel in (0.1, 0.02, 0.4)]
    handles = [Filter(s, S, m) for S, m in specs]
    _check(ctx, s, c, q, 10, handles, specs, [0, 1, 2, 1, 0], "wide", all_lists=False)
    assert "wide" in ctx.last_scan_kernel(), ctx.last_scan_kernel()
    for f in handles:
        f.close()
    s.close()
    parent.close()


# ---- 5. slots persist across calls with other filter lists ----------------------------------------------------------------------
def test_persistence(ctx, corpora):
    from quake_amd.capi import Filter
    c, s, parent = corpora(20, "l2")
    s.exact_pool_drop()
    rng = np.random.default_rng(61)
    specs = [(rng.permutation(c["ids"])[:m], "allow") for m in (300, 40, 3000)]
    A, Bf, Cf = [Filter(s, S, m) for S, m in specs]
    q = _queries(c, 17, seed=62)
    qf2 = np.arange(17) % 2
    _check(ctx, s, c, q, 10, [A, Bf], specs[:2], qf2, "[A, B]")
    info = s.exact_pool_info()
    assert info["builds"] == 2 and info["slots"] == 2 and info["rows"] == _r16(300) + _r16(40)
    _check(ctx, s, c, q, 10, [A, Bf], specs[:2], qf2, "[A, B] again", single=False)
    assert s.exact_pool_info() == info
    _check(ctx, s, c, q, 10, [Bf, Cf], specs[1:], qf2, "[B, C]")
    info2 = s.exact_pool_info()
    assert info2["builds"] == 3 and info2["slots"] == 3, info2  # exactly C was gathered
    assert info2["cap_rows"] > info["cap_rows"]  # (3000 rows did not fit the first arena: the pool was repacked)
    _check(ctx, s, c, q, 10, [A], specs[:1], np.zeros(17, np.int32), "[A] behind the repack")
    assert s.exact_pool_info() == info2
    for f in (A, Bf, Cf):
        assert f.exact_info()["builds"] == 1  # (the single-filter comparisons of _check; batch calls never touch it)
        f.close()
    s.exact_pool_drop()


# ---- 6. store changes ------------------------------------------------------------------------------------------------------------
def test_store_changes(ctx):
    """add, remove_ids, set_attribute, a relocation and refine_lists: the next call follows the ids, and every filter whose mask
    was rebuilt is gathered again -- all of them after a store change (the mask is stamped with the store's version), only the
    predicate after a column change"""
    from quake_amd.capi import Attr, Filter
    d = 20
    c = _flat_corpus([300, 40, 900, 0, 130], d, seed=9)
    s = _store_of(ctx, c)
    rng = np.random.default_rng(10)
    q = rng.standard_normal((17, d)).astype(np.float32)
    SA = np.concatenate([rng.permutation(c["ids"])[:200], np.arange(10 ** 6, 10 ** 6 + 3000, 3)]).astype(np.int64)
    SB = rng.permutation(c["ids"])[:150]
    col = {int(i): int(i) % 7 for i in c["ids"]}
    attr = Attr(s)
    attr.set(np.fromiter(col.keys(), np.int64), np.fromiter(col.values(), np.int64))
    handles = [Filter(s, SA, "allow"), Filter(s, SB, "allow"), Filter.where(s, [(attr, "range", 2, 3)])]
    qf = np.arange(17) % 3
    builds = [0]

    def check(tag, gathered):
        vecs, ids, offsets = _csr_of(s, d)
        cur = dict(c, vecs=vecs, ids=ids, offsets=offsets)
        wS = np.array([i for i in ids if col.get(int(i), -1) in (2, 3)], np.int64)
        specs = [(SA, "allow"), (SB, "allow"), (wS, "allow")]
        exact = [f.exact_info() for f in handles]
        for again in (False, True):
            _check(ctx, s, cur, q, 10, handles, specs, qf, (tag, again), single=False)
            builds[0] += 0 if again else gathered
            info = s.exact_pool_info()
            assert info["builds"] == builds[0] and info["slots"] == 3, (tag, again, info)
            assert info["rows"] == sum(_r16(n) for n in B.candidates(ids, specs))
        assert [f.exact_info() for f in handles] == exact  # the private candidate stores are not touched by batch calls
        return cur, specs

    check("as built", 3)
    check("nothing changed", 0)
    nid = np.arange(10 ** 6, 10 ** 6 + 600, dtype=np.int64)  # a third of them are in A; the list outgrows its extent
    moved = s.counters()["list_relocations"]
    s.add_entries(1, nid, rng.standard_normal((600, d)).astype(np.float32))
    assert s.counters()["list_relocations"] > moved
    check("add (relocating)", 3)
    s.remove_ids(SB[:60])
    check("remove_ids", 3)
    flip = c["ids"][:200]
    flip = flip[~np.isin(flip, SB[:60])]
    attr.set(flip, np.full(flip.shape[0], 2, np.int64))
    col.update({int(i): 2 for i in flip})
    check("set_attribute", 1)  # the store did not change: only the predicate's mask was rebuilt
    cent = rng.standard_normal((2, d)).astype(np.float32)
    s.refine_lists(np.array([0, 2], np.int64), cent, "l2", 1)
    s.publish()
    cur, specs = check("refine_lists + publish", 3)
    _check(ctx, s, cur, q, 10, handles, specs, qf, "single-filter calls too")
    for f in handles:
        f.close()
    attr.close()
    s.close()


# ---- 7. the budget ---------------------------------------------------------------------------------------------------------------
def test_budget(ctx, corpora):
    from quake_amd.capi import Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(20, "l2")
    s.exact_pool_drop()
    rng = np.random.default_rng(71)
    sizes = [100, 200, 300, 400, 250]
    specs = [(rng.permutation(c["ids"])[:m], "allow") for m in sizes]
    h = [Filter(s, S, m) for S, m in specs]
    r = [_r16(m) for m in sizes]  # 112, 208, 304, 400, 256
    q = _queries(c, 17, seed=72)

    def call(idx, pool_rows, tag, **kw):
        qf = np.arange(17) % len(idx)
        return _check(ctx, s, c, q, 10, [h[i] for i in idx], [specs[i] for i in idx], qf, tag, single=False, all_lists=False,
                      pool_rows=pool_rows, **kw)

    budget = r[0] + r[1] + r[2] + r[3]
    call([0], budget, "A")
    call([1], budget, "B")
    call([2, 3], budget, "C D")
    call([0], budget, "A again")  # A is now named later than B
    info = s.exact_pool_info()
    assert info == dict(info, slots=4, rows=budget, builds=4, evictions=0)
    call([4], budget, "E")  # 256 rows: B (208, least recently named) and then C (lower slot of the tie C / D) go
    info = s.exact_pool_info()
    assert info["evictions"] == 2 and info["slots"] == 3 and info["rows"] == r[0] + r[3] + r[4] and info["builds"] == 5, info
    call([0, 3, 4], budget, "the survivors")
    assert s.exact_pool_info() == info
    call([1], budget, "B is gathered again")
    info = s.exact_pool_info()
    assert info["builds"] == 6 and info["evictions"] == 2 and info["rows"] == r[0] + r[1] + r[3] + r[4], info
    # the call's own filters exceed pool_rows: refused, the pool unchanged
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*pool_rows"):
        call([2, 3, 4], r[2] + r[3] + r[4] - 1, "too many")
    assert s.exact_pool_info() == info
    # max_rows one below a filter's count: refused naming the index, nothing changed
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*filter 1 of 2.*max_rows"):
        call([0, 2], 0, "max_rows", max_rows=299)
    assert s.exact_pool_info() == info
    call([0, 2], 0, "max_rows = rows", max_rows=300)
    # an arena that grew without a bound comes back under the bound of a later call
    call([0, 1, 2, 3, 4], 0, "no bound")
    assert s.exact_pool_info()["cap_rows"] > 1024 and s.exact_pool_info()["rows"] == sum(r)
    call([0], r[0], "a smaller budget")
    info = s.exact_pool_info()
    assert info["slots"] == 1 and info["rows"] == r[0] and info["cap_rows"] <= 1024, info
    s.exact_pool_drop()
    # two disjoint sets alternate under a budget that holds one of them
    sets = ([0, 1, 2], [3, 4])
    budget = max(sum(r[i] for i in st) for st in sets)
    for step in range(20):
        st = sets[step % 2]
        call(st, budget, ("alternating", step))
        info = s.exact_pool_info()
        assert info["cap_rows"] <= max(2 * budget, 1024) and info["rows"] <= budget, (step, info)
        assert info["slots"] == len(st) and info["builds"] == sum(len(sets[t % 2]) for t in range(step + 1)), (step, info)
    for f in h:
        f.close()
    s.exact_pool_drop()


# ---- 8. drop, destroy --------------------------------------------------------------------------------------------------------------
def test_drop_and_destroy(ctx, corpora):
    from quake_amd.capi import Filter
    c, s, parent = corpora(20, "ip")
    s.exact_pool_drop()
    rng = np.random.default_rng(81)
    specs = [(rng.permutation(c["ids"])[:m], "allow") for m in (500, 260, 250)]
    h = [Filter(s, S, m) for S, m in specs]
    q = _queries(c, 17, seed=82)
    qf = np.arange(17) % 2
    _check(ctx, s, c, q, 10, h[:2], specs[:2], qf, "first")
    assert s.exact_pool_info()["builds"] == 2
    s.exact_pool_drop()
    assert s.exact_pool_info() == ZERO
    _check(ctx, s, c, q, 10, h[:2], specs[:2], qf, "behind the drop", single=False)
    info = s.exact_pool_info()
    assert info["builds"] == 2 and info["slots"] == 2
    h[1].close()  # 272 rows come back ...
    after = s.exact_pool_info()
    assert after["slots"] == 1 and after["rows"] == _r16(500) and after["cap_rows"] == info["cap_rows"]
    _check(ctx, s, c, q, 10, [h[0], h[2]], [specs[0], specs[2]], qf, "the extent is used again", single=False)
    again = s.exact_pool_info()  # ... and take the 256 of the next admission
    assert again["slots"] == 2 and again["cap_rows"] == info["cap_rows"] and again["device_bytes"] == info["device_bytes"]
    h[0].close()
    h[2].close()
    assert s.exact_pool_info()["slots"] == 0 and s.exact_pool_info()["rows"] == 0
    s.exact_pool_drop()


# ---- 9. qfilter out of range ---------------------------------------------------------------------------------------------------
def test_qfilter_out_of_range(ctx, corpora, families):
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(20, "l2")
    fam = families(20, "l2")
    F = len(fam.h)
    q = _queries(c, 17, seed=91)
    qf = np.arange(17) % F
    qf[[2, 9]] = [-1, F]
    gi, gd = _check(ctx, s, c, q, 10, fam.h, fam.spec, qf, "device qfilter", mem="device", all_lists=False)
    assert (gi[[2, 9]] == -1).all() and np.isposinf(gd[[2, 9]]).all() and (gi[0] >= 0).all()
    for bad in (-1, F):
        qf[2] = bad
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*qfilter"):
            ctx.search_exact_batch(s, q, 10, "l2", fam.h, qf)


def test_refusals_of_the_c_abi(ctx, corpora, families):
    from quake_amd.capi import Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(20, "l2")
    c2, s2, parent2 = corpora(8, "l2")
    fam = families(20, "l2")
    q = _queries(c, 5, seed=92)
    qf = np.zeros(5, np.int32)
    f2 = Filter(s2, c2["ids"][:100], "allow")
    before = s.exact_pool_info()
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search_exact_batch(s, q, 10, "l2", [fam.h[0], f2], qf)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*null"):
        ctx.search_exact_batch(s, q, 10, "l2", [fam.h[0], None], qf)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*max_rows"):
        ctx.search_exact_batch(s, q, 10, "l2", fam.h, qf, max_rows=-1)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*pool_rows"):
        ctx.search_exact_batch(s, q, 10, "l2", fam.h, qf, pool_rows=-1)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID"):
        ctx.search_exact_batch(s, q, 0, "l2", fam.h, qf)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED"):
        ctx.search_exact_batch(s, q, 8193, "l2", fam.h, qf)
    assert s.exact_pool_info() == before
    _check(ctx, s, c, q, 8192, fam.h, fam.spec, np.arange(5) % len(fam.h), "k = 8192", single=False)
    f2.close()


# ---- 10. two contexts ------------------------------------------------------------------------------------------------------------
def test_two_contexts(ctx, corpora, families):
    from quake_amd.capi import Context
    c, s, parent = corpora(8, "ip")
    fam = families(8, "ip")
    s.exact_pool_drop()
    q = _queries(c, 33, seed=101)
    qf = _draw_qfilter(33, len(fam.h), 0)
    _check(ctx, s, c, q, 10, fam.h, fam.spec, qf, "admitted here", single=False)
    info = s.exact_pool_info()
    other = Context(0)
    try:
        _check(other, s, c, q, 10, fam.h, fam.spec, qf, "searched there", mem="device", single=False)
        assert s.exact_pool_info() == info
    finally:
        other.close()


# ---- 11. non-finite values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["nan", "inf"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_nonfinite_candidates(ctx, cls, metric):
    """NaN rows and +-inf rows among the candidates of two filters: the search contract, unchanged"""
    from quake_amd.capi import Filter, Store
    c = NF.corpus(cls, metric, 6000, 12, 24, seed=16)
    s = Store(ctx, 24)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    q, _ = NF.queries(c, 17, seed=17)
    rng = np.random.default_rng(18)
    planted = c["ids"][c["special"]]
    specs = [(np.union1d(Y.draw_set(c["ids"], 0.2, rng), planted), "allow"), (np.setdiff1d(Y.draw_set(c["ids"], 0.3, rng), planted[::2]), "deny")]
    handles = [Filter(s, S, m) for S, m in specs]
    cc = dict(c, metric=metric)
    for k in (1, 10, 100):
        _check(ctx, s, cc, q, k, handles, specs, np.arange(17) % 2, (cls, metric, k), finite=False)
    for f in handles:
        f.close()
    s.close()


# ---- 12. both mirrors --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def _mirror_data():
    g = torch.Generator().manual_seed(121)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(33, d, generator=g)
    # tenants 0 .. 5 of about 40, 80, 160, 600, 1500 and 3600 rows
    bounds = np.cumsum([0, 40, 80, 160, 600, 1500, n - 2380])
    tenant = torch.from_numpy(np.repeat(np.arange(6), np.diff(bounds)))[torch.randperm(n, generator=g)]
    return x, ids, q, tenant


def test_both_mirrors(qb):
    import quake_amd as quake
    from test_filtered_search import _build
    x, ids, q, tenant = _mirror_data()
    Q = q.shape[0]
    qf = torch.arange(Q, dtype=torch.int32) % 6
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, 20)
        idx.set_attribute("tenant", ids, tenant)
        sp = mod.SearchParams()
        assert sp.filters_exact_rows == 0 and sp.filters_exact_pool_rows == 0
        before = repr(sp)
        sp.k, sp.nprobe = 10, 3
        flts = [idx.make_filter(where=[("tenant", "==", t)]) for t in range(6)]
        sp.filters, sp.query_filter = flts, qf
        today = idx.search(q, sp)
        assert today.exact_mask is None
        rows = [int(f.info()["rows_allowed"]) for f in flts]
        assert rows == sorted(rows) and rows[2] < 200 < rows[3]

        def check(tag, mx, qfilter, xq):
            sp.max_nprobe = mx
            sp.filters_exact_rows, sp.query_filter = 200, qfilter
            r = idx.search(xq, sp)
            counts = [int(f.info()["rows_allowed"]) for f in flts]
            want = torch.tensor([counts[int(t)] <= 200 for t in qf])
            assert r.exact is False and r.exact_mask.dtype == torch.bool and torch.equal(r.exact_mask.cpu(), want), tag
            assert r.exact_mask.is_cuda == xq.is_cuda and r.ids.is_cuda == xq.is_cuda
            one = mod.SearchParams()
            one.k, one.nprobe, one.max_nprobe = sp.k, sp.nprobe, mx
            for i in range(Q):
                t = int(qf[i])
                if want[i]:  # the single-filter exact call of that query alone
                    one.filter, one.filter_exact_rows, one.filters, one.query_filter = flts[t], 200, [], None
                else:        # the per-query probed search of that query alone
                    one.filter, one.filter_exact_rows, one.filters, one.query_filter = None, 0, flts, qf[i:i + 1]
                a = idx.search(q[i:i + 1], one)
                assert (a.exact is True) == bool(want[i])
                assert torch.equal(r.ids[i].cpu(), a.ids[0]) and torch.equal(r.distances[i].cpu().view(torch.int32), a.distances[0].view(torch.int32)), (tag, i)
            sp.filters_exact_rows = 0
            return r

        for mx in (0, 12):
            r = check((name, "host", mx), mx, qf, q)
            rd = check((name, "device", mx), mx, qf.cuda(), q.cuda())
            assert torch.equal(rd.ids.cpu(), r.ids) and torch.equal(rd.distances.cpu(), r.distances)
            assert (r.nprobed is None) == (mx == 0)
            if mx:
                assert (r.nprobed[r.exact_mask] == 0).all() and (r.nprobed[~r.exact_mask] >= 3).all()
            out[(name, mx)] = (r.ids.numpy(), r.distances.numpy())
        # through add / remove / maintenance
        g = torch.Generator().manual_seed(122)
        new_ids = torch.arange(100000, 100150)
        idx.add(torch.randn(150, 32, generator=g), new_ids)
        idx.set_attribute("tenant", new_ids, torch.full((150,), 2))  # tenant 2 now has more than 200 rows
        idx.remove(ids[tenant == 4][:1400])                           # ... and tenant 4 fewer
        idx.maintenance()
        r = check((name, "after changes"), 0, qf, q)
        assert not r.exact_mask[2] and r.exact_mask[4]
        out[(name, "changed")] = (r.ids.numpy(), r.distances.numpy())
        # hit tracking: only the probed queries leave hits (last: the policy of this mirror alone sees them)
        if name == "python":
            idx._flush_hits()
            idx.track_hits = True
            sp.max_nprobe, sp.filters_exact_rows, sp.query_filter = 0, 200, qf
            r = idx.search(q, sp)
            assert len(idx._pending_hits) == 1 and idx._pending_hits[0].shape[0] == int((~r.exact_mask).sum())
            idx._flush_hits()
            idx.track_hits = False
            sp.filters_exact_rows = 0
        assert "filters_exact" not in before and repr(mod.SearchParams()) == before
    for key in ((0,), (12,), ("changed",)):
        a, b = out[("python",) + key], out[("compiled",) + key]
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_mirror_refusals(qb):
    import quake_amd as quake
    from test_filtered_search import _build
    g = torch.Generator().manual_seed(71)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        plain = idx.search(qq, sp)
        sp.filters_exact_rows = 100
        with pytest.raises(RuntimeError, match="filters_exact_rows needs filters and query_filter"):
            idx.search(qq, sp)
        f = idx.make_filter(ids[:50])
        sp.filter = f
        with pytest.raises(RuntimeError, match="filters_exact_rows is not supported with filter"):
            idx.search(qq, sp)
        sp.filter = None
        sp.filters, sp.query_filter = [f], torch.zeros(10, dtype=torch.int32)
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="filters_exact_rows.*recall_target"):
            idx.search(qq, sp)
        sp.recall_target = -1.0
        for call in (lambda: idx.search_after(qq, sp), lambda: idx.range_search(qq, 1.0, sp)):
            with pytest.raises(RuntimeError):
                call()
        idx.set_attribute("g", ids, ids % 5)
        with pytest.raises(RuntimeError):
            idx.grouped_search(qq, "g", sp)
        sp.filters, sp.query_filter = [], None
        for call in (lambda: idx.search_after(qq, sp), lambda: idx.range_search(qq, 1.0, sp), lambda: idx.grouped_search(qq, "g", sp)):
            with pytest.raises(RuntimeError, match="filters_exact_rows"):
                call()
        sp.filters, sp.query_filter = [f], torch.zeros(10, dtype=torch.int32)
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="filters_exact_rows.*num_workers"):
            grp.search(qq, sp)
        for field in ("filters_exact_rows", "filters_exact_pool_rows"):
            setattr(sp, field, -1)
            with pytest.raises(RuntimeError, match="filters_exact_rows"):
                idx.search(qq, sp)
            setattr(sp, field, 100)
        sp.filters_exact_rows, sp.filter_exact_rows = 0, 100  # the refusal of the single-filter field stays
        with pytest.raises(RuntimeError, match="filter_exact_rows.*query_filter"):
            idx.search(qq, sp)
        sp.filters_exact_rows, sp.filter_exact_rows = 100, 0
        r = idx.search(qq, sp)  # the index still answers, and exactly
        assert r.exact_mask.all() and int((r.ids >= 0).sum()) == 10 * 5
        sp.filters, sp.query_filter, sp.filters_exact_rows, sp.filters_exact_pool_rows = [], None, 0, 0
        again = idx.search(qq, sp)
        assert torch.equal(again.ids, plain.ids) and torch.equal(again.distances, plain.distances)
