"""Exact filtered search (qk_search_filtered_exact, qk_filter_candidate_rows, qk_filter_exact_info; capi.Context.search_exact;
SearchParams.filter_exact_rows / SearchResult.exact in both mirrors): the candidates of a filter are compacted on the device into
a one-list store (k_filter_block_counts, k_filter_block_scan, k_filter_gather) and searched flat.

Expected values come from tests/exact_filter_yardstick.py -- the filter yardstick with every list probed, pinned on the CPU by
tests/test_exact_filter_oracle.py -- and every comparison is exact: ids and the uint32 view of the distances.  For k <= QK_MAX_K
the answer is also compared with the all-lists route qk_search_filtered(parent = NULL) on the same store.  No test reads a clock."""
import numpy as np
import pytest
import torch

import attr_yardstick as AY
import exact_filter_yardstick as E
import filter_yardstick as Y
import nonfinite_yardstick as NF
import oracle as O
from test_adaptive_search import _corpus, _queries, _stores
from test_filtered_search import _build, _eq, _np
from test_filtered_search import _corpus as _skewed_corpus
from test_filtered_search import _stores as _skewed_stores

pytestmark = pytest.mark.gpu

QK_MAX_K = 448
SCAN_BLOCK_WORDS = 64  # k_filter_block_counts: a scan block is 64 mask words = 1024 arena rows
DENSE = ("k_dense", "k_dense_fused", "k_dense_pf", "k_dense_wide", "k_assign_pf")


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
            c = _corpus(d, metric, seed=500 + d + (1 if metric == "ip" else 0))
            s, parent = _stores(ctx, c)
            cache[(d, metric)] = (c, s, parent)
        return cache[(d, metric)]

    yield get
    for c, s, p in cache.values():
        s.close()
        p.close()


class _Filters:
    """the filter family over one corpus as yardstick filters (`spec`: id set and mode) and as handles of the store (`h`)"""
    NAMES = ["allow0.5", "allow0.01", "range", "deny0.3", "where", "empty", "all"]

    def __init__(self, s, c, seed):
        from quake_amd.capi import Attr, Filter
        rng = np.random.default_rng(seed)
        ids = c["ids"]
        lo, hi = int(np.quantile(ids, 0.4)), int(np.quantile(ids, 0.55))
        self.spec = [(Y.draw_set(ids, 0.5, rng), "allow"), (Y.draw_set(ids, 0.01, rng), "allow"),
                     (np.arange(lo, hi + 1, dtype=np.int64), "allow"), (Y.draw_set(ids, 0.3, rng), "deny")]
        self.h = [Filter(s, S, mode) for S, mode in self.spec]
        have = rng.permutation(ids)[: int(0.9 * ids.shape[0])]
        self.column = {int(i): int(v) for i, v in zip(have, rng.integers(0, 20, size=have.shape[0]))}
        self.attr = Attr(s)
        self.attr.set(np.fromiter(self.column.keys(), np.int64), np.fromiter(self.column.values(), np.int64))
        self.spec.append((ids[AY.eval_clauses([("tenant", "range", 3, 4)], ids, {"tenant": self.column})], "allow"))
        self.h.append(Filter.where(s, [(self.attr, "range", 3, 4)]))
        self.spec += [(np.zeros(0, np.int64), "allow"), (np.zeros(0, np.int64), "deny")]
        self.h += [Filter(s, S, mode) for S, mode in self.spec[-2:]]

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
            cache[(d, metric)] = _Filters(s, c, seed=23 + d)
        return cache[(d, metric)]

    yield get
    for f in cache.values():
        f.close()


def _check(ctx, s, c, q, k, f, S, mode, tag, mem="host", all_lists=True, finite=True):
    """the exact call against the yardstick and, for k <= QK_MAX_K, against qk_search_filtered(parent = NULL)"""
    metric = c["metric"]
    x = torch.from_numpy(q).cuda() if mem == "device" else q
    gi, gd = ctx.search_exact(s, x, k, metric, f)
    ctx.synchronize()  # (device buffers are complete behind the context's stream)
    assert ctx.last_scan_kernel() in DENSE, (tag, ctx.last_scan_kernel())
    oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], k, metric, S, mode)
    _eq(gi, gd, oi, od, tag)
    n = E.candidates(c["ids"], S, mode)
    assert f.candidate_rows(ctx) == n and f.exact_info()["rows"] == n, tag
    if finite:  # (a pair whose value is NaN is no candidate: such a row is shorter)
        assert ((_np(gi) >= 0).sum(axis=1) == min(k, n)).all(), tag
    if k <= QK_MAX_K and all_lists:
        ai, ad = ctx.search(None, s, x, 1, k, metric, filter=f)
        ctx.synchronize()
        _eq(gi, gd, _np(ai), _np(ad), (tag, "all lists"))
    return gi, gd


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
AXES = dict(metric=["l2", "ip"], d=[8, 20, 128], Q=[1, 17, 33], k=[1, 10, 100, 1000], flt=_Filters.NAMES, mem=["host", "device"])


def _grid():
    """The full product filter x k x d (84 cases on the six module-scoped corpora).  Metric, Q and the queries' memory rotate over
    it, case j of filter number fi taking element j + fi, j // 2 + fi and j + fi of those axes, so that every pair of values of
    every two axes occurs as well (checked below); triples beyond filter x k x d are not all covered."""
    import itertools
    cases = []
    for fi, flt in enumerate(AXES["flt"]):
        for j, (k, d) in enumerate(itertools.product(AXES["k"], AXES["d"])):
            cases.append(dict(metric=AXES["metric"][(j + fi) % 2], d=d, Q=AXES["Q"][(j + fi) % 3], k=k, flt=flt,
                              mem=AXES["mem"][(j // 2 + fi) % 2]))
    for a, b in itertools.combinations(AXES, 2):
        assert {(c[a], c[b]) for c in cases} == set(itertools.product(AXES[a], AXES[b])), (a, b)
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, families, case):
    c, s, parent = corpora(case["d"], case["metric"])
    fam = families(case["d"], case["metric"])
    i = _Filters.NAMES.index(case["flt"])
    q = _queries(c, case["Q"], seed=7 + case["Q"])
    _check(ctx, s, c, q, case["k"], fam.h[i], *fam.spec[i], tag=case, mem=case["mem"])


# ---- 2. destination tiles, the prefix sum, the forms of the flat search -----------------------------------------------------------
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


def test_destination_tiles(ctx):
    """exactly 1, 16, 17, 31 and 32 candidates (one and two destination tiles, full and partial), and the only candidate in row 15
    of the last live tile of the arena"""
    from quake_amd.capi import Filter
    c = _flat_corpus([40, 0, 64], 8, seed=1)  # the last list is four full tiles: its last row is row 15 of the last live tile
    s = _store_of(ctx, c)
    q = np.random.default_rng(2).standard_normal((17, 8)).astype(np.float32)
    rng = np.random.default_rng(3)
    sets = [rng.permutation(c["ids"])[:m] for m in (1, 16, 17, 31, 32)] + [c["ids"][-1:], c["ids"][:1]]
    for S in sets:
        f = Filter(s, S, "allow")
        for k in (1, 10, 100):
            _check(ctx, s, c, q, k, f, S, "allow", (S.shape[0], k))
        f.close()
    s.close()


def test_prefix_sum_across_blocks(ctx):
    """a d = 8 store whose mask spans three scan blocks (64 words = 1024 rows each) plus one word: candidates only in the first and
    the last block, only in the first and the odd word behind the third, only in the middle block"""
    from quake_amd.capi import Filter
    rows = SCAN_BLOCK_WORDS * 16
    c = _flat_corpus([rows, rows, rows, 16], 8, seed=4)
    s = _store_of(ctx, c)
    o = c["offsets"]
    q = np.random.default_rng(5).standard_normal((17, 8)).astype(np.float32)
    every = Filter(s, c["ids"], "allow")
    words = 3 * SCAN_BLOCK_WORDS + 1  # the arena is exactly the lists: one mask word per tile
    assert every.info()["device_bytes"] == (words + words // 4) * 2 + c["ids"].shape[0] * 8 + 8
    every.close()
    pick = lambda p, idx: c["ids"][o[p] + np.asarray(idx)]
    cases = {"first and last block": np.concatenate([pick(0, [0, 5, 1023]), pick(2, [0, 17, 1000, 1023])]),
             "first block and the odd word": np.concatenate([pick(0, [3, 700]), pick(3, [0, 15])]),
             "the odd word only": pick(3, [7]),
             "middle block": pick(1, list(range(0, 1024, 37)) + [1023]),
             "every block, every row": c["ids"]}
    for name, S in cases.items():
        f = Filter(s, S, "allow")
        _check(ctx, s, c, q, 10, f, S, "allow", name)
        f.close()
    s.close()


@pytest.mark.parametrize("m", [1023, 1024, 1025, 4095, 4096, 4097])
def test_form_boundaries(ctx, corpora, m):
    """candidate counts just below and above 1024 and 4096 rows, where the dense forms of the flat search change"""
    from quake_amd.capi import Filter
    c, s, parent = corpora(128, "l2")
    S = np.random.default_rng(m).permutation(c["ids"])[:m]
    f = Filter(s, S, "allow")
    q = _queries(c, 33, seed=m)
    for k in (1, 10, 100):
        _check(ctx, s, c, q, k, f, S, "allow", (m, k), all_lists=(k == 10))
    # (the fused and the prefiltered form ask for 64 queries, and up to 256 queries a one-launch form takes short lists; with 257
    # queries and k = 64 the form changes at 1024 and behind 4096 rows)
    _check(ctx, s, c, _queries(c, 257, seed=m + 1), 64, f, S, "allow", (m, 64, "257 queries"), all_lists=False)
    assert ctx.last_scan_kernel() == ("k_dense" if m < 1024 else "k_dense_fused" if m <= 4096 else "k_dense_pf")
    f.close()


def test_rebuild_behind_the_row_major_copy(ctx):
    """5000 candidates x 128 and 96 queries go through k_dense_pf, whose exact finish reads a row-major copy of the one list.  Then
    300 candidates leave (rows of the first answer among them) and 300 arrive next to the queries: the rebuilt list has the same
    place and the same length, so only dropping the copy with the rebuild keeps the second answer right."""
    from quake_amd.capi import Filter
    d = 128
    c = _flat_corpus([3000, 4000, 1000], d, seed=19)
    s = _store_of(ctx, c)
    rng = np.random.default_rng(20)
    q = rng.standard_normal((96, d)).astype(np.float32)
    old, new = rng.permutation(c["ids"])[:5000], np.arange(10 ** 6, 10 ** 6 + 300, dtype=np.int64)
    S = np.concatenate([old, new])
    f = Filter(s, S, "allow")
    gi, gd = ctx.search_exact(s, q, 10, "l2", f)
    assert ctx.last_scan_kernel() == "k_dense_pf"
    oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], 10, "l2", S, "allow")
    _eq(gi, gd, oi, od, "before")
    hit = np.unique(_np(gi))
    s.remove_ids(np.concatenate([hit, np.setdiff1d(old, hit)])[:300])
    s.add_entries(1, new, (q[rng.integers(0, 96, size=300)] + 0.05 * rng.standard_normal((300, d))).astype(np.float32))
    assert f.candidate_rows(ctx) == 5000
    gi2, gd2 = ctx.search_exact(s, q, 10, "l2", f)
    assert ctx.last_scan_kernel() == "k_dense_pf" and f.exact_info()["builds"] == 2
    vecs, ids, offsets = _csr_of(s, d)
    oi, od = E.search(q, vecs, ids, offsets, 10, "l2", S, "allow")
    _eq(gi2, gd2, oi, od, "after")
    assert np.isin(_np(gi2), new).any() and not np.array_equal(_np(gi), _np(gi2))
    _check(ctx, s, dict(c, vecs=vecs, ids=ids, offsets=offsets), q, 10, f, S, "allow", "after, all lists")
    assert f.exact_info()["builds"] == 2
    f.close()
    s.close()


# ---- 3. stale rows, life cycle, max_rows ------------------------------------------------------------------------------------------
def _csr_of(s, d):
    lists = sorted(int(p) for p in s.list_ids())
    pv, pi = zip(*[s.get_list(p) for p in lists])
    return O.csr_from_partitions(pv, pi, d)


def test_stale_rows(ctx):
    """about 1000 candidates, then remove_ids down to 17: a rebuild with fewer candidates leaves no old row visible"""
    from quake_amd.capi import Filter
    c = _flat_corpus([700, 3, 1500, 260], 20, seed=6)
    s = _store_of(ctx, c)
    q = np.random.default_rng(7).standard_normal((17, 20)).astype(np.float32)
    S = np.random.default_rng(8).permutation(c["ids"])[:1000]
    f = Filter(s, S, "allow")
    _check(ctx, s, c, q, 100, f, S, "allow", "before")
    s.remove_ids(S[17:])
    vecs, ids, offsets = _csr_of(s, 20)
    c2 = dict(c, vecs=vecs, ids=ids, offsets=offsets)
    gi, gd = _check(ctx, s, c2, q, 100, f, S, "allow", "after")
    assert ((gi >= 0).sum(axis=1) == 17).all() and (gi[:, 17:] == -1).all() and np.isinf(gd[:, 17:]).all()
    assert sorted(gi[0, :17]) == sorted(S[:17])
    assert f.exact_info()["builds"] == 2
    f.close()
    s.close()


def test_life_cycle(ctx):
    """after remove_ids, a relocating add_entries, a compaction and a set_attribute under a predicate the exact result follows the
    ids; `builds` grows by one per change and by none otherwise; other filtered calls never create the candidate store; a store
    derived on one context is searched on another"""
    from quake_amd.capi import Attr, Context, Filter, Store
    d = 20
    c = _flat_corpus([300, 40, 900, 0, 130], d, seed=9)
    s = _store_of(ctx, c)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, 5], np.int64), np.arange(5, dtype=np.int64), np.random.default_rng(1).standard_normal((5, d)).astype(np.float32))
    rng = np.random.default_rng(10)
    q = rng.standard_normal((17, d)).astype(np.float32)
    S = np.concatenate([rng.permutation(c["ids"])[:400], np.arange(10 ** 6, 10 ** 6 + 40000, 3)]).astype(np.int64)
    f = Filter(s, S, "allow")
    col = {int(i): int(i) % 7 for i in c["ids"]}
    attr = Attr(s)
    attr.set(np.fromiter(col.keys(), np.int64), np.fromiter(col.values(), np.int64))
    w = Filter.where(s, [(attr, "range", 2, 3)])
    builds = {"ids": 0, "where": 0}

    def check(tag, changed):
        vecs, ids, offsets = _csr_of(s, d)
        cur = dict(c, vecs=vecs, ids=ids, offsets=offsets)
        wS = np.array([i for i in ids if col.get(int(i), -1) in (2, 3)], np.int64)
        for name, flt, spec in (("ids", f, (S, "allow")), ("where", w, (wS, "allow"))):
            for again in (False, True):  # two searches in a row: the second never derives
                _check(ctx, s, cur, q, 10, flt, *spec, tag=(tag, name, again))
                want = builds[name] + (1 if changed and not again else 0)
                info = flt.exact_info()
                assert info["builds"] == want, (tag, name, again, info)
                builds[name] = want
                assert info["device_bytes"] >= info["rows"] * (32 * 4 + 12) and flt.info()["device_bytes"] > info["device_bytes"]

    # the other filtered calls neither allocate nor launch anything for the candidate store
    ctx.search(parent, s, q, 2, 10, "l2", filter=f)
    ctx.search_adaptive(parent, s, q, 1, 5, 10, "l2", filter=f)
    ctx.range_search(parent, s, q, 2, 3.0, "l2", filter=f)
    ctx.search_after(parent, s, q, 2, 10, "l2", filter=f)
    assert f.exact_info() == {"rows": 0, "builds": 0, "device_bytes": 0}
    before = f.info()["device_bytes"]
    check("as built", changed=True)  # (the first exact call derives the store)
    assert f.info()["device_bytes"] == before + f.exact_info()["device_bytes"]
    check("nothing changed", changed=False)
    s.remove_ids(np.concatenate([S[:100], np.setdiff1d(c["ids"], S)[:100]]))
    check("remove_ids", changed=True)
    moved = s.counters()["list_relocations"]
    nid = np.arange(10 ** 6, 10 ** 6 + 600, dtype=np.int64)  # a third of them are in S
    s.add_entries(1, nid, rng.standard_normal((600, d)).astype(np.float32))
    attr.set(nid, nid % 7)
    col.update({int(i): int(i) % 7 for i in nid})
    assert s.counters()["list_relocations"] > moved
    check("relocating add_entries", changed=True)
    compactions, nxt = s.counters()["arena_compactions"], 10 ** 6 + 600
    for step in range(40):
        if s.counters()["arena_compactions"] > compactions:
            break
        n = 500 * (step + 1)
        s.add_entries(4 if step % 2 else 1, np.arange(nxt, nxt + n, dtype=np.int64), rng.standard_normal((n, d)).astype(np.float32))
        nxt += n
    assert s.counters()["arena_compactions"] > compactions
    check("compaction", changed=True)
    flip = np.array([i for i in c["ids"][:200] if int(i) in col], np.int64)
    attr.set(flip, np.full(flip.shape[0], 2, np.int64))
    col.update({int(i): 2 for i in flip})
    vecs, ids, offsets = _csr_of(s, d)
    cur = dict(c, vecs=vecs, ids=ids, offsets=offsets)
    wS = np.array([i for i in ids if col.get(int(i), -1) in (2, 3)], np.int64)
    _check(ctx, s, cur, q, 10, w, wS, "allow", "set_attribute")
    assert w.exact_info()["builds"] == builds["where"] + 1 and f.exact_info()["builds"] == builds["ids"]
    # derived on one context, searched on another
    other = Context(0)
    try:
        gi, gd = other.search_exact(s, q, 10, "l2", w)
        oi, od = E.search(q, vecs, ids, offsets, 10, "l2", wS, "allow")
        _eq(gi, gd, oi, od, "another context")
        assert w.exact_info()["builds"] == builds["where"] + 1
        s.remove_ids(wS[:5])
        gi, gd = other.search_exact(s, q, 10, "l2", w)  # ... and derived there, searched here
        vecs, ids, offsets = _csr_of(s, d)
        oi, od = E.search(q, vecs, ids, offsets, 10, "l2", wS[5:], "allow")
        _eq(gi, gd, oi, od, "derived on the other context")
        gi, gd = ctx.search_exact(s, q, 10, "l2", w)
        _eq(gi, gd, oi, od, "back on the first context")
        assert w.exact_info()["builds"] == builds["where"] + 2
    finally:
        other.close()
    for x in (f, w, attr, s, parent):
        x.close()


def test_max_rows(ctx, corpora):
    from quake_amd.capi import Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(20, "l2")
    S = np.random.default_rng(11).permutation(c["ids"])[:300]
    f = Filter(s, S, "allow")
    q = _queries(c, 5, seed=12)
    assert f.candidate_rows(ctx) == 300
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*max_rows"):
        ctx.search_exact(s, q, 10, "l2", f, max_rows=299)
    assert f.exact_info() == {"rows": 0, "builds": 0, "device_bytes": 0}  # nothing is allocated by the refusal
    gi, gd = ctx.search_exact(s, q, 10, "l2", f, max_rows=300)
    oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], 10, "l2", S, "allow")
    _eq(gi, gd, oi, od, "max_rows = rows")
    info = f.exact_info()
    assert info["rows"] == 300 and info["builds"] == 1 and info["device_bytes"] > 0
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*max_rows"):
        ctx.search_exact(s, q, 10, "l2", f, max_rows=299)
    assert f.exact_info() == info
    f.close()


def test_refusals_of_the_c_abi(ctx, corpora):
    from quake_amd.capi import Filter
    from quake_amd._lib import QuakeHipError
    c, s, parent = corpora(20, "l2")
    c2, s2, parent2 = corpora(8, "l2")
    q = _queries(c, 5, seed=13)
    f2 = Filter(s2, c2["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search_exact(s, q, 10, "l2", f2)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        f2.store = s
        try:
            f2.candidate_rows(ctx)
        finally:
            f2.store = s2
    f = Filter(s, c["ids"][:100], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED"):
        ctx.search_exact(s, q, 8193, "l2", f)
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID"):
        ctx.search_exact(s, q, 0, "l2", f)
    gi, gd = ctx.search_exact(s, q, 8192, "l2", f)  # the largest k the flat search takes
    oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], 8192, "l2", c["ids"][:100], "allow")
    _eq(gi, gd, oi, od, "k = 8192")
    f.close()
    f2.close()


def test_empty_store(ctx):
    from quake_amd.capi import Filter, Store
    s = Store(ctx, 20)
    q = np.random.default_rng(14).standard_normal((3, 20)).astype(np.float32)
    for f in (Filter(s, np.arange(5, dtype=np.int64), "allow"), Filter(s, np.zeros(0, np.int64), "deny")):
        gi, gd = ctx.search_exact(s, q, 10, "l2", f)
        assert (gi == -1).all() and np.isposinf(gd).all() and f.candidate_rows(ctx) == 0
        gi, gd = ctx.search_exact(s, q, 10, "ip", f)
        assert (gi == -1).all() and np.isneginf(gd).all()
        f.close()
    s.close()


# ---- 4. squared L2, non-finite values, wide rows, 64-bit ids -----------------------------------------------------------------------
def test_squared_l2(ctx, corpora, families):
    """qk_ctx_set_squared_l2 is honoured as in qk_search: the flat search of a one-list store of the same rows, bit for bit"""
    from quake_amd.capi import Store
    c, s, parent = corpora(20, "l2")
    fam = families(20, "l2")
    S, mode = fam.spec[0]
    keep = Y.allowed_rows(c["ids"], S, mode)
    one = Store(ctx, 20)
    one.build_csr(np.array([0, int(keep.sum())], np.int64), c["ids"][keep], c["vecs"][keep])
    q = _queries(c, 17, seed=15)
    oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], 10, "l2", S, mode)
    ctx.set_squared_l2(True)
    try:
        gi, gd = ctx.search_exact(s, q, 10, "l2", fam.h[0])
        fi, fd = ctx.search(None, one, q, 1, 10, "l2")
    finally:
        ctx.set_squared_l2(False)
    _eq(gi, gd, fi, fd, "squared: the flat search")
    _eq(gi, np.sqrt(gd), oi, od, "squared: the yardstick")  # sqrtf is correctly rounded on both sides
    assert not np.array_equal(gd, od)
    one.close()


@pytest.mark.parametrize("cls", ["nan", "inf"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_nonfinite_candidates(ctx, cls, metric):
    """NaN rows and +-inf rows among the candidates: the flat search's contract, unchanged"""
    from quake_amd.capi import Filter, Store
    c = NF.corpus(cls, metric, 6000, 12, 24, seed=16)
    s = Store(ctx, 24)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    q, _ = NF.queries(c, 17, seed=17)
    rng = np.random.default_rng(18)
    S = np.union1d(Y.draw_set(c["ids"], 0.2, rng), c["ids"][c["special"]])  # every planted row is a candidate
    f = Filter(s, S, "allow")
    cc = dict(c, metric=metric)
    for k in (1, 10, 100):
        _check(ctx, s, cc, q, k, f, S, "allow", (cls, metric, k), finite=False)
    f.close()
    s.close()


def test_wide_rows(ctx):
    """one d beyond the LDS limit of the dense kernel's query tile"""
    from quake_amd.capi import Filter
    c = _skewed_corpus(3072, 24, 3000, "l2", seed=51)
    s, parent = _skewed_stores(ctx, c)
    q = np.ascontiguousarray(c["x"][:19] + 0.01)
    S = Y.draw_set(c["ids"], 0.1, np.random.default_rng(53))
    f = Filter(s, S, "allow")
    for k in (1, 10, 500):
        gi, gd = ctx.search_exact(s, q, k, "l2", f)
        assert ctx.last_scan_kernel() == "k_dense_wide"
        oi, od = E.search(q, c["vecs"], c["ids"], c["offsets"], k, "l2", S, "allow")
        _eq(gi, gd, oi, od, k)
    f.close()
    s.close()
    parent.close()


def test_64_bit_ids(ctx):
    from quake_amd.capi import Filter
    c = _skewed_corpus(128, 32, 12000, "l2", seed=81, id_base=1 << 33, id_step=16)
    assert c["ids"].min() >= (1 << 33)
    s, parent = _skewed_stores(ctx, c)
    q = np.ascontiguousarray(c["x"][:33] + 0.01)
    S = Y.draw_set(c["ids"], 0.1, np.random.default_rng(83))
    for S_, mode in [(S, "allow"), (S, "deny"), (S + 1, "allow")]:
        f = Filter(s, S_, mode)
        for k in (1, 10):
            _check(ctx, s, c, q, k, f, S_, mode, (mode, k))
        f.close()
    s.close()
    parent.close()


# ---- 5. both mirrors ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def _flat_csr(idx):
    s = idx._store
    lists = sorted(int(p) for p in s.list_ids())
    pv, pi = zip(*[s.get_list(p) for p in lists])
    return O.csr_from_partitions(pv, pi, idx._d)


def test_both_mirrors(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(61)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(33, d, generator=g)
    S = Y.draw_set(ids.numpy(), 0.02, np.random.default_rng(62))  # 120 candidates
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, 20)
        sp = mod.SearchParams()
        assert sp.filter_exact_rows == 0
        before = repr(sp)
        sp.k, sp.nprobe = 10, 3
        plain = idx.search(q, sp)
        assert plain.exact is None
        sp.filter = idx.make_filter(torch.from_numpy(S))
        today = idx.search(q, sp)
        assert today.exact is None
        sp.filter_exact_rows = S.shape[0] - 1  # below the filter's count: the call of today
        r = idx.search(q, sp)
        assert r.exact is False and r.nprobed is None
        assert torch.equal(r.ids, today.ids) and torch.equal(r.distances, today.distances)
        sp.max_nprobe = 12  # ... the adaptive call when max_nprobe is set
        r = idx.search(q, sp)
        sp.filter_exact_rows = 0
        adaptive = idx.search(q, sp)
        assert r.exact is False and r.nprobed is not None and torch.equal(r.nprobed, adaptive.nprobed)
        assert torch.equal(r.ids, adaptive.ids) and torch.equal(r.distances, adaptive.distances)
        sp.filter_exact_rows = S.shape[0]  # at the filter's count: exact, with or without max_nprobe
        for mx in (12, 0):
            sp.max_nprobe = mx
            track = name == "python" and mx == 0
            if track:
                idx._flush_hits()
                idx.track_hits = True
            r = idx.search(q, sp)
            rd = idx.search(q.cuda(), sp)
            assert r.exact is True and rd.exact is True and r.nprobed is None
            assert r.timing_info.parent_info is None
            assert torch.equal(rd.ids.cpu(), r.ids) and torch.equal(rd.distances.cpu(), r.distances)
            if track:
                assert len(idx._pending_hits) == 0  # an exact call probes no partition: no hits for the policy
                idx.track_hits = False
        # what the mirror's search of a flat (parent-less) index reports: the Python mirror the lists of the call (qk_timing's
        # n_items: the one list), the compiled mirror the (query, list) pairs (qk_timing's partitions_scanned: one per query)
        assert r.timing_info.partitions_scanned == (1 if name == "python" else 33)
        out[name] = (r.ids.numpy(), r.distances.numpy())
        sp.k = 1000  # beyond QK_MAX_K under a filter
        r = idx.search(q, sp)
        assert r.exact is True and tuple(r.ids.shape) == (33, 1000) and int((r.ids >= 0).sum()) == 33 * S.shape[0]
        out[name + "-1000"] = (r.ids.numpy(), r.distances.numpy())
        assert "filter_exact_rows" not in before and repr(mod.SearchParams()) == before
        if name == "python":
            vecs, aids, offs = _flat_csr(idx)
            for key, k in (("python", 10), ("python-1000", 1000)):
                oi, od = E.search(q.numpy(), vecs, aids, offs, k, "l2", S, "allow")
                _eq(*out[key], oi, od, key)
    for key in ("", "-1000"):
        np.testing.assert_array_equal(out["python" + key][0], out["compiled" + key][0])
        np.testing.assert_array_equal(out["python" + key][1].view(np.uint32), out["compiled" + key][1].view(np.uint32))


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(71)
    x = torch.randn(4000, 16, generator=g)
    ids = torch.arange(4000)
    qq = torch.randn(10, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 16)
        sp = mod.SearchParams()
        sp.k, sp.nprobe = 5, 4
        plain = idx.search(qq, sp)
        sp.filter_exact_rows = 100
        with pytest.raises(RuntimeError, match="filter_exact_rows needs a filter"):
            idx.search(qq, sp)
        f = idx.make_filter(ids[:50])
        sp.filters, sp.query_filter = [f], torch.zeros(10, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="filter_exact_rows.*query_filter"):
            idx.search(qq, sp)
        sp.filters, sp.query_filter = [], None
        sp.filter = f
        sp.recall_target = 0.9
        with pytest.raises(RuntimeError, match="filter_exact_rows.*recall_target"):
            idx.search(qq, sp)
        sp.recall_target = -1.0
        for call in (lambda: idx.search_after(qq, sp), lambda: idx.range_search(qq, 1.0, sp)):
            with pytest.raises(RuntimeError, match="filter_exact_rows"):
                call()
        idx.set_attribute("g", ids, ids % 5)
        with pytest.raises(RuntimeError, match="filter_exact_rows"):
            idx.grouped_search(qq, "g", sp)
        grp = _build(mod, x, ids, 16, workers=2)
        with pytest.raises(RuntimeError, match="filter_exact_rows.*num_workers"):
            grp.search(qq, sp)
        sp.filter_exact_rows = -1
        with pytest.raises(RuntimeError, match="filter_exact_rows"):
            idx.search(qq, sp)
        sp.filter_exact_rows = 100
        r = idx.search(qq, sp)  # the index still answers, and exactly
        assert r.exact is True and int((r.ids >= 0).sum()) == 10 * 5
        sp.filter, sp.filter_exact_rows = None, 0
        again = idx.search(qq, sp)
        assert torch.equal(again.ids, plain.ids) and torch.equal(again.distances, plain.distances)
