"""Attribute filters on the GPU (qk_attr_*, qk_filter_create_where; Attr / Filter.where; set_attribute / make_filter(where=) in both
mirrors): int64 columns keyed by vector id and predicate filters over them, turned into the row mask of a qk_filter by
k_filter_build_where.

The equation under test: at any moment a predicate filter answers exactly like the QK_FILTER_ALLOW id-set filter over
{id : every clause holds for id}.  Every comparison is bit for bit -- ids, and the uint32 view of the distances -- against
tests/attr_yardstick.py (a numpy evaluation of the clauses, then the oracle's search over the CSR with the other rows deleted) and,
on top of that, against an id-set filter made from the yardstick's id set.

Shapes: the corpus of tests/test_filtered_search.py (20 000 x 64 in 64 skewed lists: empty lists, lists of 5 and 7 rows, lengths
that are no multiple of 16, a list longer than the 1024 rows a block of k_filter_build_where covers per step)."""
import zlib

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import filter_yardstick as Y
import oracle as O

pytestmark = pytest.mark.gpu

MIN, MAX = AY.INT64_MIN, AY.INT64_MAX
FAR = 1 << 45  # an id nobody stores: a value for it alone pushes a column out of the table layout
SPARSE_STEP = 54_975_581  # ids up to ~2^40


def _corpus(d, nlist, n, metric, seed, empty=2, id_base=7, id_step=1):
    """tests/test_filtered_search.py's: clustered rows in skewed lists, `empty` empty lists, a list of 5 and one of 7 rows"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 0.05
    w[:empty + 2] = 0.0
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    assign[:5] = empty
    assign[5:12] = empty + 1
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) * id_step + id_base
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return dict(cent=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets, x=x, d=d,
                metric=metric)


def _queries(c, Q, seed):
    rng = np.random.default_rng(seed)
    q = (c["x"][rng.integers(0, c["x"].shape[0], size=Q)] + 0.05 * rng.standard_normal((Q, c["d"]))).astype(np.float32)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q)


def _stores(ctx, c):
    from quake_amd.capi import Store
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _eq(gi, gd, oi, od, tag):
    np.testing.assert_array_equal(_np(gi), _np(oi), err_msg=str(tag))
    np.testing.assert_array_equal(_np(gd).view(np.uint32), _np(od).view(np.uint32), err_msg=str(tag))


def _columns(c, seed):
    """three columns over the corpus' ids as dicts id -> value.  `tenant`: 0 .. 49, missing for ~5 % of the stored ids, constant
    (3) over the first 64 rows of the longest list -- whole tiles of candidates next to whole tiles of none; `ts`: the whole int64
    range with both extremes, missing for ~10 %; `flags`: 16 random bits, every stored id.  All hold ids nobody stores."""
    rng = np.random.default_rng(seed)
    ids, o = c["ids"], c["offsets"]
    n = ids.shape[0]
    big = int(np.argmax(np.diff(o)))
    tenant = {int(i): int(v) for i, v in zip(ids, rng.integers(0, 50, n)) if rng.random() >= 0.05}
    for i in ids[o[big]:o[big] + 64]:
        tenant[int(i)] = 3
    for i in ids[o[big] + 64:o[big] + 128]:
        tenant[int(i)] = 4
    ts_vals = rng.integers(MIN, MAX, n, dtype=np.int64, endpoint=True)
    ts_vals[::3] = rng.integers(-1000, 1000, ts_vals[::3].shape[0])
    ts = {int(i): int(v) for i, v in zip(ids, ts_vals) if rng.random() >= 0.10}
    some = [int(i) for i in ids[rng.permutation(n)[:4]]]
    ts[some[0]], ts[some[1]], ts[some[2]], ts[some[3]] = MIN, MAX, -1, 0
    flags = {int(i): int(v) for i, v in zip(ids, rng.integers(0, 1 << 16, n))}
    ghost = int(ids.max()) + 1  # (not stored)
    tenant[ghost], ts[ghost], flags[ghost] = 3, 0, 0xFFFF
    return dict(tenant=tenant, ts=ts, flags=flags), big


def _set_column(attr, col, device):
    k = np.fromiter(col.keys(), np.int64, len(col))
    v = np.fromiter(col.values(), np.int64, len(col))
    if device:
        attr.set(torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
    else:
        attr.set(k, v)


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    """(corpus, store, parent, column dicts, Attrs, longest list) per (metric, sparse).  Dense ids (step 1): `tenant` and `flags`
    are tables, `ts` also holds FAR and is sorted -- conjunctions over them mix the layouts; sparse ids: all sorted.  The columns
    of the ip corpora are set from device tensors, those of the l2 corpora from host arrays."""
    from quake_amd.capi import Attr
    cache = {}

    def get(metric, sparse):
        key = (metric, sparse)
        if key not in cache:
            c = _corpus(64, 64, 20000, metric, seed=188 if metric == "ip" else 183, id_step=SPARSE_STEP if sparse else 1)
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and ((sizes > 0) & (sizes < 16)).sum() >= 2 and (sizes % 16 != 0).any()
            # more than the 64 tiles a block of k_filter_build_where covers per step, so the longest list is shared by two block
            # rows (blockIdx.y = 0, 1) and all four rows a lane keeps in flight are live.  The launch sizes gridDim.y so that a
            # block's stride loop runs once unless a list has more than 65535 x 64 tiles (k_filter_build is built the same way):
            # a second iteration of that loop is covered by no test of this size
            assert sizes.max() > 1024
            s, parent = _stores(ctx, c)
            cols, big = _columns(c, seed=9 + sparse)
            if not sparse:
                cols["ts"][FAR] = 5
            attrs = {}
            for name, col in cols.items():
                attrs[name] = Attr(s)
                _set_column(attrs[name], col, device=metric == "ip")
                info = attrs[name].info()
                assert info["n_ids"] == len(col) and info["device_bytes"] > 0
            lay = {name: a.info()["layout"] for name, a in attrs.items()}
            assert lay == (dict(tenant="sorted", ts="sorted", flags="sorted") if sparse else dict(tenant="table", ts="sorted", flags="table"))
            # some stored id has no value
            assert any(int(i) not in cols["tenant"] for i in c["ids"]) and any(int(i) not in cols["ts"] for i in c["ids"])
            cache[key] = (c, s, parent, cols, attrs, big)
        return cache[key]

    yield get
    for c, s, p, cols, attrs, big in cache.values():
        for a in attrs.values():
            a.close()
        s.close()
        p.close()


def test_get_reads_back_both_layouts(corpora):
    for sparse in (False, True):
        c, s, parent, cols, attrs, big = corpora("l2", sparse)
        rng = np.random.default_rng(5)
        probe = np.concatenate([c["ids"][rng.permutation(20000)[:500]], np.array([0, 1, FAR, FAR + 1, int(c["ids"].max()) + 1, MAX], np.int64)])
        for name, col in cols.items():
            vals, found = attrs[name].get(probe)
            np.testing.assert_array_equal(found, np.array([int(i) in col for i in probe]))
            np.testing.assert_array_equal(vals, np.array([col.get(int(i), 0) for i in probe], np.int64))


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
R, NR, ANY, ALL, NO = "range", "not_range", "any_bits", "all_bits", "no_bits"
EIGHT = [("tenant", R, 0, 40), ("tenant", NR, 7, 7), ("ts", R, -(1 << 62), 1 << 62), ("ts", NR, -50, 50), ("flags", ANY, 0xFF, 0),
         ("flags", NO, 0x8000, 0), ("flags", ALL, 0x1, 0), ("tenant", R, 1, 49)]
# clauses, and what the case must show: "all" every stored row with a flags value, "none" no row, "pad" a padded result row,
# "tiles" a tile word 0 and a tile word 0xFFFF
CLAUSES = [
    ([("flags", NO, 0, 0)], "all"),
    ([("tenant", R, 5, 4)], "none"),
    ([("tenant", R, 3, 3)], "tiles"),
    ([("tenant", NR, 0, 24)], ""),
    ([("flags", ANY, 0x3, 0)], ""),
    ([("flags", ALL, 0x5, 0)], ""),
    ([("flags", NO, 0xF0, 0)], ""),
    ([("ts", R, MIN, -1)], ""),
    ([("ts", NR, MIN + 1, MAX - 1)], "pad"),
    ([("tenant", R, 0, 9), ("ts", R, -1000, 1000)], ""),
    ([("ts", NO, 1, 0), ("flags", ANY, 0xF000, 0)], ""),
    (EIGHT, ""),
]


def _grid():
    """every clause list once, the other axes dealt round by seeded shuffles (every value of every axis appears)"""
    axes = dict(metric=["l2", "ip"], sparse=[False, True], mem=["host", "device"], entry=["search", "coarse+scan"], nprobe=[1, 8, 32],
                k=[1, 10, 100], Q=[1, 33, 300])
    rng = np.random.default_rng(20250611)
    n = len(CLAUSES)
    cols = {}
    for name, vals in axes.items():
        seq = []
        while len(seq) < n:
            seq += [vals[i] for i in rng.permutation(len(vals))]
        cols[name] = seq[:n]
    cases = [dict(cl=i, **{name: cols[name][i] for name in axes}) for i in range(n)]
    for name, vals in axes.items():
        assert {c[name] for c in cases} == set(vals), name
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_grid(ctx, corpora, case):
    from quake_amd.capi import Filter
    c, s, parent, cols, attrs, big = corpora(case["metric"], case["sparse"])
    clauses, shows = CLAUSES[case["cl"]]
    metric, nprobe, k, Q = case["metric"], case["nprobe"], case["k"], case["Q"]
    rng = np.random.default_rng(zlib.crc32(repr(sorted(case.items())).encode()))
    q = _queries(c, Q, seed=int(rng.integers(1 << 30)))
    if "pad" in shows or "none" in shows:
        k = max(k, 100)  # (a handful of candidates in the whole store: short rows)
    keep = AY.eval_clauses(clauses, c["ids"], cols)
    S = AY.allowed_set(keep, c["ids"])
    if "all" in shows:
        assert keep.all()
    if "none" in shows:
        assert not keep.any()
    if "tiles" in shows:
        words = AY.tile_words(keep, c["offsets"])
        assert (words == 0).any() and (words == 0xFFFF).any()
    oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, keep)
    if "pad" in shows or "none" in shows:
        assert (oi < 0).any()
    dev = case["mem"] == "device"
    xq = torch.from_numpy(q).cuda() if dev else q

    def run(f):
        if case["entry"] == "search":
            gi, gd = ctx.search(parent, s, xq, nprobe, k, metric, filter=f)
        else:
            pids, _ = ctx.coarse(parent, xq, nprobe, metric)
            gi, gd = ctx.scan(s, xq, pids, k, metric, filter=f)
        ctx.synchronize()
        assert "(filtered)" in ctx.last_scan_kernel()
        return gi, gd

    cl = [(attrs[name], op, a, b) for name, op, a, b in clauses]
    f = Filter.where(s, cl)
    f_perm = Filter.where(s, [cl[i] for i in rng.permutation(len(cl))][::-1])
    f_ids = Filter(s, S, "allow")
    try:
        gi, gd = run(f)
        _eq(gi, gd, oi, od, case)
        _eq(*run(f_ids), oi, od, (case, "id set"))
        _eq(*run(f_perm), oi, od, (case, "clause order"))
        got = _np(gi)
        assert np.isin(got[got >= 0], S).all()
        for flt in (f, f_perm):
            info = flt.info()
            assert info["n_ids"] == -1 and info["rebuilds"] == 0 and info["rows_allowed"] == int(keep.sum())
            assert info["device_bytes"] < f_ids.info()["device_bytes"] or S.shape[0] == 0
    finally:
        f.close()
        f_perm.close()
        f_ids.close()


def test_conjunctions_over_different_layouts(ctx, corpora):
    from quake_amd.capi import Filter
    for metric in ("l2", "ip"):
        c, s, parent, cols, attrs, big = corpora(metric, False)
        assert attrs["tenant"].info()["layout"] == "table" and attrs["ts"].info()["layout"] == "sorted"
        q = _queries(c, 33, seed=21)
        for clauses in ([("tenant", R, 0, 9), ("ts", R, -1000, 1000)], [("ts", NR, -500, MAX), ("tenant", NR, 10, 49)], EIGHT):
            keep = AY.eval_clauses(clauses, c["ids"], cols)
            assert 0 < keep.sum() < keep.shape[0]
            oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 8, 10, metric, keep)
            f = Filter.where(s, [(attrs[n], op, a, b) for n, op, a, b in clauses])
            _eq(*ctx.search(parent, s, q, 8, 10, metric, filter=f), oi, od, (metric, clauses))
            assert f.info()["rows_allowed"] == int(keep.sum())
            f.close()


# ---- 2. liveness -----------------------------------------------------------------------------------------------------------------
def _store_csr(s, nlist, d):
    pv, pi = zip(*[s.get_list(p) for p in range(nlist)])
    return O.csr_from_partitions(pv, pi, d)


def test_liveness(ctx):
    from quake_amd.capi import Attr, Filter
    c = _corpus(64, 64, 20000, "l2", seed=171)
    s, parent = _stores(ctx, c)
    nlist, d = 64, 64
    rng = np.random.default_rng(172)
    q = _queries(c, 40, seed=173)
    ids = c["ids"]
    col = {int(i): int(v) for i, v in zip(ids, rng.integers(0, 20, ids.shape[0])) if rng.random() >= 0.1}
    a = Attr(s)
    _set_column(a, col, device=False)
    assert a.info()["layout"] == "table"
    clauses = [("t", R, 0, 4)]
    f = Filter.where(s, [(a, R, 0, 4)])
    state = dict(rebuilds=0, last=None)

    def check(tag, rebuilt, same_as_last=False):
        vecs, cids, offs = _store_csr(s, nlist, d)
        keep = AY.eval_clauses(clauses, cids, {"t": col})
        assert 0 < keep.sum() < keep.shape[0], tag
        oi, od = AY.search(q, c["cent"], vecs, cids, offs, 8, 100, "l2", keep)
        for again in (False, True):  # the second call finds nothing changed
            gi, gd = ctx.search(parent, s, q, 8, 100, "l2", filter=f)
            _eq(gi, gd, oi, od, (tag, again))
            info = f.info()
            state["rebuilds"] += 1 if rebuilt and not again else 0
            assert info["rebuilds"] == state["rebuilds"], (tag, again, info)
            assert info["rows_allowed"] == int(keep.sum()), tag
        if same_as_last:
            _eq(gi, gd, *state["last"], tag)
        state["last"] = (gi, gd)
        fi = Filter(s, AY.allowed_set(keep, cids), "allow")
        _eq(*ctx.search(parent, s, q, 8, 100, "l2", filter=fi), oi, od, (tag, "id set"))
        fi.close()
        vals, found = a.get(cids[:300])
        np.testing.assert_array_equal(found, np.array([int(i) in col for i in cids[:300]]), err_msg=tag)
        np.testing.assert_array_equal(vals[found], np.array([col[int(i)] for i in cids[:300][found]], np.int64), err_msg=tag)

    check("as made", rebuilt=False)
    v0 = a.info()["version"]
    # values change, the store does not
    upd = ids[rng.permutation(ids.shape[0])[:500]]
    newv = rng.integers(0, 20, 500)
    a.set(upd, newv)
    col.update({int(i): int(v) for i, v in zip(upd, newv)})
    assert a.info()["version"] == v0 + 1
    check("set", rebuilt=True)
    gone = np.concatenate([upd[:150], ids[:150], np.array([FAR, 3], np.int64)])  # (ids without a value are ignored)
    a.unset(torch.from_numpy(gone).cuda())
    for i in gone:
        col.pop(int(i), None)
    assert a.info()["n_ids"] == len(col)
    check("unset", rebuilt=True)
    # one set that names an id several times: the last value wins
    x, y = int(ids[1000]), int(ids[1001])
    a.set(np.array([x, x, y, x, y], np.int64), np.array([1, 19, 19, 2, 3], np.int64))
    col[x], col[y] = 2, 3
    vals, found = a.get(np.array([x, y], np.int64))
    assert found.all() and vals.tolist() == [2, 3]
    check("duplicates in one set", rebuilt=True)
    # rows are added: without values they are no candidates; then they get values and the table grows
    new_ids = np.arange(30000, 30600, dtype=np.int64)
    newx = (c["cent"][10] + 0.4 * rng.standard_normal((600, d))).astype(np.float32)
    s.add_entries(10, new_ids, newx)
    check("add", rebuilt=True)
    bytes0 = a.info()["device_bytes"]
    a.set(new_ids, np.full(600, 2, np.int64))
    col.update({int(i): 2 for i in new_ids})
    assert a.info()["layout"] == "table" and a.info()["device_bytes"] > bytes0
    check("values for the added rows", rebuilt=True)
    # remove: allowed rows go, their values stay
    rem = new_ids[:200]
    assert s.remove_ids(rem) == 200
    check("remove", rebuilt=True)
    assert a.get(rem)[1].all()
    # one far id flips the column to sorted pairs, its unset flips it back: the answers do not move
    a.set(np.array([FAR], np.int64), np.array([1], np.int64))
    col[FAR] = 1
    assert a.info()["layout"] == "sorted"
    check("table -> sorted", rebuilt=True, same_as_last=True)
    a.unset(np.array([FAR], np.int64))
    del col[FAR]
    assert a.info()["layout"] == "table"
    check("sorted -> table", rebuilt=True, same_as_last=True)
    check("nothing changed", rebuilt=False, same_as_last=True)
    f.close()
    a.close()
    s.close()
    parent.close()


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------
def test_per_query_batch_mixes_predicates_and_id_sets(ctx, corpora):
    """Five NARROW filters -- three predicates, two id sets -- in one per-query table: each row equals the single-filter call.
    Then one predicate's column changes under an unchanged store.  The scan of a per-query call reads only the tiles of the OR of
    the masks, which the context caches: a union kept from before the change has no bit in the tiles the new candidates sit in
    (asserted below), so the call after the change is right only if the cache noticed the rebuild."""
    from quake_amd.capi import Attr, Filter
    c, s, parent, cols, attrs, big = corpora("l2", False)
    rng = np.random.default_rng(31)
    o, ids = c["offsets"], c["ids"]
    rows_a, rows_b = np.arange(o[big] + 256, o[big] + 512), np.arange(o[big] + 512, o[big] + 768)  # 16 whole tiles each
    own = Attr(s)  # a column of this test: candidates (value 1) are the rows B now, the rows A after the change
    own_col = {**{int(i): 0 for i in ids[rows_a]}, **{int(i): 1 for i in ids[rows_b]}}
    _set_column(own, own_col, device=False)
    elsewhere = np.setdiff1d(ids, ids[o[big]:o[big + 1]])
    sets = [Y.draw_set(elsewhere, 0.01, rng), Y.draw_set(elsewhere, 0.005, rng)]
    preds = [[("tenant", R, 3, 3)], [("flags", ALL, 0xFFF0, 0)]]
    fl = [Filter.where(s, [(attrs[n], op, a, b) for n, op, a, b in preds[0]]), Filter(s, sets[0], "allow"),
          Filter.where(s, [(attrs[n], op, a, b) for n, op, a, b in preds[1]]), Filter(s, sets[1], "allow"),
          Filter.where(s, [(own, R, 1, 1)])]
    qf = rng.permutation(np.arange(50) % len(fl)).astype(np.int32)
    assert set(qf.tolist()) == set(range(len(fl)))
    q = _queries(c, 50, seed=32)
    mine = np.flatnonzero(qf == 4)  # the queries of the changing filter sit on the rows A
    q[mine] = c["vecs"][rows_a[rng.integers(0, 256, mine.shape[0])]] + 0.05 * rng.standard_normal((mine.shape[0], 64)).astype(np.float32)

    def check(tag):
        gi, gd = ctx.search(parent, s, q, 8, 10, "l2", filters=fl, query_filter=qf)
        assert "per query" in ctx.last_scan_kernel()
        for i in range(50):
            si, sd = ctx.search(parent, s, q[i:i + 1], 8, 10, "l2", filter=fl[qf[i]])
            _eq(gi[i:i + 1], gd[i:i + 1], si, sd, (tag, i))
        return gi, gd

    check("as made")
    # the union as the context cached it: what the five filters allow now
    union_old = AY.eval_clauses([("own", R, 1, 1)], ids, {"own": own_col})
    for pr in preds:
        union_old |= AY.eval_clauses(pr, ids, cols)
    for S in sets:
        union_old |= np.isin(ids, S)
    # the column changes under an unchanged store: A's rows become the candidates
    own.set(ids[np.concatenate([rows_a, rows_b])], np.concatenate([np.ones(256, np.int64), np.full(256, 2, np.int64)]))
    own_col = {**{int(i): 1 for i in ids[rows_a]}, **{int(i): 2 for i in ids[rows_b]}}
    keep2 = AY.eval_clauses([("own", R, 1, 1)], ids, {"own": own_col})
    assert keep2.sum() == 256 and keep2[rows_a].all()
    # precondition: whole tiles of new candidates that the old union does not cover (the lists are tiled from their first row)
    stale_tiles = [t for t in range(16) if not union_old[rows_a[16 * t:16 * t + 16]].any()]
    assert len(stale_tiles) >= 4, stale_tiles
    gi, gd = check("after a set")
    assert fl[4].info()["rebuilds"] == 1
    oi, od = AY.search(q[mine], c["cent"], c["vecs"], ids, c["offsets"], 8, 10, "l2", keep2)
    _eq(gi[mine], gd[mine], oi, od, "the changed filter's queries")
    got = gi[mine]
    assert (got >= 0).all() and np.isin(got, ids[rows_a]).all()
    assert np.isin(got, ids[np.concatenate([rows_a[16 * t:16 * t + 16] for t in stale_tiles])]).any()  # ... from those tiles too
    for f in fl:
        f.close()
    own.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_range_search_and_tracked(ctx, corpora, metric):
    from quake_amd.capi import Filter
    c, s, parent, cols, attrs, big = corpora(metric, True)
    q = _queries(c, 20, seed=41)
    clauses = [("tenant", R, 0, 19), ("flags", NO, 0x1, 0)]
    keep = AY.eval_clauses(clauses, c["ids"], cols)
    assert 0 < keep.sum() < keep.shape[0]
    f = Filter.where(s, [(attrs[n], op, a, b) for n, op, a, b in clauses])
    fi = Filter(s, AY.allowed_set(keep, c["ids"]), "allow")
    radius = 4.6 if metric == "l2" else 0.6
    lw, iw, dw = ctx.range_search(parent, s, q, 8, radius, metric, filter=f)
    li, ii, di = ctx.range_search(parent, s, q, 8, radius, metric, filter=fi)
    assert int(lw[-1]) > 0
    np.testing.assert_array_equal(lw, li)
    _eq(iw, dw, ii, di, "range")
    assert np.isin(iw, c["ids"][keep]).all()
    gi, gd, gp = ctx.search_tracked(parent, s, q, 8, 10, metric, filter=f)
    oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 8, 10, metric, keep)
    _eq(gi, gd, oi, od, "tracked")
    ui, ud, up = ctx.search_tracked(parent, s, q, 8, 10, metric)
    np.testing.assert_array_equal(gp, up)  # the probed lists are the unfiltered search's
    f.close()
    fi.close()


def test_wide_rows(ctx):
    from quake_amd.capi import Attr, Filter
    d = 2560
    c = _corpus(d, 6, 700, "l2", seed=51, empty=2)  # two lists hold (almost) all rows
    assert (np.diff(c["offsets"]) > 16).sum() == 2
    s, parent = _stores(ctx, c)
    q = _queries(c, 9, seed=52)
    rng = np.random.default_rng(53)
    col = {int(i): int(v) for i, v in zip(c["ids"], rng.integers(0, 10, 700)) if rng.random() >= 0.1}
    a = Attr(s)
    _set_column(a, col, device=True)
    for clauses in ([("c", R, 0, 2)], [("c", NR, 0, 2), ("c", ANY, 1, 0)]):
        keep = AY.eval_clauses(clauses, c["ids"], {"c": col})
        assert 0 < keep.sum() < 700
        f = Filter.where(s, [(a, op, x, y) for _, op, x, y in clauses])
        for k, nprobe in [(10, 2), (448, 6)]:
            gi, gd = ctx.search(parent, s, q, nprobe, k, "l2", filter=f)
            assert ctx.last_scan_kernel() == "k_scan_wide (filtered)"
            oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, "l2", keep)
            _eq(gi, gd, oi, od, (clauses, k))
        assert f.info()["rows_allowed"] == int(keep.sum())
        f.close()
    a.close()
    s.close()
    parent.close()


# ---- 4. lifetime and errors --------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(ctx, corpora):
    from quake_amd.capi import Attr, Filter, Store
    from quake_amd._lib import QuakeHipError
    c, s, parent, cols, attrs, big = corpora("l2", False)
    q = _queries(c, 12, seed=61)
    # a column destroyed before its filter: the filter keeps answering with the last values, through a rebuild too
    rng = np.random.default_rng(62)
    col = {int(i): int(v) for i, v in zip(c["ids"], rng.integers(0, 3, 20000))}
    a = Attr(s)
    _set_column(a, col, device=False)
    f = Filter.where(s, [(a, R, 1, 1)])
    a.close()
    keep = AY.eval_clauses([("c", R, 1, 1)], c["ids"], {"c": col})
    oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 8, 10, "l2", keep)
    _eq(*ctx.search(parent, s, q, 8, 10, "l2", filter=f), oi, od, "column destroyed")
    assert f.info()["rows_allowed"] == int(keep.sum()) and f.info()["rebuilds"] == 0
    # ... and k_filter_build_where reads the destroyed column's data again: the store changes (a row comes and goes at the end of
    # a list, which leaves the list as it was), so the next call re-derives the mask from the values the filter still owns
    s.add_entries(big, np.array([FAR + 7], np.int64), c["vecs"][:1])
    assert s.remove_ids(np.array([FAR + 7], np.int64)) == 1
    _eq(*ctx.search(parent, s, q, 8, 10, "l2", filter=f), oi, od, "column destroyed, mask rebuilt")
    assert f.info()["rebuilds"] == 1 and f.info()["rows_allowed"] == int(keep.sum())
    f.close()
    # refusals
    other = Store(ctx, 64)
    other.build_csr(np.array([0, 4], np.int64), np.arange(4, dtype=np.int64), c["vecs"][:4])
    foreign = Attr(other)
    t = attrs["tenant"]
    for bad, what in [([(foreign, R, 0, 1)], "another store"), ([(None, R, 0, 1)], "null column"), ([(t, 5, 0, 1)], "unknown op"),
                      ([(t, -1, 0, 1)], "unknown op"), ([], "at least one clause"), ([(t, R, 0, 1), (foreign, NO, 1, 0)], "another store")]:
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*" + what):
            Filter.where(s, bad)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_CLAUSES"):
        Filter.where(s, [(t, R, 0, i) for i in range(9)])
    before = t.info()
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*negative"):
        t.set(np.array([5, -1], np.int64), np.array([1, 1], np.int64))
    assert t.info() == before  # (nothing was changed)
    f8 = Filter.where(s, [(t, R, 0, 49)] * 8)  # eight clauses are fine
    assert f8.info()["rows_allowed"] == int(AY.eval_clauses([("tenant", R, 0, 49)], c["ids"], cols).sum())
    f8.close()
    foreign.close()
    other.close()
    gi, gd = ctx.search(parent, s, q, 4, 10, "l2")  # the context still answers
    oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, 10, "l2", batched_scan=True)
    _eq(gi, gd, oi, od, "after refusals")


# ---- 5. both mirrors ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def _build(mod, x, ids, nlist, workers=0):
    idx = mod.QuakeIndex()
    bp = mod.IndexBuildParams()
    bp.nlist, bp.metric, bp.num_workers = nlist, "l2", workers
    idx.build(x, ids, bp)
    return idx


def _index_csr(idx):
    """tests/test_filtered_search.py's: the Python index's partitions as a CSR in the order of the parent's rows"""
    s = idx._store
    cent, cids = idx.parent._store.get_list(0)
    pv, pi = zip(*[s.get_list(int(p)) for p in cids])
    vecs, aids, offs = O.csr_from_partitions(pv, pi, idx._d)
    return cent, vecs, aids, offs


def test_both_mirrors_through_a_stream_of_changes(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(71)
    n, d = 6000, 32
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(40, d, generator=g)
    rng = np.random.default_rng(72)
    cols = {"tenant": {int(i): int(v) for i, v in zip(ids, rng.integers(0, 8, n)) if rng.random() >= 0.05},
            "ts": {int(i): int(v) for i, v in zip(ids, rng.integers(-(1 << 40), 1 << 40, n))}}
    where = [("tenant", "between", 1, 5), ("tenant", "!=", 3), ("ts", ">=", -(1 << 39)), ("ts", "<", 1 << 70)]
    idxs = {"python": _build(quake, x, ids, 20), "compiled": _build(qb, x, ids, 20)}
    sps, filters = {}, {}
    for name, idx in idxs.items():
        mod = quake if name == "python" else qb
        assert idx.attribute_names() == []
        for cn, col in cols.items():
            k = torch.tensor(list(col.keys()), dtype=torch.int64)
            v = torch.tensor(list(col.values()), dtype=torch.int64)
            idx.set_attribute(cn, k.cuda() if cn == "ts" else k, v.cuda() if cn == "ts" else v)
        assert idx.attribute_names() == ["tenant", "ts"]
        sps[name] = mod.SearchParams()
        sps[name].k, sps[name].nprobe = 10, 5
        filters[name] = idx.make_filter(where=where)
        assert filters[name].info()["n_ids"] == -1

    def check(tag):
        py = idxs["python"]
        cent, cv, ci, co = _index_csr(py)
        keep = AY.eval_where(where, ci, cols)
        assert 0 < keep.sum() < keep.shape[0], tag
        oi, od = AY.search(q.numpy(), cent, cv, ci, co, 5, 10, "l2", keep)
        out = {}
        for name, idx in idxs.items():
            sps[name].filter = filters[name]
            r = idx.search(q, sps[name])
            sps[name].filter = None
            out[name] = r
            assert filters[name].info()["rows_allowed"] == int(keep.sum()), (tag, name)
        _eq(out["python"].ids, out["python"].distances, oi, od, (tag, "python"))
        assert sorted(idxs["compiled"].get_ids().tolist()) == sorted(py.get_ids().tolist()), tag
        _eq(out["compiled"].ids, out["compiled"].distances, oi, od, (tag, "compiled"))

    def each(fn):
        for idx in idxs.values():
            fn(idx)

    check("as built")
    na = 500
    ax, aid = torch.randn(na, d, generator=g), torch.arange(20000, 20000 + na)
    each(lambda idx: idx.add(ax, aid))
    check("add (no values yet)")
    av = torch.from_numpy(rng.integers(0, 8, na))
    cols["tenant"].update({int(i): int(v) for i, v in zip(aid, av)})
    cols["ts"].update({int(i): 7 for i in aid})
    each(lambda idx: (idx.set_attribute("tenant", aid, av), idx.set_attribute("ts", aid, torch.full((na,), 7))))
    check("values for the added rows")
    rem = ids[:800]
    each(lambda idx: idx.remove(rem))
    check("remove")
    # modify = remove + add: the attributes stay with the ids
    mid = ids[800:1100]
    mx = torch.randn(300, d, generator=g)
    each(lambda idx: idx.modify(mid, mx))
    check("modify")
    for name, idx in idxs.items():
        vals, found = idx.get_attribute("ts", mid)
        assert bool(found.all()) and vals.tolist() == [cols["ts"][int(i)] for i in mid], name
    each(lambda idx: idx.refine_partitions(torch.tensor([0, 1, 2, 3]), 2))
    check("refine_partitions")
    each(lambda idx: idx.maintenance())
    check("maintenance")
    un = ids[1100:1400]
    each(lambda idx: idx.unset_attribute("tenant", un))
    for i in un:
        cols["tenant"].pop(int(i), None)
    check("unset_attribute")
    vals, found = idxs["compiled"].get_attribute("tenant", un[:5])
    assert not bool(found.any())


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(81)
    x = torch.randn(3000, 16, generator=g)
    ids = torch.arange(3000)
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 8)
        idx.set_attribute("a", ids, ids % 5)
        with pytest.raises(RuntimeError, match="unknown attribute column"):
            idx.make_filter(where=[("b", "==", 1)])
        with pytest.raises(RuntimeError, match="unknown where op"):
            idx.make_filter(where=[("a", "=~", 1)])
        with pytest.raises(RuntimeError, match="9 clauses"):
            idx.make_filter(where=[("a", "==", 1)] * 9)
        with pytest.raises(RuntimeError, match="at least one clause"):
            idx.make_filter(where=[])
        with pytest.raises(RuntimeError, match="exactly one of"):
            idx.make_filter()
        with pytest.raises(RuntimeError, match="exactly one of"):
            idx.make_filter(ids[:5], where=[("a", "==", 1)])
        with pytest.raises(RuntimeError, match="unknown attribute column"):
            idx.get_attribute("b", ids[:5])
        with pytest.raises(RuntimeError, match="unknown attribute column"):
            idx.unset_attribute("b", ids[:5])
        f = idx.make_filter(ids[:100], True)  # the positional form still works
        assert f.info()["n_ids"] == 100
        f = idx.make_filter(where=[("a", "==", 1 << 70)])  # no int64 equals 2^70
        assert f.info()["rows_allowed"] == 0
        f = idx.make_filter(where=[("a", "any_bits", (1 << 64) - 1)])
        assert f.info()["rows_allowed"] == 3000 - 600  # every value but 0
        grp = _build(mod, x, ids, 8, workers=2)
        with pytest.raises(RuntimeError, match="filtered search is not supported with num_workers > 0"):
            grp.set_attribute("a", ids, ids)
        with pytest.raises(RuntimeError, match="filtered search is not supported with num_workers > 0"):
            grp.make_filter(where=[("a", "==", 1)])
