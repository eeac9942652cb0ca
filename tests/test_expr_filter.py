"""Expression filters on the GPU (qk_filter_create_expr; Filter.expr; make_filter(any_of=) and the set ops of make_filter(where=) in
both mirrors): an OR of conjunctions over attribute columns, with the value sets IN_SET / NOT_IN_SET, turned into the row mask of a
qk_filter by k_filter_build_expr.

The equation under test: at any moment an expression filter answers exactly like the QK_FILTER_ALLOW id-set filter over
{id : every clause of some term holds for id}.  Every comparison is bit for bit -- ids, and the uint32 view of the distances --
against tests/expr_yardstick.py (a numpy evaluation of the terms, then the oracle's search over the CSR with the other rows deleted)
and, on top of that, against an id-set filter made from the yardstick's id set and against the same expression with its terms and
clauses permuted.

Shapes: the corpus and the columns of tests/test_attr_filter.py (20 000 x 64 in 64 skewed lists: empty lists, lists of 5 and 7
rows, lengths that are no multiple of 16, a list longer than the 1024 rows a block of k_filter_build_expr covers per step, so two
block rows share it; `tenant` and `flags` direct tables, `ts` sorted pairs, the sparse-id variant all sorted): the smallest at which
the kernel's tiling, its chunk stride and both lookups can go wrong."""
import zlib

import numpy as np
import pytest
import torch

import attr_yardstick as AY
import expr_yardstick as EY
import filter_yardstick as Y
import oracle as O

pytestmark = pytest.mark.gpu

MIN, MAX = AY.INT64_MIN, AY.INT64_MAX
FAR = 1 << 45  # an id nobody stores: a value for it alone pushes a column out of the table layout
SPARSE_STEP = 54_975_581  # ids up to ~2^40


def _corpus(d, nlist, n, metric, seed, empty=2, id_base=7, id_step=1):
    """tests/test_attr_filter.py's: clustered rows in skewed lists, `empty` empty lists, a list of 5 and one of 7 rows"""
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
    """tests/test_attr_filter.py's three columns over the corpus' ids as dicts id -> value.  `tenant`: 0 .. 49, missing for ~5 % of
    the stored ids, constant 3 over the first 64 rows of the longest list and 4 over the next 64 -- whole tiles of candidates next
    to whole tiles of none; `ts`: the whole int64 range with both extremes, missing for ~10 %; `flags`: 16 random bits, every
    stored id.  All hold ids nobody stores."""
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


def _capi_terms(terms, attrs):
    """the yardstick's (name, op, a, b, values) as Filter.expr takes them"""
    return [[(attrs[n], op, a, b) if values is None else (attrs[n], op, values) for n, op, a, b, values in t] for t in terms]


def _permuted(terms, rng):
    return [[t[i] for i in rng.permutation(len(t))] for t in (terms[j] for j in rng.permutation(len(terms)))][::-1]


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    """(corpus, store, parent, column dicts, Attrs, longest list) per (metric, sparse), as in tests/test_attr_filter.py.  Dense ids:
    `tenant` and `flags` are tables, `ts` also holds FAR and is sorted; sparse ids: all sorted."""
    from quake_amd.capi import Attr
    cache = {}

    def get(metric, sparse):
        key = (metric, sparse)
        if key not in cache:
            c = _corpus(64, 64, 20000, metric, seed=188 if metric == "ip" else 183, id_step=SPARSE_STEP if sparse else 1)
            sizes = np.diff(c["offsets"])
            assert (sizes == 0).sum() >= 2 and ((sizes > 0) & (sizes < 16)).sum() >= 2 and (sizes % 16 != 0).any()
            assert sizes.max() > 1024  # two block rows (blockIdx.y = 0, 1) share the longest list
            s, parent = _stores(ctx, c)
            cols, big = _columns(c, seed=9 + sparse)
            if not sparse:
                cols["ts"][FAR] = 5
            attrs = {}
            for name, col in cols.items():
                attrs[name] = Attr(s)
                _set_column(attrs[name], col, device=metric == "ip")
            lay = {name: a.info()["layout"] for name, a in attrs.items()}
            assert lay == (dict(tenant="sorted", ts="sorted", flags="sorted") if sparse else dict(tenant="table", ts="sorted", flags="table"))
            assert any(int(i) not in cols["tenant"] for i in c["ids"]) and any(int(i) not in cols["ts"] for i in c["ids"])
            cache[key] = (c, s, parent, cols, attrs, big)
        return cache[key]

    yield get
    for c, s, p, cols, attrs, big in cache.values():
        for a in attrs.values():
            a.close()
        s.close()
        p.close()


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
R, NR, ANY, ALL, NO, IN, NIN = "range", "not_range", "any_bits", "all_bits", "no_bits", "in", "not_in"
EIGHT = [("tenant", R, 0, 40, None), ("tenant", NR, 7, 7, None), ("ts", R, -(1 << 62), 1 << 62, None), ("ts", NR, -50, 50, None),
         ("flags", ANY, 0xFF, 0, None), ("flags", NO, 0x8000, 0, None), ("flags", ALL, 0x1, 0, None), ("tenant", R, 1, 49, None)]
TENANT_SETS = {0: [], 1: [17], 2: [49, 0], 3: [3, 4, 30], 7: [9, 2, 2, 44, 3, 21, 38, 2, 10], 8: list(range(40, 48)),
               9: [1, 2, 5, 8, 13, 21, 34, 55, 89, -1, 47, 48], 50: list(range(49, -1, -1))}


def _ts_set(cols):
    """about 1000 values: 500 stored ones, as many misses, and both extremes -- values below and above every element are met"""
    rng = np.random.default_rng(77)
    stored = np.array(sorted(set(cols["ts"].values())), np.int64)
    hits = stored[rng.permutation(stored.shape[0])[:500]]
    miss = np.setdiff1d(rng.integers(-5000, 5000, 1500), stored)
    miss = miss[rng.permutation(miss.shape[0])[:500]]
    return [int(v) for v in rng.permutation(np.concatenate([hits, miss, np.array([MIN, MAX], np.int64)]))]


def _exprs():
    """(name, terms or a function of the column dicts, what the case must show): "where" one old clause -- also compared with
    Filter.where --, "all" every stored row with a flags value, "none" no row, "pad" a padded result row, "tiles" a tile word 0 and
    a tile word 0xFFFF, "some" neither no row nor every row, "layouts" the columns of the two terms are kept in different layouts"""
    ex = [("one old clause", [[("tenant", NR, 0, 24, None)]], "where some")]
    for n, vals in TENANT_SETS.items():
        assert len(set(v for v in vals if 0 <= v < 50)) == n
        ex.append(("in %d" % n, [[("tenant", IN, 0, 0, vals)]], "none pad" if n == 0 else "some"))
        ex.append(("not_in %d" % n, [[("tenant", NIN, 0, 0, vals)]], "none pad" if n == 50 else "some"))
    ex += [
        ("ts in ~1000", lambda cols: [[("ts", IN, 0, 0, _ts_set(cols))]], "some"),
        ("flags in 70001", [[("flags", IN, 0, 0, np.arange(0, 140001, 2, dtype=np.int64)[::-1])]], "some"),
        ("2 terms, 2 layouts", [[("tenant", R, 0, 9, None)], [("ts", R, -1000, 1000, None)]], "some layouts"),
        ("8 terms", [[("tenant", R, 5 * i, 5 * i, None), ("flags", ANY, 1 << i, 0, None)] for i in range(7)] +
         [[("ts", IN, 0, 0, [MIN, MAX, -1, 0, 12345])]], "some"),
        ("32 clauses", [EIGHT, EIGHT[::-1][:7] + [("tenant", NIN, 0, 0, [1, 2, 3])], [("ts", IN, 0, 0, list(range(-300, 300)))] +
                        [("flags", NO, 1 << b, 0, None) for b in range(7)], [("tenant", IN, 0, 0, [3, 4])] + EIGHT[1:]], "some"),
        ("empty or live", [[("tenant", R, 5, 4, None), ("flags", NO, 0, 0, None)], [("tenant", IN, 0, 0, [11, 12])]], "some"),
        ("all terms empty", [[("tenant", R, 5, 4, None)], [("ts", IN, 0, 0, [])], [("flags", ANY, 0, 0, None)],
                             [("tenant", NIN, 0, 0, list(range(50)))]], "none pad"),
        ("every row", [[("flags", ANY, 1, 0, None)], [("flags", NIN, 0, 0, [1, 3, 5]), ("flags", NO, 1, 0, None)]], "all"),
        ("tenant 3 or 4", [[("tenant", R, 3, 3, None)], [("tenant", IN, 0, 0, [4])]], "tiles some"),
    ]
    return ex


EXPRS = _exprs()
# axis values a case needs to show what it is there to show (the other axes are dealt): a table next to sorted pairs exists on
# the dense-id corpus only
PINNED = {"2 terms, 2 layouts": dict(sparse=False)}


def _grid():
    """every expression once, the other axes dealt round by seeded shuffles (every value of every axis appears)"""
    axes = dict(metric=["l2", "ip"], sparse=[False, True], mem=["host", "device"], entry=["search", "coarse+scan"], nprobe=[1, 8, 32],
                k=[1, 10, 100], Q=[1, 33, 300])
    rng = np.random.default_rng(20260115)
    n = len(EXPRS)
    cols = {}
    for name, vals in axes.items():
        seq = []
        while len(seq) < n:
            seq += [vals[i] for i in rng.permutation(len(vals))]
        cols[name] = seq[:n]
    cases = [dict(ex=i, **{name: cols[name][i] for name in axes}) for i in range(n)]
    for c in cases:
        c.update(PINNED.get(EXPRS[c["ex"]][0], {}))
    assert all(k in axes and v in axes[k] for pin in PINNED.values() for k, v in pin.items()) and set(PINNED) <= {e[0] for e in EXPRS}
    for name, vals in axes.items():
        assert {c[name] for c in cases} == set(vals), name
    return cases


@pytest.mark.parametrize("case", _grid(), ids=lambda c: EXPRS[c["ex"]][0].replace(" ", "_") + "-" + "-".join(str(v) for v in list(c.values())[1:]))
def test_grid(ctx, corpora, case):
    from quake_amd.capi import Filter
    c, s, parent, cols, attrs, big = corpora(case["metric"], case["sparse"])
    name, terms, shows = EXPRS[case["ex"]]
    terms = terms(cols) if callable(terms) else terms
    metric, nprobe, k, Q = case["metric"], case["nprobe"], case["k"], case["Q"]
    rng = np.random.default_rng(zlib.crc32(repr(sorted(case.items())).encode()))
    q = _queries(c, Q, seed=int(rng.integers(1 << 30)))
    if "pad" in shows:
        k = max(k, 100)  # (no candidate in the whole store: short rows)
    keep = EY.eval_expr(terms, c["ids"], cols)
    S = AY.allowed_set(keep, c["ids"])
    if "all" in shows:
        assert keep.all()
    if "none" in shows:
        assert not keep.any()
    if "some" in shows:
        assert 0 < keep.sum() < keep.shape[0]
    if "tiles" in shows:
        words = AY.tile_words(keep, c["offsets"])
        assert (words == 0).any() and (words == 0xFFFF).any()
    if "layouts" in shows:
        assert len(terms) == 2 and attrs[terms[0][0][0]].info()["layout"] == "table" and attrs[terms[1][0][0]].info()["layout"] == "sorted"
        each = [EY.eval_expr([t], c["ids"], cols) for t in terms]  # (both terms decide rows of their own)
        assert (each[0] & ~each[1]).any() and (each[1] & ~each[0]).any()
    if name == "8 terms":
        assert len(terms) == 8 and len({attrs[cl[0]].info()["layout"] for t in terms for cl in t}) == (1 if case["sparse"] else 2)
    if name == "32 clauses":
        assert sum(len(t) for t in terms) == 32
    if name == "flags in 70001":
        assert len(terms[0][0][4]) > 65536
    if name == "empty or live":
        assert not EY.eval_expr(terms[:1], c["ids"], cols).any() and EY.eval_expr(terms[1:], c["ids"], cols).any()
    if name == "ts in ~1000":
        vals = terms[0][0][4]
        assert 990 <= len(vals) <= 1010 and MIN in vals and MAX in vals
        stored = set(cols["ts"].values())
        assert sum(v in stored for v in vals) >= 400 and sum(v not in stored for v in vals) >= 400
    oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, keep)
    if "pad" in shows:
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

    fl = [Filter.expr(s, _capi_terms(terms, attrs)), Filter.expr(s, _capi_terms(_permuted(terms, rng), attrs)), Filter(s, S, "allow")]
    if "where" in shows:
        fl.append(Filter.where(s, [(attrs[n], op, a, b) for n, op, a, b, _ in terms[0]]))
    try:
        gi, gd = run(fl[0])
        _eq(gi, gd, oi, od, case)
        _eq(*run(fl[2]), oi, od, (case, "id set"))
        _eq(*run(fl[1]), oi, od, (case, "term and clause order"))
        got = _np(gi)
        assert np.isin(got[got >= 0], S).all()
        for flt in fl[:2]:
            info = flt.info()
            assert info["n_ids"] == -1 and info["rebuilds"] == 0 and info["rows_allowed"] == int(keep.sum())
            assert info["device_bytes"] > 0
        if "where" in shows:
            _eq(*run(fl[3]), oi, od, (case, "Filter.where"))
            assert fl[3].info()["rows_allowed"] == fl[0].info()["rows_allowed"] == int(keep.sum())
    finally:
        for f in fl:
            f.close()


def test_device_bytes_count_the_sets(ctx, corpora):
    from quake_amd.capi import Filter
    c, s, parent, cols, attrs, big = corpora("l2", False)
    t = attrs["tenant"]
    f0 = Filter.expr(s, [[(t, R, 0, 5)]])
    f1 = Filter.expr(s, [[(t, IN, [5, 5, 4, 3])], [(t, NIN, list(range(1000)))]])  # 3 + 1000 distinct values
    assert f1.info()["device_bytes"] - f0.info()["device_bytes"] == (1003 - 1) * 8
    f0.close()
    f1.close()


# ---- 2. liveness -----------------------------------------------------------------------------------------------------------------
def _store_csr(s, nlist, d):
    pv, pi = zip(*[s.get_list(p) for p in range(nlist)])
    return O.csr_from_partitions(pv, pi, d)


def test_liveness(ctx):
    from quake_amd.capi import Attr, Filter
    c = _corpus(64, 64, 20000, "l2", seed=271)
    s, parent = _stores(ctx, c)
    nlist, d = 64, 64
    rng = np.random.default_rng(272)
    q = _queries(c, 40, seed=273)
    ids = c["ids"]
    cola = {int(i): int(v) for i, v in zip(ids, rng.integers(0, 20, ids.shape[0])) if rng.random() >= 0.1}
    colb = {int(i): int(v) for i, v in zip(ids, rng.integers(0, 20, ids.shape[0])) if rng.random() >= 0.1}
    a, b = Attr(s), Attr(s)
    _set_column(a, cola, device=False)
    _set_column(b, colb, device=True)
    # b is named by the second term only, a by both
    terms = [[("a", R, 0, 2, None)], [("b", IN, 0, 0, [7, 3]), ("a", NIN, 0, 0, [19, 18])]]
    f = Filter.expr(s, _capi_terms(terms, dict(a=a, b=b)))
    state = dict(rebuilds=0, last=None, keep=None)

    def check(tag, rebuilt, changed=None):
        vecs, cids, offs = _store_csr(s, nlist, d)
        keep = EY.eval_expr(terms, cids, dict(a=cola, b=colb))
        assert 0 < keep.sum() < keep.shape[0], tag
        S = AY.allowed_set(keep, cids)
        if changed is not None:
            assert (not np.array_equal(S, state["keep"])) == changed, tag
        state["keep"] = S
        oi, od = AY.search(q, c["cent"], vecs, cids, offs, 8, 100, "l2", keep)
        for again in (False, True):  # the second call finds nothing changed
            gi, gd = ctx.search(parent, s, q, 8, 100, "l2", filter=f)
            _eq(gi, gd, oi, od, (tag, again))
            info = f.info()
            state["rebuilds"] += 1 if rebuilt and not again else 0
            assert info["rebuilds"] == state["rebuilds"], (tag, again, info)
            assert info["rows_allowed"] == int(keep.sum()), tag
        if changed is False and rebuilt is False:
            _eq(gi, gd, *state["last"], tag)
        state["last"] = (gi, gd)
        fi = Filter(s, S, "allow")
        _eq(*ctx.search(parent, s, q, 8, 100, "l2", filter=fi), oi, od, (tag, "id set"))
        fi.close()

    check("as made", rebuilt=False)
    # the column of the second term alone changes: one rebuild, another answer
    upd = ids[rng.permutation(ids.shape[0])[:500]]
    b.set(upd, np.full(500, 7, np.int64))
    colb.update({int(i): 7 for i in upd})
    check("set in the second term's column", rebuilt=True, changed=True)
    gone = np.concatenate([upd[:150], ids[:150], np.array([FAR, 3], np.int64)])  # (ids without a value are ignored)
    b.unset(torch.from_numpy(gone).cuda())
    for i in gone:
        colb.pop(int(i), None)
    check("unset", rebuilt=True, changed=True)
    # the column two terms name
    upd = ids[rng.permutation(ids.shape[0])[:500]]
    newv = rng.integers(0, 20, 500)
    a.set(upd, newv)
    cola.update({int(i): int(v) for i, v in zip(upd, newv)})
    check("set in the column of two terms", rebuilt=True, changed=True)
    # both columns between two calls: still one rebuild
    a.set(ids[:10], np.zeros(10, np.int64))
    b.set(ids[:10], np.zeros(10, np.int64))
    cola.update({int(i): 0 for i in ids[:10]})
    colb.update({int(i): 0 for i in ids[:10]})
    check("both columns", rebuilt=True)
    # rows are added: without values they are no candidates; then they get values
    new_ids = np.arange(30000, 30600, dtype=np.int64)
    newx = (c["cent"][10] + 0.4 * rng.standard_normal((600, d))).astype(np.float32)
    s.add_entries(10, new_ids, newx)
    check("add", rebuilt=True, changed=False)
    a.set(new_ids, np.full(600, 5, np.int64))
    b.set(new_ids, np.where(np.arange(600) % 2 == 0, 3, 4).astype(np.int64))
    cola.update({int(i): 5 for i in new_ids})
    colb.update({int(i): 3 if j % 2 == 0 else 4 for j, i in enumerate(new_ids)})
    check("values for the added rows", rebuilt=True, changed=True)
    rem = new_ids[:200]
    assert s.remove_ids(rem) == 200
    check("remove", rebuilt=True, changed=True)
    check("nothing changed", rebuilt=False, changed=False)
    # the columns are closed while the filter lives: it keeps answering, through a rebuild too
    a.close()
    b.close()
    check("columns closed", rebuilt=False, changed=False)
    s.add_entries(10, np.array([FAR + 7], np.int64), c["vecs"][:1])
    assert s.remove_ids(np.array([FAR + 7], np.int64)) == 1
    check("columns closed, mask rebuilt", rebuilt=True, changed=False)
    f.close()
    s.close()
    parent.close()


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------
COMP = [[("tenant", IN, 0, 0, [1, 2, 3, 5, 8, 13, 21, 34]), ("flags", NO, 0x1, 0, None)], [("ts", R, -1000, 1000, None), ("tenant", NIN, 0, 0, [0, 7])]]


def _pair(corpora, metric, sparse, terms=COMP):
    """(corpus tuple, the expression filter, the id-set filter over the yardstick's set, keep)"""
    from quake_amd.capi import Filter
    t = corpora(metric, sparse)
    c, s, parent, cols, attrs, big = t
    keep = EY.eval_expr(terms, c["ids"], cols)
    assert 0 < keep.sum() < keep.shape[0]
    return t, Filter.expr(s, _capi_terms(terms, attrs)), Filter(s, AY.allowed_set(keep, c["ids"]), "allow"), keep


def test_per_query_table_mixes_expressions_predicates_and_id_sets(ctx, corpora):
    from quake_amd.capi import Filter
    (c, s, parent, cols, attrs, big), fe, fi, keep = _pair(corpora, "l2", False)
    rng = np.random.default_rng(31)
    fw = Filter.where(s, [(attrs["tenant"], R, 3, 3)])
    fs = Filter(s, Y.draw_set(c["ids"], 0.01, rng), "allow")
    fe2 = Filter.expr(s, [[(attrs["flags"], ALL, 0xFF0, 0)], [(attrs["tenant"], IN, [44])]])
    fl = [fe, fw, fs, fe2]
    qf = rng.permutation(np.arange(40) % len(fl)).astype(np.int32)
    q = _queries(c, 40, seed=32)
    gi, gd = ctx.search(parent, s, q, 8, 10, "l2", filters=fl, query_filter=qf)
    assert "per query" in ctx.last_scan_kernel()
    hi, hd = ctx.search(parent, s, q, 8, 10, "l2", filters=[fi, fw, fs, fe2], query_filter=qf)
    _eq(gi, gd, hi, hd, "the id set in the expression's place")
    for i in range(40):
        _eq(gi[i:i + 1], gd[i:i + 1], *ctx.search(parent, s, q[i:i + 1], 8, 10, "l2", filter=fl[qf[i]]), i)
    mine = np.flatnonzero(qf == 0)
    oi, od = AY.search(q[mine], c["cent"], c["vecs"], c["ids"], c["offsets"], 8, 10, "l2", keep)
    _eq(gi[mine], gd[mine], oi, od, "the expression's queries")
    for f in fl + [fi]:
        f.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_range_search(ctx, corpora, metric):
    (c, s, parent, cols, attrs, big), fe, fi, keep = _pair(corpora, metric, True)
    q = _queries(c, 20, seed=41)
    radius = 4.6 if metric == "l2" else 0.6
    le, ie, de = ctx.range_search(parent, s, q, 8, radius, metric, filter=fe)
    li, ii, di = ctx.range_search(parent, s, q, 8, radius, metric, filter=fi)
    assert int(le[-1]) > 0
    np.testing.assert_array_equal(le, li)
    _eq(ie, de, ii, di, "range")
    assert np.isin(ie, c["ids"][keep]).all()
    fe.close()
    fi.close()


def test_adaptive_exact_grouped_paged(ctx, corpora):
    (c, s, parent, cols, attrs, big), fe, fi, keep = _pair(corpora, "l2", False)
    q = _queries(c, 25, seed=51)
    # adaptive probing: the per-list counts come from the mask
    re_, ri = (ctx.search_adaptive(parent, s, q, 1, 32, 200, "l2", filter=f) for f in (fe, fi))
    _eq(re_[0], re_[1], ri[0], ri[1], "adaptive")
    np.testing.assert_array_equal(_np(re_[2]), _np(ri[2]))
    np.testing.assert_array_equal(_np(re_[3]), _np(ri[3]))
    assert (_np(re_[2]) > 1).any()
    # exact search: the candidate store is gathered from the mask
    assert fe.candidate_rows(ctx) == int(keep.sum())
    _eq(*ctx.search_exact(s, q, 20, "l2", fe)[:2], *ctx.search_exact(s, q, 20, "l2", fi)[:2], "exact")
    assert fe.exact_info()["rows"] == int(keep.sum())
    qf = (np.arange(25) % 2).astype(np.int32)
    from quake_amd.capi import Filter
    fw = Filter.where(s, [(attrs["tenant"], R, 3, 9)])
    be = ctx.search_exact_batch(s, q, 20, "l2", [fe, fw], qf)
    bi = ctx.search_exact_batch(s, q, 20, "l2", [fi, fw], qf)
    _eq(be[0], be[1], bi[0], bi[1], "exact per query")
    # grouped search
    ge = ctx.search_grouped(parent, s, q, 8, 10, "l2", attrs["tenant"], filter=fe)
    gi = ctx.search_grouped(parent, s, q, 8, 10, "l2", attrs["tenant"], filter=fi)
    _eq(ge[0], ge[1], gi[0], gi[1], "grouped")
    np.testing.assert_array_equal(_np(ge[2]), _np(gi[2]))
    assert (_np(ge[0]) >= 0).any()
    # two pages
    pe = ctx.search_after(parent, s, q, 8, 10, "l2", filter=fe)
    pi = ctx.search_after(parent, s, q, 8, 10, "l2", filter=fi)
    _eq(pe[0], pe[1], pi[0], pi[1], "page 1")
    oi, od = ctx.search(parent, s, q, 8, 20, "l2", filter=fi)
    pe2 = ctx.search_after(parent, s, q, 8, 10, "l2", after=pe[2], filter=fe)
    pi2 = ctx.search_after(parent, s, q, 8, 10, "l2", after=pi[2], filter=fi)
    _eq(pe2[0], pe2[1], pi2[0], pi2[1], "page 2")
    _eq(np.concatenate([_np(pe[0]), _np(pe2[0])], 1), np.concatenate([_np(pe[1]), _np(pe2[1])], 1), oi, od, "two pages")
    for f in (fe, fi, fw):
        f.close()


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
    terms = [[("c", IN, 0, 0, [0, 2, 9])], [("c", NR, 0, 6, None), ("c", ANY, 1, 0, None)]]
    keep = EY.eval_expr(terms, c["ids"], {"c": col})
    assert 0 < keep.sum() < 700
    f = Filter.expr(s, _capi_terms(terms, {"c": a}))
    fi = Filter(s, AY.allowed_set(keep, c["ids"]), "allow")
    for k, nprobe in [(10, 2), (448, 6)]:
        gi, gd = ctx.search(parent, s, q, nprobe, k, "l2", filter=f)
        assert ctx.last_scan_kernel() == "k_scan_wide (filtered)"
        oi, od = AY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, "l2", keep)
        _eq(gi, gd, oi, od, k)
        _eq(*ctx.search(parent, s, q, nprobe, k, "l2", filter=fi), oi, od, (k, "id set"))
    assert f.info()["rows_allowed"] == int(keep.sum())
    for o in (f, fi, a, s, parent):
        o.close()


# ---- 4. errors and lifetime --------------------------------------------------------------------------------------------------------
def _create_raw(s, clauses, term_sizes):
    """qk_filter_create_expr with the arguments as given: clauses (attr, op, a, b, set pointer or None, n_set); rows_allowed"""
    import ctypes as C
    from quake_amd import _lib
    arr = (_lib.QkExprClause * max(len(clauses), 1))()
    for i, (attr, op, a, b, ptr, n) in enumerate(clauses):
        arr[i].attr = attr.h if attr is not None else None
        arr[i].op, arr[i].a, arr[i].b, arr[i].n_set = int(op), int(a), int(b), int(n)
        if ptr is not None:
            arr[i].set = ptr
    sizes = (C.c_int * max(len(term_sizes), 1))(*term_sizes)
    h, ra = C.c_void_p(), C.c_int64()
    _lib.check(s.lib.qk_filter_create_expr(s.h, arr, sizes, len(term_sizes), C.byref(h)))
    _lib.check(s.lib.qk_filter_info(h, None, C.byref(ra), None, None, None))
    _lib.check(s.lib.qk_filter_destroy(h))
    return ra.value


def test_errors(ctx, corpora):
    import ctypes as C
    from quake_amd.capi import Attr, Filter, Store
    from quake_amd._lib import QK_MAX_SET_VALUES, QuakeHipError
    c, s, parent, cols, attrs, big = corpora("l2", False)
    other = Store(ctx, 64)
    other.build_csr(np.array([0, 4], np.int64), np.arange(4, dtype=np.int64), c["vecs"][:4])
    foreign = Attr(other)
    t = attrs["tenant"]
    ok = (t, 0, 0, 1, None, 0)
    buf = (C.c_int64 * 1)(5)
    one = C.cast(buf, C.POINTER(C.c_int64))
    for clauses, sizes, what in [([], [], "at least one term"), ([ok], [0], "term 0 needs at least one clause"),
                                 ([ok, ok], [2, -1], "term 1 needs at least one clause"),
                                 ([(None, 0, 0, 1, None, 0)], [1], "null column"), ([ok, (foreign, 0, 0, 1, None, 0)], [1, 1], "another store"),
                                 ([(t, 7, 0, 1, None, 0)], [1], "unknown op 7"), ([(t, -1, 0, 1, None, 0)], [1], "unknown op -1"),
                                 ([(t, 5, 0, 0, one, -1)], [1], "negative n_set"), ([ok, (t, 6, 0, 0, None, 3)], [2], "null set")]:
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*" + what):
            _create_raw(s, clauses, sizes)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_TERMS"):
        Filter.expr(s, [[(t, R, 0, 1)]] * 9)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*33 clauses.*QK_MAX_EXPR_CLAUSES"):
        Filter.expr(s, [[(t, R, 0, 1)] * 11] * 3)
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_SET_VALUES"):
        Filter.expr(s, [[(t, IN, np.zeros(QK_MAX_SET_VALUES + 1, np.int64))]])
    # the limits themselves are fine: a term may hold more than 8 clauses here, and a set 2^20 values as given
    keep = AY.eval_clauses([("tenant", R, 0, 24)], c["ids"], cols)
    f = Filter.expr(s, [[(t, R, 0, 49)] * 25, [(t, R, 0, 24)] * 7])
    assert f.info()["rows_allowed"] == int(AY.eval_clauses([("tenant", R, 0, 49)], c["ids"], cols).sum())
    f.close()
    f = Filter.expr(s, [[(t, R, 0, 24)]] * 8)
    assert f.info()["rows_allowed"] == int(keep.sum())
    f.close()
    f = Filter.expr(s, [[(t, IN, np.arange(QK_MAX_SET_VALUES, dtype=np.int64) % 25)]])
    assert f.info()["rows_allowed"] == int(keep.sum())
    f.close()
    # set / n_set are read by the set ops only
    assert _create_raw(s, [(t, 0, 0, 24, None, -5)], [1]) == int(keep.sum())
    # qk_filter_create_where is what it was
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*unknown op"):
        Filter.where(s, [(t, 5, 0, 1)])
    foreign.close()
    other.close()
    q = _queries(c, 12, seed=61)
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
    """the Python index's partitions as a CSR in the order of the parent's rows"""
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
    exprs = {"any_of": [[("tenant", "==", 7), ("ts", ">=", 0)], [("tenant", "in", [1, 3, 1 << 70]), ("ts", "<", 1 << 70)],
                        [("tenant", "not_in", [0, 1, 2, 3, 4, 5, 7, -(1 << 70)]), ("ts", "between", -(1 << 39), 1 << 39)]],
             "where": [[("tenant", "in", (5, 2, 2, 6)), ("ts", "!=", 7)]]}
    idxs = {"python": _build(quake, x, ids, 20), "compiled": _build(qb, x, ids, 20)}
    sps, filters = {}, {}
    for name, idx in idxs.items():
        mod = quake if name == "python" else qb
        for cn, col in cols.items():
            k = torch.tensor(list(col.keys()), dtype=torch.int64)
            v = torch.tensor(list(col.values()), dtype=torch.int64)
            idx.set_attribute(cn, k.cuda() if cn == "ts" else k, v.cuda() if cn == "ts" else v)
        sps[name] = mod.SearchParams()
        sps[name].k, sps[name].nprobe = 10, 5
        filters[name] = {"any_of": idx.make_filter(any_of=exprs["any_of"]), "where": idx.make_filter(where=exprs["where"][0])}
        for f in filters[name].values():
            assert f.info()["n_ids"] == -1

    def check(tag):
        py = idxs["python"]
        cent, cv, ci, co = _index_csr(py)
        assert sorted(idxs["compiled"].get_ids().tolist()) == sorted(py.get_ids().tolist()), tag
        for form, any_of in exprs.items():
            keep = EY.eval_any_of(any_of, ci, cols)
            assert 0 < keep.sum() < keep.shape[0], (tag, form)
            oi, od = AY.search(q.numpy(), cent, cv, ci, co, 5, 10, "l2", keep)
            for name, idx in idxs.items():
                for flt in (filters[name][form], idx.make_filter(ids=torch.from_numpy(AY.allowed_set(keep, ci)))):
                    sps[name].filter = flt
                    r = idx.search(q, sps[name])
                    sps[name].filter = None
                    _eq(r.ids, r.distances, oi, od, (tag, form, name))
                assert filters[name][form].info()["rows_allowed"] == int(keep.sum()), (tag, form, name)

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
    cols["ts"].update({int(i): 9 for i in aid})
    each(lambda idx: (idx.set_attribute("tenant", aid, av), idx.set_attribute("ts", aid, torch.full((na,), 9))))
    check("values for the added rows")
    each(lambda idx: idx.remove(ids[:800]))
    check("remove")
    each(lambda idx: idx.maintenance())
    check("maintenance")


def test_mirror_refusals(qb):
    import quake_amd as quake
    g = torch.Generator().manual_seed(81)
    x = torch.randn(3000, 16, generator=g)
    ids = torch.arange(3000)
    one = [("a", "==", 1)]
    for mod in (quake, qb):
        idx = _build(mod, x, ids, 8)
        idx.set_attribute("a", ids, ids % 5)
        for kw in (dict(), dict(ids=ids[:5], any_of=[one]), dict(where=one, any_of=[one]), dict(ids=ids[:5], where=one)):
            with pytest.raises(RuntimeError, match="exactly one of"):
                idx.make_filter(**kw)
        with pytest.raises(RuntimeError, match="unknown attribute column"):
            idx.make_filter(any_of=[one, [("b", "in", [1])]])
        with pytest.raises(RuntimeError, match="unknown where op"):
            idx.make_filter(any_of=[[("a", "=~", 1)]])
        with pytest.raises(RuntimeError, match="9 clauses"):
            idx.make_filter(where=one * 9)
        with pytest.raises(RuntimeError, match="9 clauses"):
            idx.make_filter(where=[("a", "in", [1])] * 9)
        with pytest.raises(RuntimeError, match="9 clauses"):
            idx.make_filter(any_of=[one, one * 9])
        with pytest.raises(RuntimeError, match="9 terms"):
            idx.make_filter(any_of=[one] * 9)
        with pytest.raises(RuntimeError, match="33 clauses in total"):
            idx.make_filter(any_of=[one * 8] * 4 + [one])
        with pytest.raises(RuntimeError, match="at least one term"):
            idx.make_filter(any_of=[])
        with pytest.raises(RuntimeError, match="at least one clause"):
            idx.make_filter(any_of=[one, []])
        for bad in (3, {1, 2}, frozenset([1]), {1: 2}, "12", None):
            with pytest.raises(RuntimeError, match="must be a sequence"):
                idx.make_filter(where=[("a", "in", bad)])
        assert idx.make_filter(where=[("a", "in", (1, 2))]).info()["rows_allowed"] == 1200  # a tuple, a range, an array are sequences
        assert idx.make_filter(where=[("a", "in", range(3))]).info()["rows_allowed"] == 1800
        assert idx.make_filter(where=[("a", "in", np.array([4]))]).info()["rows_allowed"] == 600
        for bad in (5, None):
            with pytest.raises(RuntimeError, match="any_of is a list of where lists" if bad is not None else "exactly one of"):
                idx.make_filter(any_of=bad)
        with pytest.raises(RuntimeError, match="a term is a list of where clauses"):
            idx.make_filter(any_of=[one, 5])
        with pytest.raises(RuntimeError, match="operands must be integers"):
            idx.make_filter(where=[("a", "not_in", [1, 2.5])])
        with pytest.raises(RuntimeError, match="%d values" % ((1 << 20) + 1)):
            idx.make_filter(where=[("a", "in", [0] * ((1 << 20) + 1))])
        with pytest.raises(RuntimeError, match="exclude applies to ids"):
            idx.make_filter(exclude=True, any_of=[one])
        assert idx.make_filter(any_of=[one * 8] * 4).info()["rows_allowed"] == 600  # 32 clauses are fine
        assert idx.make_filter(where=[("a", "in", [1 << 70])]).info()["rows_allowed"] == 0  # no int64 equals 2^70
        assert idx.make_filter(where=[("a", "not_in", [])]).info()["rows_allowed"] == 3000
        assert idx.make_filter(any_of=[[("a", "in", [0, 4])], [("a", "==", 4)], [("a", "<", 0)]]).info()["rows_allowed"] == 1200
        grp = _build(mod, x, ids, 8, workers=2)
        with pytest.raises(RuntimeError, match="filtered search is not supported with num_workers > 0"):
            grp.make_filter(any_of=[one])
