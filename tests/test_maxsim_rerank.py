"""Multi-vector rerank (qk_maxsim_rerank; Context.maxsim_rerank; QuakeIndex.multi_vector_rerank and multi_vector_search(fetch_k=)):
per logical query the k best of a shortlist of documents by the sum over the query's vectors of the best pair among ALL rows of
the document.

The reference is tests/maxsim_yardstick.py: scan over every list with radius +-inf and k = the number of documents, its entries
restricted to the candidates in order (a total order restricted to a subset is the subset's order).  Groups, score bits, matched
and n_groups must be equal; rows must equal a numpy count.  Every test asserts on its inputs that its situations occur."""
import numpy as np
import pytest
import torch

import maxsim_yardstick as MY
from test_maxsim_search import _attr, _corpus, _np

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
L = 5
MISSING = {"ip": 0.0, "l2": 9.5}
NODOC, NANDOC = 999, 55


def _column(ids):
    """ids under 3000 have a value (half of them): one document of 2600 rows, documents of 1, 15, 16 and 17 rows under the extreme
    values, a one-row document that is a row of NaNs, 60 small ones"""
    i = ids[ids < 3000]
    v = np.where(i < 2600, 7, np.where(i == 2600, I64MIN, np.where(i < 2616, I64MAX, np.where(i < 2632, -1, np.where(
        i < 2649, 5, np.where(i == 2649, NANDOC, 100 + i % 60))))))
    return i, v.astype(np.int64)


def _rows_of(e, keep=None):
    """value -> live rows with that value (numpy)"""
    ai, av = e["col"]
    ids = e["c"]["ids"] if keep is None else e["c"]["ids"][keep]
    uv, n = np.unique(av[np.isin(ai, ids)], return_counts=True)
    return dict(zip(uv.tolist(), n.tolist()))


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora(ctx):
    from quake_amd.capi import Filter, Store
    cache = {}

    def get(metric, d=32):
        if (metric, d) not in cache:
            c = _corpus(metric, 501 if metric == "l2" else 502)
            if d != 32:   # the same lists over wider rows (a padded last block for d = 40)
                x = np.random.default_rng(503).standard_normal((6000, d)).astype(np.float32)
                c.update(vecs=x / np.linalg.norm(x, axis=1, keepdims=True), d=d)
            c["vecs"][np.flatnonzero(c["ids"] == 2649)] = np.nan
            s = Store(ctx, d)
            s.build_csr(c["offsets"], c["ids"], c["vecs"])
            col = _column(c["ids"])
            S = np.concatenate([np.arange(2632, 2640), [2600]]).astype(np.int64)   # some rows of document 5, all of INT64_MIN's
            e = dict(c=c, s=s, col=col, attr=_attr(s, *col), S=S, flt=Filter(s, S, "deny"), memo={})
            n = _rows_of(e)
            big = np.flatnonzero(np.isin(c["ids"], col[0][col[1] == 7]))
            assert (n[7], n[I64MIN], n[I64MAX], n[-1], n[5], n[NANDOC]) == (2600, 1, 15, 16, 17, 1) and NODOC not in n
            assert np.unique(np.searchsorted(c["offsets"], big, "right")).shape[0] > 3 and col[0].shape[0] == 3000 and len(n) <= 1024
            cache[(metric, d)] = e
        return cache[(metric, d)]

    yield get
    for e in cache.values():
        e["attr"].close()
        e["flt"].close()
        e["s"].close()


def _queries(e, T):
    c = e["c"]
    rng = np.random.default_rng(510 + T)
    q = (c["vecs"][rng.integers(0, 2000, size=L * T)] + 0.05 * rng.standard_normal((L * T, c["d"]))).astype(np.float32)
    q = np.nan_to_num(q)
    if c["metric"] == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q.reshape(L, T, c["d"]))


def _candidates(e, C):
    """[L, C] and n_cand: every document, one without rows, one named twice, in a shuffled order; n_cand[1] = 0"""
    vals = np.unique(e["col"][1])
    pool = np.concatenate([vals, [NODOC, 7, 5]]).astype(np.int64)
    rng = np.random.default_rng(520 + C)
    cand = np.stack([np.resize(rng.permutation(pool), C) for _ in range(L)])
    n_cand = np.array([C, 0, min(C, 40), C, max(C // 2, 1)], np.int32)
    if C >= pool.shape[0]:
        assert all(x in cand[0] for x in (I64MIN, I64MAX, -1, NODOC)) and (cand[0] == 7).sum() >= 2
    return cand, n_cand


def _want(e, q3, cand, n_cand, k, n_tokens=None, filtered=False, squared=False):
    """the yardstick over all lists, restricted to the candidates, and the row counts"""
    c, m = e["c"], e["c"]["metric"]
    key = (q3.tobytes(), None if n_tokens is None else tuple(n_tokens), filtered, squared)
    if key not in e["memo"]:
        ndoc = np.unique(e["col"][1]).shape[0]
        e["memo"][key] = MY.scan(q3, c["vecs"], c["ids"], c["offsets"], np.arange(12, dtype=np.int64), ndoc, m, *e["col"], radius=None,
                                 n_tokens=n_tokens, missing=MISSING[m], S=e["S"] if filtered else None, mode="deny", squared=squared)
    g, s, mt, n, _ = e["memo"][key]
    rows = _rows_of(e, ~np.isin(c["ids"], e["S"]) if filtered else None)
    inf = np.float32(np.inf if m == "l2" else -np.inf)
    out = np.zeros((L, k), np.int64), np.full((L, k), inf, np.float32), np.zeros((L, k), np.int32), np.zeros(L, np.int64)
    out_r = np.zeros((L, k), np.int32)
    for l in range(L):
        named = np.isin(g[l, :n[l]], cand[l, :n_cand[l]])
        out[3][l] = named.sum()
        j = np.flatnonzero(named)[:k]
        out[0][l, :j.shape[0]], out[1][l, :j.shape[0]], out[2][l, :j.shape[0]] = g[l, j], s[l, j], mt[l, j]
        out_r[l, :j.shape[0]] = [rows[v] for v in g[l, j].tolist()]
    return out, out_r


def _check(got, want, tag):
    (g, s, mt, n), rows = want
    MY.assert_equal([_np(o) for o in (got[0], got[1], got[2], got[4])] + [np.zeros(0)], (g, s, mt, n, np.zeros(0)), tag)
    assert np.array_equal(_np(got[3]), rows), tag + " rows"


@pytest.mark.parametrize("T", [1, 3, 17, 64])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_against_yardstick(ctx, corpora, metric, T):
    e = corpora(metric)
    q3 = _queries(e, T)
    if T >= 3:
        q3[2, 1] = np.nan   # a query vector without a pair that is a number: its term is `missing`
    nt = [T, 0, max(T // 2, 1), 1, T]
    for C, k, ntok, flt in ((1024, 1024, nt, False), (1024, 10, None, True), (1, 3, nt, False)):
        cand, n_cand = _candidates(e, C)
        want = _want(e, q3, cand, n_cand, k, ntok, flt)
        assert NANDOC not in want[0][0] and (want[0][3][1] == 0) and (flt or ntok[1] == 0)
        if T >= 3 and ntok is None:
            assert want[0][3][2] > 0 and (want[0][2][2, :min(k, want[0][3][2])] == T - 1).all()
        if flt:
            left = _rows_of(e, ~np.isin(e["c"]["ids"], e["S"]))
            assert I64MIN not in left and left[5] == 9 and I64MIN not in want[0][0]
        got = ctx.maxsim_rerank(e["s"], q3, metric, e["attr"], cand, k, MISSING[metric], ntok, n_cand, e["flt"] if flt else None)
        _check(got, want, "%s T=%d C=%d" % (metric, T, C))
    # device memory, n_cand NULL: every named value counts; row l equals the call of logical query l alone
    cand, _ = _candidates(e, 70)
    full = np.full(L, 70, np.int32)
    dev = ctx.maxsim_rerank(e["s"], torch.from_numpy(q3).cuda(), metric, e["attr"], torch.from_numpy(cand).cuda(), 10, MISSING[metric])
    _check(dev, _want(e, q3, cand, full, 10), "device")
    one = ctx.maxsim_rerank(e["s"], q3[3:4], metric, e["attr"], cand[3:4], 10, MISSING[metric])
    assert all(np.array_equal(_np(a)[3], _np(b)[0]) for a, b in zip(dev[:5], one[:5]))


def test_squared_l2_mutation_and_wide_rows(ctx, corpora):
    from quake_amd.capi import Store
    e = corpora("l2")
    q3 = _queries(e, 3)
    cand, n_cand = _candidates(e, 128)
    ctx.set_squared_l2(True)
    try:
        got = ctx.maxsim_rerank(e["s"], q3, "l2", e["attr"], cand, 20, 9.5, None, n_cand)
        _check(got, _want(e, q3, cand, n_cand, 20, squared=True), "squared")
    finally:
        ctx.set_squared_l2(False)
    # d = 40: a padded last block
    e40 = corpora("ip", 40)
    q40 = _queries(e40, 17)
    _check(ctx.maxsim_rerank(e40["s"], q40, "ip", e40["attr"], cand, 20, 0.0, None, n_cand), _want(e40, q40, cand, n_cand, 20), "d=40")
    # add + remove: the next call sees the store as it is (document 5 loses rows, document 7 gains one in the empty list)
    c = e["c"]
    x_new = q3[0, :1].copy()
    e["s"].add_entries(1, np.array([2999999], np.int64), x_new)
    e["attr"].set(np.array([2999999], np.int64), np.array([7], np.int64))
    e["s"].remove_ids(np.arange(2632, 2636, dtype=np.int64))
    keep = ~np.isin(c["ids"], np.arange(2632, 2636))
    c2 = dict(c, vecs=np.concatenate([c["vecs"][keep], x_new]), ids=np.concatenate([c["ids"][keep], [2999999]]))
    sizes = np.diff(c["offsets"]) - np.bincount(np.searchsorted(c["offsets"], np.flatnonzero(~keep), "right") - 1, minlength=12)
    order = np.argsort(np.concatenate([np.repeat(np.arange(12), sizes), [1]]), kind="stable")
    sizes[1] += 1
    c2.update(vecs=c2["vecs"][order], ids=c2["ids"][order], offsets=np.concatenate([[0], np.cumsum(sizes)]))
    e2 = dict(c=c2, col=(np.append(e["col"][0], 2999999), np.append(e["col"][1], 7)), S=e["S"], memo={})
    want = _want(e2, q3, cand, n_cand, 20)
    assert (_rows_of(e2)[7], _rows_of(e2)[5]) == (2601, 13)
    _check(ctx.maxsim_rerank(e["s"], q3, "l2", e["attr"], cand, 20, 9.5, None, n_cand), want, "after add + remove")
    # wide rows: T = 17 takes two column tiles, whose 608 columns exceed the 64 KiB of staged tokens -- the chunked walk
    rng = np.random.default_rng(530)
    d, n = 600, 300
    assert 32 * ((d + 15) // 16) * 64 > 64 << 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    cw = dict(vecs=x, ids=np.arange(n, dtype=np.int64), offsets=np.array([0, 120, 120, 300], np.int64), d=d, metric="ip")
    cw["offsets"] = np.concatenate([cw["offsets"], np.full(9, 300, np.int64)])   # (12 lists, as _want scans)
    s = Store(ctx, d)
    s.build_csr(cw["offsets"], cw["ids"], x)
    col = (cw["ids"], np.where(cw["ids"] < 100, 1, 2 + cw["ids"] % 11).astype(np.int64))
    a = _attr(s, *col)
    ew = dict(c=cw, col=col, S=np.zeros(0, np.int64), memo={})
    qw = (x[rng.integers(0, n, L * 17)] + 0.05 * rng.standard_normal((L * 17, d)).astype(np.float32)).reshape(L, 17, d)
    cands = np.tile(np.arange(0, 16, dtype=np.int64), (L, 1))
    nc = np.full(L, 16, np.int32)
    try:
        got = ctx.maxsim_rerank(s, qw, "ip", a, cands, 16, 0.0)
        _check(got, _want(ew, qw, cands, nc, 16), "wide rows")
        # float64 cross-check on unit-norm rows: the plain sum of maxima, within T * 1e-4 (the per-pair parity bar)
        g, sc = _np(got[0]), _np(got[1])
        sim = np.einsum("ltd,nd->ltn", qw.astype(np.float64), x.astype(np.float64))
        for l in range(L):
            ref = np.array([sim[l][:, col[1] == v].max(axis=1).sum() for v in g[l, :12]])
            assert np.abs(sc[l, :12] - ref).max() <= 17 * 1e-4
    finally:
        a.close()
        s.close()


@pytest.mark.parametrize("mirror", ["python", "compiled"])
def test_index_surface(mirror, tmp_path):
    """in both mirrors: multi_vector_rerank equals the C call, and multi_vector_search(fetch_k=) equals stage one followed by the
    rerank of its groups"""
    import quake_amd as quake
    rng = np.random.default_rng(540)
    n, d, T = 3000, 32, 3
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    bp = quake.IndexBuildParams()
    bp.nlist, bp.metric = 8, "ip"
    py = quake.QuakeIndex()
    py.build(torch.from_numpy(x), torch.arange(n), bp)
    idx, mod = py, quake
    if mirror == "compiled":
        from quake_amd.build_ext import build_bindings
        build_bindings()
        import quake_amd.bindings as mod
        py.save(str(tmp_path / "index"))
        idx = mod.QuakeIndex()
        idx.load(str(tmp_path / "index"))
    for m in {id(py): py, id(idx): idx}.values():
        m.set_attribute("doc", torch.arange(n), torch.arange(n) // 7)
    q = torch.from_numpy(x[rng.integers(0, n, 4 * T)].reshape(4, T, d).copy())
    sp, sp30 = mod.SearchParams(), mod.SearchParams()
    sp.k, sp.nprobe, sp30.k, sp30.nprobe = 5, 2, 30, 2
    one = idx.multi_vector_search(q, "doc", sp30)
    assert int(one.n_groups.min()) >= 30
    two = idx.multi_vector_rerank(q, "doc", one.groups, 5)
    raw = py._ctx.maxsim_rerank(py._store, q, "ip", py._attributes()["doc"], one.groups.numpy(), 5, 0.0)
    both = idx.multi_vector_search(q, "doc", sp, fetch_k=30)
    for a, b, c in zip((two.groups, two.scores, two.matched, two.rows, two.n_groups), raw[:5],
                       (both.groups, both.scores, both.matched, both.rows, both.n_groups)):
        assert np.array_equal(_np(a), _np(b)) and np.array_equal(_np(a), _np(c))
    assert (two.rows[:, 0] == 7).all() and two.hits is None and both.hits is not None
    dev = idx.multi_vector_rerank(q.cuda(), "doc", one.groups.cuda(), 5, n_candidates=[30, 0, 7, 30])
    assert dev.groups.is_cuda and _np(dev.n_groups).tolist() == [30, 0, 7, 30] and np.array_equal(_np(dev.groups)[0], _np(two.groups)[0])
    with pytest.raises(RuntimeError, match="fetch_k"):
        idx.multi_vector_search(q, "doc", sp, fetch_k=3)
