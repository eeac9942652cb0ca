"""Paged search (qk_search_after / qk_scan_after; capi.Context.search_after / scan_after; QuakeIndex.search_after and
SearchResult.cursor in both mirrors): the page of k results behind every query's (key, id) cursor, decided in the epilogue of the
filtered tile form (k_scan_after, k_scan_wide_after), the next cursor written behind the merge (k_next_cursor).

Expected values come from tests/paging_yardstick.py -- the definition, one query at a time, pinned on the CPU by
tests/test_paging_oracle.py -- and every comparison is exact: ids, the uint32 view of the distances, the cursors.  The corpus is
the one of tests/test_adaptive_search.py.  No test reads a clock."""
import numpy as np
import pytest
import torch

import filter_yardstick as Y
import nonfinite_yardstick as NF
import paging_yardstick as PY
import range_yardstick as RY
from test_adaptive_search import NLIST, _corpus, _Filters, _queries, _stores
from test_filtered_search import _build, _eq, _np, _only_allowed

pytestmark = pytest.mark.gpu

QK_MAX_K = 448


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


def _order(c, q, nprobe, spec=None, pids=None):
    S, mode = spec if spec is not None else (None, "allow")
    return PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, c["metric"], S=S, mode=mode, pids=pids)


def _same_page(got, want, tag):
    """(ids, dist, (next keys, next ids)) of a call against the yardstick's (ids, dist, next cursors)"""
    gi, gd, (nk, ni) = got[:3]
    oi, od, nxt = want
    _eq(gi, gd, oi, od, tag)
    assert PY.cursor_list(_np(nk), _np(ni)) == nxt, tag


def _chain(call, order, k, tag, max_pages=5000):
    """pages of size k from the start until every query is exhausted, each compared with its yardstick slice.  Returns the cursors
    (as lists of (key, id)) in front of every page, the exhausted one included, and the pages' ids"""
    Q = len(order)
    cur, after = [PY.START] * Q, None
    cursors, pages = [], []
    for p in range(max_pages):
        cursors.append(cur)
        got = call(after, k)
        want = PY.page(order, cur, k)
        _same_page(got, want, (tag, "page", p))
        pages.append(_np(got[0]))
        cur, after = want[2], got[2]
        if all(c == PY.EXHAUSTED for c in cur):
            cursors.append(cur)
            return cursors, pages
    raise AssertionError("the chain did not end")


# ---- 1. the start page is the search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [16, 64, 128, 768])
def test_start_page_is_the_search(ctx, corpora, d, metric):
    c, s, parent = corpora(d, metric)
    q = _queries(c, 40, seed=710 + d)
    Q = q.shape[0]
    start = PY.cursor_arrays([PY.START] * Q)
    for nprobe in (1, 4, 130):
        for k in (1, 10, 100, 448):
            oi, od = ctx.search(parent, s, q, nprobe, k, metric)
            gi, gd, _ = ctx.search_after(parent, s, q, nprobe, k, metric)
            assert ctx.last_scan_kernel() == "k_scan (after)"
            _eq(gi, gd, _np(oi), _np(od), (d, metric, nprobe, k, "NULL cursors"))
            gi, gd, (nk, ni) = ctx.search_after(parent, s, q, nprobe, k, metric, after=start)
            _eq(gi, gd, _np(oi), _np(od), (d, metric, nprobe, k, "start cursor"))
            # the next cursor names the k-th result, or says that there is none
            full = _np(oi)[:, k - 1] >= 0
            np.testing.assert_array_equal(_np(ni)[full], _np(oi)[full, k - 1])
            assert (_np(ni)[~full] == PY.EXHAUSTED[1]).all() and (_np(nk).view(np.uint32)[~full] == 0xFFFFFFFF).all()
    # device-resident queries and cursors: the same bits
    oi, od = ctx.search(parent, s, q, 4, 10, metric)
    xq = torch.from_numpy(q).cuda()
    gi, gd, (nk, ni) = ctx.search_after(parent, s, xq, 4, 10, metric, after=(torch.from_numpy(start[0]).cuda(), torch.from_numpy(start[1]).cuda()))
    ctx.synchronize()  # (the context's own stream: torch does not wait for it)
    assert gi.is_cuda and nk.is_cuda and ni.is_cuda
    _eq(gi, gd, _np(oi), _np(od), (d, metric, "device"))


# ---- 2. chaining to exhaustion, and resuming every cursor at another page size ---------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_chain_to_exhaustion_and_resume(ctx, corpora, metric):
    c, s, parent = corpora(64, metric)
    q = _queries(c, 6, seed=720)
    Q, nprobe = q.shape[0], 4
    order = _order(c, q, nprobe)
    cursors, pages = _chain(lambda after, k: ctx.search_after(parent, s, q, nprobe, k, metric, after=after), order, 7, (metric, "k=7"))
    for i in range(Q):  # every candidate once, in order; the last page padded
        got = np.concatenate([p[i] for p in pages])
        np.testing.assert_array_equal(got[got >= 0], order.ids[i])
    assert (pages[-1] == -1).any()
    # one more page behind the exhausted cursors: padding only, and the cursor stays exhausted
    gi, gd, (nk, ni) = ctx.search_after(parent, s, q, nprobe, 7, metric, after=PY.cursor_arrays(cursors[-1]))
    assert (_np(gi) == -1).all() and np.isinf(_np(gd)).all()
    assert PY.cursor_list(_np(nk), _np(ni)) == [PY.EXHAUSTED] * Q
    # every stored cursor resumed with k = 13 -- as ONE batch: the queries repeated once per stored cursor, each at its own depth
    P = len(cursors)
    xq = np.ascontiguousarray(np.tile(q, (P, 1)))
    flat = [cur for page in cursors for cur in page]
    gi, gd, (nk, ni) = ctx.search_after(parent, s, xq, nprobe, 13, metric, after=PY.cursor_arrays(flat))
    gi, gd, got_next = _np(gi), _np(gd), PY.cursor_list(_np(nk), _np(ni))
    for p in range(P):
        for i in range(Q):
            oi, od, nxt = PY.page_at(order, i, PY.position(order, i, cursors[p][i]), 13)
            _eq(gi[p * Q + i], gd[p * Q + i], oi, od, (metric, "resume", p, i))
            assert got_next[p * Q + i] == nxt, (metric, "resume", p, i)


# ---- 3. ties on the key across a page boundary -------------------------------------------------------------------------------------------
def test_ties_across_the_page_boundary(ctx):
    from quake_amd.capi import Store
    c = _corpus(16, "l2", seed=730)
    vecs, ids, off = c["vecs"].copy(), c["ids"].copy(), c["offsets"]
    # one vector five times: lists 8 (257 rows) and 9 (5003 rows), tiles 0, 1, 2 of the one and 0, 2 of the other, ids out of order
    rows = [off[9] + 3, off[9] + 40, off[8] + 1, off[8] + 17, off[8] + 33]
    v = vecs[rows[0]].copy()
    for r, new in zip(rows, (900001, 0, 900003, 5, 900000)):
        vecs[r], ids[r] = v, new
    assert np.unique(ids).shape[0] == ids.shape[0]
    c = dict(c, vecs=vecs, ids=ids)
    s, parent = _stores(ctx, c)
    q = np.ascontiguousarray(np.stack([v, _queries(c, 1, seed=731)[0]]))
    pids = np.array([[9, 8], [8, 9]], np.int64)
    order = _order(c, q, 0, pids=pids)
    assert (order.keys[0][:5] == 0).all() and list(order.ids[0][:5]) == [0, 5, 900000, 900001, 900003]
    cur, after = [PY.START] * 2, None
    seen = []
    for p in range(4):  # a page of 2 cuts the run of five behind its 2nd copy, the next one behind its 4th
        got = ctx.scan_after(s, q, pids, 2, "l2", after=after)
        want = PY.page(order, cur, 2)
        _same_page(got, want, ("ties", p))
        seen.append(_np(got[0])[0])
        cur, after = want[2], got[2]
    assert list(np.concatenate(seen)[:5]) == [0, 5, 900000, 900001, 900003]  # (id 0 on the first page: the start cursor is (0, -1))
    # the same through the coarse step (query 0 is a row of list 9: its nearest list)
    order = _order(c, q, 130)
    got = ctx.search_after(parent, s, q, 130, 2, "l2", after=PY.cursor_arrays([(0, 5), PY.START]))
    _same_page(got, PY.page(order, [(0, 5), PY.START], 2), "ties, search")
    assert list(_np(got[0])[0]) == [900000, 900001]
    s.close()
    parent.close()


# ---- 4. mixed depths in one 16-query tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_mixed_depths_in_one_batch(ctx, corpora, metric):
    c, s, parent = corpora(128, metric)
    q = _queries(c, 40, seed=740)
    Q, nprobe, k = q.shape[0], 4, 10
    order = _order(c, q, nprobe)
    chain = [[PY.START] * Q]  # chain[p]: the cursors in front of page p
    after = None
    for p in range(5):
        got = ctx.search_after(parent, s, q, nprobe, k, metric, after=after)
        after = got[2]
        chain.append(PY.cursor_list(_np(after[0]), _np(after[1])))
    mixed = [chain[i % 5 + 1][i] for i in range(Q)]  # query i continues behind page i mod 5
    got = ctx.search_after(parent, s, q, nprobe, k, metric, after=PY.cursor_arrays(mixed))
    _same_page(got, PY.page(order, mixed, k), (metric, "mixed"))
    for i in range(Q):  # row i is the single-query call
        one = ctx.search_after(parent, s, q[i:i + 1], nprobe, k, metric, after=PY.cursor_arrays(mixed[i:i + 1]))
        _eq(one[0], one[1], _np(got[0])[i:i + 1], _np(got[1])[i:i + 1], (metric, "single", i))
        assert PY.cursor_list(_np(one[2][0]), _np(one[2][1])) == PY.cursor_list(_np(got[2][0])[i:i + 1], _np(got[2][1])[i:i + 1])


# ---- 5. the near rows before the cursor set no bound --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_rows_before_the_cursor_set_no_bound(ctx, corpora, metric):
    c, s, parent = corpora(128, metric)
    pool = _queries(c, 48, seed=750)
    nprobe, k = 8, 10
    order = _order(c, pool, nprobe)
    probed = RY.probed(pool, c["cent"], c["offsets"], nprobe, metric)
    keep, cursors = [], []
    for i in range(pool.shape[0]):
        # the rows a seeded bound would be learnt from: the first 128 of the query's nearest non-empty list
        near = [int(p) for p in probed[i] if c["offsets"][p + 1] > c["offsets"][p]][0]
        head = c["ids"][c["offsets"][near]:c["offsets"][near + 1]][:128]
        pos = np.nonzero(np.isin(order.ids[i], head))[0]
        depth = max(300, int(pos.max()) + 1)  # past the first 300 rows AND past every one of those
        if depth + k <= order.ids[i].shape[0]:
            keep.append(i)
            cursors.append((int(order.keys[i][depth - 1]), int(order.ids[i][depth - 1])))
    assert len(keep) >= 16, "too few queries with a full page that deep"
    q = np.ascontiguousarray(pool[keep])
    sub = PY.Order([order.ids[i] for i in keep], [order.dist[i] for i in keep], [order.keys[i] for i in keep], metric)
    got = ctx.search_after(parent, s, q, nprobe, k, metric, after=PY.cursor_arrays(cursors))
    assert (_np(got[0]) >= 0).all()  # (a bound from the rows before the cursor leaves padding here)
    _same_page(got, PY.page(sub, cursors, k), (metric, "deep"))


# ---- 6. under a filter, past 448 results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filtered_pages(ctx, corpora, metric):
    c, s, parent = corpora(64, metric)
    fam = _Filters(s, c, seed=760)
    q = _queries(c, 6, seed=761)
    nprobe = 130
    try:
        for name, k in (("allow0.1", 200), ("allow0.01", 50), ("deny0.3", 448), ("allow0", 10), ("where", 200)):
            j = _Filters.NAMES.index(name)
            spec = fam.spec[j]
            if not isinstance(spec, tuple):  # the predicate's yardstick is a keep mask over the ids
                spec = (c["ids"][np.asarray(spec, bool)], "allow")
            order = _order(c, q, nprobe, spec=spec)
            f = fam.h[j]
            cursors, pages = _chain(lambda after, kk: ctx.search_after(parent, s, q, nprobe, kk, metric, after=after, filter=f), order, k,
                                    (metric, name))
            assert ctx.last_scan_kernel() == "k_scan (after)"
            got = np.concatenate(pages, axis=1)
            _only_allowed(got, c["ids"], spec[0], spec[1], (metric, name))
            for i in range(q.shape[0]):
                np.testing.assert_array_equal(got[i][got[i] >= 0], order.ids[i])
            if name in ("allow0.1", "deny0.3", "where"):
                assert max(o.shape[0] for o in order.ids) > QK_MAX_K  # deeper than a filtered search can reach
            if name == "allow0":
                assert (got == -1).all()
            # the slices are those of the filtered yardstick asked for everything
            K = got.shape[1]
            fi, fd = Y.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, K, metric, spec[0], spec[1])
            np.testing.assert_array_equal(got, fi)
    finally:
        fam.close()


# ---- 7. wide rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_wide_rows(ctx, metric):
    from quake_amd.capi import Store
    c = RY.corpus(3072, 12, 1500, metric, seed=770)
    q = RY.queries(c, 20, seed=771)
    s = Store(ctx, 3072)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = Store(ctx, 3072)
    parent.build_csr(np.array([0, 12], np.int64), np.arange(12, dtype=np.int64), c["cent"])
    order = PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, metric)
    for k in (10, 448):
        oi, od = ctx.search(parent, s, q, 4, k, metric)
        cur, after = [PY.START] * q.shape[0], None
        for p in range(2):
            got = ctx.search_after(parent, s, q, 4, k, metric, after=after)
            assert ctx.last_scan_kernel() == "k_scan_wide (after)"
            want = PY.page(order, cur, k)
            _same_page(got, want, (metric, k, "wide page", p))
            if p == 0:
                _eq(got[0], got[1], _np(oi), _np(od), (metric, k, "wide start"))
            cur, after = want[2], got[2]
    s.close()
    parent.close()


# ---- 8. non-finite values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_nonfinite_values(ctx, cls, metric):
    from quake_amd.capi import Store
    c = NF.corpus(cls, metric, 6000, 16, 32, seed=780)
    q, special = NF.queries(c, 16, seed=781)
    s = Store(ctx, 32)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = Store(ctx, 32)
    parent.build_csr(np.array([0, 16], np.int64), np.arange(16, dtype=np.int64), c["centroids"])
    nprobe, k = 4, 448
    order = PY.ordering(q, c["centroids"], c["vecs"], c["ids"], c["offsets"], nprobe, metric)
    Q = q.shape[0]

    def same(got, want, tag):  # (which sign a returned zero carries is not part of the contract: NF.assert_same_answer)
        NF.assert_same_answer(_np(got[0]), _np(got[1]), want[0], want[1])
        assert PY.cursor_list(_np(got[2][0]), _np(got[2][1])) == want[2], tag

    cur, after, pages = [PY.START] * Q, None, []
    for p in range(64):
        got = ctx.search_after(parent, s, q, nprobe, k, metric, after=after)
        want = PY.page(order, cur, k)
        same(got, want, (cls, metric, p))
        NF.assert_no_nan_pair(c, q, special, _np(got[0]))
        pages.append(_np(got[0]))
        cur, after = want[2], got[2]
        if all(x == PY.EXHAUSTED for x in cur):
            break
    else:
        raise AssertionError("the chain did not end")
    allp = np.concatenate(pages, axis=1)
    for i in range(Q):  # every candidate once and in order: +-inf rows included, NaN pairs never
        np.testing.assert_array_equal(allp[i][allp[i] >= 0], order.ids[i])
    if cls == "underflow":
        # -0 and +0 share a key: a page boundary inside such a run is decided by the id.  The run of query 9 (the signed-zero pair)
        zero = [i for i in range(Q) if ((order.dist[i] == 0).sum() >= 2)]
        assert 9 in zero or metric == "l2", zero
        for i in zero:
            z = np.nonzero(order.dist[i] == 0)[0]
            assert (np.diff(z) == 1).all() and (np.diff(order.keys[i][z]) == 0).all() and (np.diff(order.ids[i][z]) > 0).all()
            first = int(z[0])
            lo = max(0, first - 3)
            c0 = PY.START if lo == 0 else (int(order.keys[i][lo - 1]), int(order.ids[i][lo - 1]))
            kk = first + 1 - lo  # the page ends ON the first row of the run
            got = ctx.search_after(parent, s, q[i:i + 1], nprobe, kk, metric, after=PY.cursor_arrays([c0]))
            sub = PY.Order([order.ids[i]], [order.dist[i]], [order.keys[i]], metric)
            want = PY.page(sub, [c0], kk)
            same(got, want, (cls, metric, "zero run", i))
            assert want[2][0] == (int(order.keys[i][first]), int(order.ids[i][first]))
            got = ctx.search_after(parent, s, q[i:i + 1], nprobe, 4, metric, after=got[2])
            want = PY.page(sub, want[2], 4)
            same(got, want, (cls, metric, "behind the first zero", i))
            assert _np(got[0])[0, 0] == order.ids[i][first + 1]
    s.close()
    parent.close()


# ---- 9. mutation between two pages ----------------------------------------------------------------------------------------------------------
def test_mutation_between_pages(ctx):
    c = _corpus(64, "l2", seed=790)
    s, parent = _stores(ctx, c)
    q = _queries(c, 8, seed=791)
    Q, nprobe, k = q.shape[0], 4, 10
    order = _order(c, q, nprobe)
    got1 = ctx.search_after(parent, s, q, nprobe, k, "l2")
    want1 = PY.page(order, [PY.START] * Q, k)
    _same_page(got1, want1, "page 1")
    # for query 0: a new row nearer than the cursor (the query itself), a new row farther (a copy of its 16th result under a larger
    # id: the same key, right behind it), and its 13th result removed
    off, ids, vecs = c["offsets"], c["ids"], c["vecs"]
    list_of = np.repeat(np.arange(NLIST), np.diff(off))
    probed = RY.probed(q, c["cent"], off, nprobe, "l2")
    near_list = [int(p) for p in probed[0] if off[p + 1] > off[p]][0]
    r15 = int(np.nonzero(ids == order.ids[0][15])[0][0])
    gone = int(order.ids[0][12])
    new_ids = np.array([10 ** 9 + 1, 10 ** 9 + 2], np.int64)
    s.add_entries(near_list, new_ids[:1], q[:1])
    s.add_entries(int(list_of[r15]), new_ids[1:], vecs[r15:r15 + 1])
    assert s.remove_ids(np.array([gone], np.int64)) == 1
    # the same on the CSR: rows appended to their lists, one row deleted
    add_list = np.array([near_list, int(list_of[r15])])
    add_vecs = np.stack([q[0], vecs[r15]])
    keep = ids != gone
    lists2 = np.concatenate([list_of[keep], add_list])
    o2 = np.argsort(lists2, kind="stable")
    c2 = dict(c, vecs=np.ascontiguousarray(np.concatenate([vecs[keep], add_vecs])[o2]), ids=np.concatenate([ids[keep], new_ids])[o2])
    c2["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(lists2, minlength=NLIST))]).astype(np.int64)
    order2 = _order(c2, q, nprobe)
    got2 = ctx.search_after(parent, s, q, nprobe, k, "l2", after=got1[2])
    _same_page(got2, PY.page(order2, want1[2], k), "page 2 over the changed store")
    p1, p2 = _np(got1[0]), _np(got2[0])
    for i in range(Q):
        assert not np.isin(p2[i][p2[i] >= 0], p1[i]).any(), i  # nothing twice
    assert new_ids[0] not in p2[0] and gone not in p2[0] and new_ids[1] in p2[0]
    assert list(p2[0][:7]) == list(order.ids[0][10:12]) + list(order.ids[0][13:16]) + [int(new_ids[1]), int(order.ids[0][16])]
    s.close()
    parent.close()


# ---- 10. both mirrors, and a flat index ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


@pytest.mark.parametrize("nlist", [1, 20])
def test_both_mirrors(qb, nlist):
    import quake_amd as quake
    g = torch.Generator().manual_seed(801)
    n, d, page = 6000, 32, 5
    x = torch.randn(n, d, generator=g)
    ids = torch.randperm(n, generator=g) + 11
    q = torch.randn(33, d, generator=g)
    S = torch.from_numpy(Y.draw_set(ids.numpy(), 0.2, np.random.default_rng(802)))
    out = {}
    for name, mod in (("python", quake), ("compiled", qb)):
        idx = _build(mod, x, ids, nlist)
        for filtered in (False, True):
            for dev in (False, True):
                sp = mod.SearchParams()
                sp.nprobe, sp.k = 4, 3 * page
                if filtered:
                    sp.filter = idx.make_filter(S)
                xq = q.cuda() if dev else q
                full = idx.search(xq, sp)
                assert full.cursor is None
                sp.k = page
                cur, got_i, got_d = None, [], []
                for p in range(3):
                    r = idx.search_after(xq, sp, cur)
                    assert r.ids.is_cuda == dev and r.cursor.keys.is_cuda == dev and len(r.cursor) == q.shape[0]
                    assert r.cursor.keys.dtype == torch.int32 and r.cursor.ids.dtype == torch.int64
                    got_i.append(r.ids.cpu())
                    got_d.append(r.distances.cpu())
                    cur = r.cursor
                    # prefix by prefix
                    np.testing.assert_array_equal(torch.cat(got_i, 1).numpy(), full.ids.cpu().numpy()[:, :(p + 1) * page])
                    np.testing.assert_array_equal(torch.cat(got_d, 1).numpy().view(np.uint32),
                                                  full.distances.cpu().numpy()[:, :(p + 1) * page].view(np.uint32))
                    assert (r.cursor.ids.cpu() == r.ids.cpu()[:, -1]).all()
                out[(name, filtered, dev)] = (torch.cat(got_i, 1).numpy(), torch.cat(got_d, 1).numpy(), cur.keys.cpu().numpy(), cur.ids.cpu().numpy())
        # a cursor built by hand from what a page returned continues the same way
        sp = mod.SearchParams()
        sp.nprobe, sp.k = 4, page
        r1 = idx.search_after(q, sp)
        r2 = idx.search_after(q, sp, mod.SearchCursor(r1.cursor.keys.clone(), r1.cursor.ids.clone()))
        np.testing.assert_array_equal(r2.ids.numpy(), out[(name, False, False)][0][:, page:2 * page])
    for key in [k for k in out if k[0] == "python"]:
        a, b = out[key], out[("compiled",) + key[1:]]
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------
def _plain(mod):
    sp = mod.SearchParams()
    sp.nprobe, sp.k = 4, 10
    return sp


def test_refusals(ctx, corpora, qb):
    import quake_amd as quake
    from quake_amd._lib import QuakeHipError
    from quake_amd.capi import Filter, Store
    c, s, parent = corpora(16, "l2")
    q = _queries(c, 5, seed=811)
    Q = q.shape[0]
    want = ctx.search(parent, s, q, 4, 10, "l2")

    def still_answers():
        gi, gd, _ = ctx.search_after(parent, s, q, 4, 10, "l2")
        _eq(gi, gd, _np(want[0]), _np(want[1]), "after a refusal")

    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.search_after(parent, s, q, 4, QK_MAX_K + 1, "l2")
    still_answers()
    with pytest.raises(QuakeHipError, match="QK_ERR_UNSUPPORTED.*QK_MAX_K"):
        ctx.scan_after(s, q, np.array([3, 4], np.int64), QK_MAX_K + 1, "l2")
    still_answers()
    keys, ids = PY.cursor_arrays([PY.START] * Q)
    for after in ((keys, None), (None, ids)):  # one cursor array without the other
        with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*after_key and after_id"):
            ctx.search_after(parent, s, q, 4, 10, "l2", after=after)
        still_answers()
    with pytest.raises(ValueError, match="one entry per query"):
        ctx.search_after(parent, s, q, 4, 10, "l2", after=(keys[:-1], ids[:-1]))
    other = Store(ctx, 16)
    other.build_csr(c["offsets"], c["ids"], c["vecs"])
    fo = Filter(other, c["ids"][:50], "allow")
    with pytest.raises(QuakeHipError, match="QK_ERR_INVALID.*another store"):
        ctx.search_after(parent, s, q, 4, 10, "l2", filter=fo)
    still_answers()
    fo.close()
    other.close()
    # the mirrors: what a page is not defined for is refused, not approximated
    g = torch.Generator().manual_seed(812)
    x = torch.randn(3000, 16, generator=g)
    xid = torch.arange(3000) + 5
    xq = torch.randn(7, 16, generator=g)
    for mod in (quake, qb):
        idx = _build(mod, x, xid, 16)
        sp = _plain(mod)
        ok = idx.search_after(xq, sp)
        fl = [idx.make_filter(xid[:100]), idx.make_filter(xid[100:300])]

        def refused(match, cursor=None, index=idx):
            with pytest.raises(RuntimeError, match=match):
                index.search_after(xq, sp, cursor)
            assert (idx.search_after(xq, _plain(mod)).ids == ok.ids).all()  # the index still answers

        sp.k = QK_MAX_K + 1
        refused("449")
        sp.k = 10
        sp.filters, sp.query_filter = fl, torch.zeros(7, dtype=torch.int32)
        refused("one filter per query")
        sp.filters, sp.query_filter = [], None
        sp.filter, sp.max_nprobe = fl[0], 8
        refused("max_nprobe")
        sp.filter, sp.max_nprobe = None, 0
        sp.recall_target = 0.9
        refused("recall_target")
        sp.recall_target = -1.0
        refused("for 7 queries", cursor=mod.SearchCursor(ok.cursor.keys[:-1].clone(), ok.cursor.ids[:-1].clone()))
        for half in (mod.SearchCursor(ok.cursor.keys.clone(), None), mod.SearchCursor(None, ok.cursor.ids.clone())):
            refused("keys and ids", cursor=half)  # one of the two cursor arrays missing
        refused("num_workers", index=_build(mod, x, xid, 16, workers=2))
        oth = _build(mod, x, xid, 16)
        sp.filter = oth.make_filter(xid[:100])
        refused("another index")
        sp.filter = None
        assert (idx.search_after(xq, sp, ok.cursor).ids[:, 0] != ok.ids[:, 0]).all()
