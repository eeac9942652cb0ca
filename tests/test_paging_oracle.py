"""The yardstick of paged search (tests/paging_yardstick.py) pinned on the CPU, against the oracle's own search and against the
rule written from the per-pair values: pages chained by (key, id) cursors are consecutive slices of the full ordering, the end is
padding and the exhausted cursor, and ties on the key are broken by the id.  No GPU."""
import numpy as np
import pytest

import filter_yardstick as FY
import nonfinite_yardstick as NF
import oracle as O
import paging_yardstick as PY
import range_yardstick as RY

NPROBE = 4


@pytest.fixture(scope="module")
def corpus():
    c = RY.corpus(16, 12, 1500, "l2", seed=41)
    return c, RY.queries(c, 6, seed=42)


def _chain(order, k, max_pages=100000):
    """every query's pages of size k from the start cursor until one comes back padded"""
    Q = len(order)
    cur = [PY.START] * Q
    pages = []
    for _ in range(max_pages):
        oi, od, cur = PY.page(order, cur, k)
        pages.append((oi, od, list(cur)))
        if all(c == PY.EXHAUSTED for c in cur):
            return pages
    raise AssertionError("the chain did not end")


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("k", [1, 7, 448])
def test_chained_pages_are_slices_of_the_full_search(k, metric):
    c = RY.corpus(16, 12, 1500, metric, seed=43)
    q = RY.queries(c, 5, seed=44)
    order = PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], NPROBE, metric)
    pages = _chain(order, k)
    K = len(pages) * k  # (the chain ends with the first page on which every query is short: K covers every candidate)
    fi, fd = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], NPROBE, K, metric, batched_scan=True, num_threads=8)
    for p, (oi, od, cur) in enumerate(pages):
        np.testing.assert_array_equal(oi, fi[:, p * k:(p + 1) * k])
        np.testing.assert_array_equal(od.view(np.uint32), fd[:, p * k:(p + 1) * k].view(np.uint32))
    # every candidate exactly once, in order
    for i in range(len(order)):
        got = np.concatenate([pg[0][i] for pg in pages])
        got = got[got >= 0]
        np.testing.assert_array_equal(got, order.ids[i])


def test_the_end_is_padding_and_the_exhausted_cursor(corpus):
    c, q = corpus
    order = PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], NPROBE, "l2")
    k = 7
    for i in range(len(order)):
        n = order.ids[i].shape[0]
        # the last page that holds anything: full only if n is a multiple of k
        pos = (n // k) * k
        oi, od, nxt = PY.page_at(order, i, pos, k)
        assert (oi[:n - pos] == order.ids[i][pos:]).all() and (oi[n - pos:] == -1).all() and np.isinf(od[n - pos:]).all()
        assert nxt == PY.EXHAUSTED
        # a full page ends at its k-th row's (key, id), and the page behind that cursor starts right behind it
        if n >= k:
            oi, od, nxt = PY.page_at(order, i, 0, k)
            assert nxt == (int(order.keys[i][k - 1]), int(order.ids[i][k - 1])) and PY.position(order, i, nxt) == k
        # behind the exhausted cursor: nothing
        assert PY.position(order, i, PY.EXHAUSTED) == n
        oi, od, nxt = PY.page_at(order, i, n, k)
        assert (oi == -1).all() and np.isinf(od).all() and nxt == PY.EXHAUSTED
        assert PY.position(order, i, PY.START) == 0


def test_ties_on_the_key_are_broken_by_the_id():
    c = RY.corpus(16, 12, 1500, "l2", seed=45)
    vecs, ids, offsets = c["vecs"].copy(), c["ids"].copy(), c["offsets"]
    sizes = np.diff(offsets)
    big = np.argsort(-sizes)[:2]
    # one vector five times, in two lists, under ids that are not in stored order
    rows = [offsets[big[0]] + 3, offsets[big[0]] + 40, offsets[big[1]] + 1, offsets[big[1]] + 17, offsets[big[1]] + 33]
    v = vecs[rows[0]].copy()
    for r, new in zip(rows, (900001, 0, 900003, 5, 900000)):
        vecs[r] = v
        ids[r] = new
    assert np.unique(ids).shape[0] == ids.shape[0]
    q = v[None, :].copy()
    pids = np.array([[big[0], big[1]]], np.int64)
    order = PY.ordering(q, None, vecs, ids, offsets, 0, "l2", pids=pids)
    assert (order.keys[0][:5] == 0).all() and order.keys[0][5] > 0
    np.testing.assert_array_equal(order.ids[0][:5], [0, 5, 900000, 900001, 900003])
    # a page of 2 cuts the run of equal keys: the cursor's id is what keeps the other three for the next page
    oi, od, nxt = PY.page_at(order, 0, 0, 2)
    assert nxt == (0, 5) and list(oi) == [0, 5]
    oi, od, nxt = PY.page_at(order, 0, PY.position(order, 0, nxt), 2)
    assert list(oi) == [900000, 900001] and nxt == (0, 900001)
    # the start cursor (0, -1) lies below the row with key 0 and id 0
    assert PY.position(order, 0, PY.START) == 0 and PY.position(order, 0, (0, 0)) == 1


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_keys_are_the_order_of_the_values(metric):
    """key_of against the rule of tests/nonfinite_yardstick.py: sorting by (key, id) is sorting by (value, id) with NaN dropped,
    descending for IP, -0 == +0"""
    v = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3e-40, -3e-40, 2.0 ** 100, 1.5], np.float32)
    if metric == "l2":
        v = np.abs(v)
    ids = np.arange(v.shape[0], dtype=np.int64)[::-1].copy()
    key = PY.key_of(v, metric)
    assert (key[np.isnan(v)] == 0xFFFFFFFF).all() and (key[~np.isnan(v)] != 0xFFFFFFFF).all()
    ok = key != 0xFFFFFFFF
    mine = ids[ok][np.lexsort((ids[ok], key[ok]))]
    want, _ = NF.topk_of_values(v, ids, v.shape[0], metric)
    np.testing.assert_array_equal(mine, want)


def test_a_filter_is_a_smaller_corpus(corpus):
    c, q = corpus
    rng = np.random.default_rng(46)
    S = FY.draw_set(c["ids"], 0.1, rng)
    order = PY.ordering(q, c["cent"], c["vecs"], c["ids"], c["offsets"], NPROBE, "l2", S=S, mode="allow")
    K = max(o.shape[0] for o in order.ids) + 1
    fi, fd = FY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], NPROBE, K, "l2", S, "allow")
    for i in range(len(order)):
        n = order.ids[i].shape[0]
        np.testing.assert_array_equal(order.ids[i], fi[i, :n])
        assert np.isin(order.ids[i], S).all() and (fi[i, n:] == -1).all()
