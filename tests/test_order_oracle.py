"""Ordered search on the CPU: tests/order_yardstick.py against hand-written answers and against independent statements of the same
thing on the corpus the GPU tests use -- facet statistics' counters and extremes, the oracle's top-k, the range hits -- and the
situations the GPU tests rely on, asserted on the inputs themselves."""
import numpy as np
import pytest

import facet_stats_yardstick as FSY
import facet_yardstick as FCY
import oracle as O
import order_yardstick as OY
import paging_yardstick as PY
import range_yardstick as RY

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def _order(ids, dist, metric="l2"):
    """one query whose candidates are given in (key, id) order"""
    d = np.array(dist, np.float32)
    return PY.Order([np.array(ids, np.int64)], [d], [PY.key_of(d * d if metric == "l2" else d, metric)], metric)


def test_by_hand():
    # five hits in (key, id) order; 30 has no value; 10 and 40 share the value 7: the nearer one (10) comes first in BOTH directions
    o = _order([10, 20, 30, 40, 50], [1.0, 2.0, 3.0, 4.0, 5.0])
    col = {10: 7, 20: -1, 40: 7, 50: I64MAX, 99: 0}
    ids, dist, values, count, missing, total = OY.expected(o, 10.0, col, 6)
    assert ids.tolist() == [[20, 10, 40, 50, -1, -1]] and values.tolist() == [[-1, 7, 7, I64MAX, 0, 0]]
    assert dist[0, :4].tolist() == [2.0, 1.0, 4.0, 5.0] and np.isposinf(dist[0, 4:]).all()
    assert (count.tolist(), missing.tolist(), total.tolist()) == ([4], [1], [5])
    ids, _, values, _, _, _ = OY.expected(o, 10.0, col, 6, descending=True)
    assert ids.tolist() == [[50, 10, 40, 20, -1, -1]] and values.tolist() == [[I64MAX, 7, 7, -1, 0, 0]]
    ids, dist, values, count, _, _ = OY.expected(o, 10.0, col, 6, descending=True, missing_last=True)
    assert ids.tolist() == [[50, 10, 40, 20, 30, -1]] and values.tolist() == [[I64MAX, 7, 7, -1, 0, 0]] and dist[0, 4] == 3.0
    assert (np.arange(6) < count[0]).tolist() == [True, True, True, True, False, False]        # entry j has a value iff j < count
    # the cut inside the tie: k = 2 ascending takes 20 and the nearer of the two 7s
    assert OY.expected(o, 10.0, col, 2)[0].tolist() == [[20, 10]]
    # the radius is inclusive and comes first: 4.0 keeps 10, 20, 30, 40
    ids, _, _, count, missing, total = OY.expected(o, 4.0, col, 3, missing_last=True)
    assert ids.tolist() == [[20, 10, 40]] and (count.tolist(), missing.tolist(), total.tolist()) == ([3], [1], [4])
    # no hit, and hits none of which has a value
    assert OY.expected(o, 0.5, col, 2)[0].tolist() == [[-1, -1]]
    ids, _, values, count, missing, _ = OY.expected(o, 10.0, {}, 2, missing_last=True)
    assert ids.tolist() == [[10, 20]] and values.tolist() == [[0, 0]] and (count.tolist(), missing.tolist()) == ([0], [5])
    assert OY.expected(o, 10.0, {}, 2)[0].tolist() == [[-1, -1]]
    # inner product: larger is nearer, padding -inf, the radius a lower bound
    o = _order([3, 1, 2], [0.9, 0.5, 0.1], "ip")
    ids, dist, _, _, _, total = OY.expected(o, 0.5, {1: 4, 2: 0, 3: 4}, 3)
    assert ids.tolist() == [[3, 1, -1]] and total.tolist() == [2] and np.isneginf(dist[0, 2])
    # every int64 orders as a signed number
    o = _order([1, 2, 3, 4], [1.0, 2.0, 3.0, 4.0])
    col = {1: -1, 2: I64MAX, 3: I64MIN, 4: 0}
    assert OY.expected(o, 9.0, col, 4)[0].tolist() == [[3, 1, 4, 2]] and OY.expected(o, 9.0, col, 4, True)[0].tolist() == [[2, 4, 1, 3]]


def _uniq_value(i):
    return int(np.uint64((int(i) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)).astype(np.int64))


@pytest.fixture(scope="module", params=["l2", "ip"])
def world(request):
    metric = request.param
    c = RY.corpus(32, 20, 6000, metric, seed=301 if metric == "l2" else 302)
    q = RY.queries(c, 40, seed=304)
    ids = c["ids"]
    rng = np.random.default_rng(303)
    pick = rng.random(ids.shape[0]) < 0.95
    few = {int(i): int(v) for i, v in zip(ids[pick], np.array([I64MIN, -1, 0, 5, I64MAX], np.int64)[rng.integers(0, 5, size=int(pick.sum()))])}
    cols = dict(few=few, uniq={int(i): _uniq_value(i) for i in ids}, const={int(i): 42 for i in ids},
                none={int(i): int(i) % 9 for i in range(50000, 50050)})
    order = PY.ordering(q, c["cent"], c["vecs"], ids, c["offsets"], 3, metric)
    mine = np.sort(order.dist[0])
    half = float(mine[mine.shape[0] // 2] if metric == "l2" else mine[-(mine.shape[0] // 2) - 1])
    inf = float("inf") if metric == "l2" else float("-inf")
    return dict(c=c, q=q, cols=cols, order=order, half=half, inf=inf, metric=metric)


def _hits(w, radius):
    c = w["c"]
    lims, hid, _ = RY.search(w["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], 3, radius, w["metric"])
    return FCY.split(lims, hid)


def test_counters_and_extremes_are_those_of_facet_statistics(world):
    w = world
    for radius in (w["half"], w["inf"]):
        hits = _hits(w, radius)
        for name in ("few", "uniq", "none"):
            count, missing, vmin, vmax, _, _, total = FSY.expected(hits, w["cols"][name], [])
            for desc in (False, True):
                got = OY.expected(w["order"], radius, w["cols"][name], 4, desc)
                np.testing.assert_array_equal(got[3], count)
                np.testing.assert_array_equal(got[4], missing)
                np.testing.assert_array_equal(got[5], total)
                some = count > 0
                np.testing.assert_array_equal(got[2][some, 0], (vmax if desc else vmin)[some])       # the first entry is the extreme
                assert (got[0][~some] == -1).all()
    assert (FSY.expected(_hits(w, w["inf"]), w["cols"]["few"], [])[1] > 0).any()


def test_a_constant_column_leaves_the_search_order(world):
    w, c = world, world["c"]
    k = 50
    oi, od = O.search(w["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, w["metric"], batched_scan=True, num_threads=8)
    for desc in (False, True):
        ids, dist, values, _, _, total = OY.expected(w["order"], w["inf"], w["cols"]["const"], k, desc)
        assert (total >= k).any()
        np.testing.assert_array_equal(ids, oi)
        np.testing.assert_array_equal(dist.view(np.uint32), od.view(np.uint32))
        assert ((values == 42) == (ids >= 0)).all()


def test_descending_is_the_reverse_on_distinct_values(world):
    w = world
    k = 6000
    for radius in (w["half"], w["inf"]):
        a = OY.expected(w["order"], radius, w["cols"]["uniq"], k)
        d = OY.expected(w["order"], radius, w["cols"]["uniq"], k, True)
        assert (a[3] <= k).all() and a[3].sum() > 0
        for qi in range(40):
            n = int(a[3][qi])
            for j in range(3):
                np.testing.assert_array_equal(a[j][qi, :n], d[j][qi, :n][::-1])


def test_missing_last_returns_every_hit(world):
    w = world
    hits = _hits(w, w["half"])
    for name in ("few", "none"):
        for desc in (False, True):
            ids, _, values, count, missing, total = OY.expected(w["order"], w["half"], w["cols"][name], 6000, desc, True)
            for qi in range(40):
                assert sorted(ids[qi, :total[qi]].tolist()) == sorted(hits[qi].tolist()) and (ids[qi, total[qi]:] == -1).all()
                tail = ids[qi, count[qi]:total[qi]]
                assert all(int(i) not in w["cols"][name] for i in tail) and (values[qi, count[qi]:] == 0).all()
            assert (missing > 0).any()


def test_the_situations_the_gpu_tests_rely_on(world):
    w, c = world, world["c"]
    # a cut where entries k and k + 1 share the value: few has hundreds of hits per value
    want = OY.expected(w["order"], w["inf"], w["cols"]["few"], 11)
    tied = (want[2][:, 9] == want[2][:, 10]) & (want[0][:, 10] >= 0)
    assert tied.any()
    qi = int(np.nonzero(tied)[0][0])
    at = {int(i): j for j, i in enumerate(w["order"].ids[qi])}
    ka, kb = (int(w["order"].keys[qi][at[int(want[0][qi, j])]]) for j in (9, 10))
    assert (ka, int(want[0][qi, 9])) < (kb, int(want[0][qi, 10]))                       # ... and (key, id) decides between them
    # a query with fewer than k hits that have a value, and one with none of them although it has hits
    half = OY.expected(w["order"], w["half"], w["cols"]["few"], 1024)
    assert ((half[3] > 0) & (half[3] < 1024)).any()
    none = OY.expected(w["order"], w["half"], w["cols"]["none"], 10)
    assert ((none[3] == 0) & (none[5] > 0)).any()
    # a cut where the two entries share value AND key: three rows with one vector and one value, the query at that vector
    metric = w["metric"]
    c2 = RY.corpus(32, 20, 6000, metric, seed=311)
    big = int(np.argmax(np.diff(c2["offsets"])))
    rows = c2["offsets"][big] + np.array([3, 40, 41])
    c2["vecs"][rows] = c2["vecs"][rows[0]]
    tid = np.sort(c2["ids"][rows])
    col = {int(i): 5 for i in c2["ids"]}
    for i in tid:
        col[int(i)] = 1
    q = np.ascontiguousarray(c2["vecs"][rows[:1]])
    o = PY.ordering(q, None, c2["vecs"], c2["ids"], c2["offsets"], 1, metric)
    where = [int(np.nonzero(o.ids[0] == i)[0][0]) for i in tid]
    assert len({int(o.keys[0][j]) for j in where}) == 1
    w3 = OY.expected(o, w["inf"], col, 3)
    assert w3[0][0].tolist() == tid.tolist() and (w3[2][0] == 1).all()
    assert OY.expected(o, w["inf"], col, 2)[0][0].tolist() == tid[:2].tolist()                 # the id decides
    # a row that is a hit twice is two equal entries (the multiset form of the yardstick)
    vecs2 = np.concatenate([c["vecs"], c["vecs"][:5]])
    ids2 = np.concatenate([c["ids"], c["ids"][:5]])
    offs2 = np.concatenate([c["offsets"], [c["offsets"][-1] + 5]])
    first = int(np.nonzero(np.diff(c["offsets"]) > 0)[0][0])
    pairs = RY.all_pairs(w["q"][:2], vecs2, ids2, offs2, np.array([first, 20], np.int64), metric)
    tw = OY.expected_pairs(w["q"][:2], vecs2, ids2, pairs, w["inf"], metric, w["cols"]["uniq"], 4)
    assert (tw[0][:, 0] == tw[0][:, 1]).all() and (tw[0][:, 2] == tw[0][:, 3]).all() and (tw[0][:, 1] != tw[0][:, 2]).all()
    assert (tw[5] == c["offsets"][first + 1] - c["offsets"][first] + 5).all()
