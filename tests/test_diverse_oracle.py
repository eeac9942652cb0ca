"""The yardstick of diversified search checked on the CPU (tests/diverse_yardstick.py; the definition: include/quake_hip.h,
"diversified search"): expected() against an independent brute-force form, the consequences the interface documents (lambda = 1
is the prefix, fetch_k == k a permutation), a hand-computed 2-D case, the tie, NaN and infinity rules, and padding."""
import numpy as np
import pytest

import diverse_yardstick as DY
import oracle as O
import range_yardstick as RY


def same(a, b):
    for name, x, y in zip(DY.NAMES, a, b):
        if name == "dist":
            x, y = np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)
        np.testing.assert_array_equal(x, y, err_msg=name)


def toy(n, d, metric, seed, dup=0):
    """n candidates of one query from the oracle's arithmetic: ids, distances in (key, id) order, pairwise values"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, d)).astype(np.float32)
    for t in range(dup):
        V[n - 1 - t] = V[t]
    q = rng.standard_normal((1, d)).astype(np.float32)
    ids = (rng.permutation(10 * n)[:n]).astype(np.int64)
    oi, od = O.batched_serial_scan(q, V, ids, np.array([0, n], np.int64), np.zeros((1, 1), np.int64), n, metric)
    row_of = {int(t): i for i, t in enumerate(ids.tolist())}
    rows = np.array([row_of[int(t)] for t in oi[0]], np.int64)
    return oi[0], od[0], DY.pairwise(V[rows], metric)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,d,dup", [(1, 4, 0), (2, 3, 0), (17, 8, 0), (40, 33, 5), (64, 2, 8)])
def test_expected_equals_brute_force(metric, n, d, dup):
    ids, dist, P = toy(n, d, metric, 100 * n + d, dup)
    nan = np.isnan(P)
    assert ((P == P.T) | (nan & nan.T)).all()
    for lam in (0.0, 0.3, 0.5, 0.9, 1.0):
        for k in sorted({1, 2, min(5, n), n, n + 3}):
            same(DY.expected(ids, dist, P, k, lam, metric), DY.brute_force(ids, dist, P, k, lam, metric))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_lambda_one_is_the_prefix_and_full_fetch_a_permutation(metric):
    ids, dist, P = toy(30, 16, metric, 7, dup=3)
    for k in (1, 7, 30):
        gi, gd, gr = DY.expected(ids, dist, P, k, 1.0, metric)
        np.testing.assert_array_equal(gi, ids[:k])
        np.testing.assert_array_equal(gd.view(np.uint32), dist[:k].view(np.uint32))
        np.testing.assert_array_equal(gr, np.arange(k))
    for lam in (0.0, 0.5):
        gi, gd, gr = DY.expected(ids, dist, P, 30, lam, metric)
        assert sorted(gr.tolist()) == list(range(30)) and gr[0] == 0
        np.testing.assert_array_equal(gi, ids[gr])
        np.testing.assert_array_equal(gd.view(np.uint32), dist[gr].view(np.uint32))
    assert (DY.expected(ids, dist, P, 30, 0.0, metric)[2] != np.arange(30)).any(), "lambda = 0 must reorder this case"


def test_hand_computed_case():
    """Query at the origin, L2 (sqrt domain), lambda = 0.5, every product and difference below exact in float32:
      a = (1, 0) r = 1, b = (1.25, 0) r = 1.25, c = (0, 2) r = 2, d = (-3, 0) r = 3 -- ranks 0, 1, 2, 3.
    Step 1, S = {a}: N = |x - a| = 0.25 (b), sqrt(5) (c), 4 (d); cost = r / 2 - N / 2 = 0.5 (b), 1 - 1.118 = -0.118 (c),
      1.5 - 2 = -0.5 (d) -> d.
    Step 2, S = {a, d}: N = 0.25 (b), min(sqrt 5, sqrt 13) = sqrt 5 (c) -> costs 0.5 (b), -0.118 (c) -> c.  Then b."""
    V = np.array([[1, 0], [1.25, 0], [0, 2], [-3, 0]], np.float32)
    ids = np.array([40, 30, 20, 10], np.int64)
    dist = np.array([1, 1.25, 2, 3], np.float32)
    P = DY.pairwise(V, "l2")
    assert P[1, 0] == np.float32(0.25) and P[3, 0] == np.float32(4) and P[2, 0] == np.sqrt(np.float32(5))
    gi, gd, gr = DY.expected(ids, dist, P, 4, 0.5, "l2")
    assert gr.tolist() == [0, 3, 2, 1] and gi.tolist() == [40, 10, 20, 30] and gd.tolist() == [1, 3, 2, 1.25]
    assert DY.expected(ids, dist, P, 2, 0.5, "l2")[2].tolist() == [0, 3]
    same(DY.expected(ids, dist, P, 4, 0.5, "l2"), DY.brute_force(ids, dist, P, 4, 0.5, "l2"))
    # inner product, lambda = 0.5: relevance r = <q, x> with q = (1, 1): a = (2, 2) r = 4, b = (2, 1.5) r = 3.5, c = (-1, 3) r = 2
    # step 1, S = {a}: N = <x, a> = 7 (b), 4 (c); cost = r / 2 - N / 2 = -1.75 (b), -1 (c) -> the largest: c
    V = np.array([[2, 2], [2, 1.5], [-1, 3]], np.float32)
    P = DY.pairwise(V, "ip")
    assert P[1, 0] == 7 and P[2, 0] == 4
    gi, gd, gr = DY.expected(np.array([5, 6, 7], np.int64), np.array([4, 3.5, 2], np.float32), P, 3, 0.5, "ip")
    assert gr.tolist() == [0, 2, 1] and gi.tolist() == [5, 7, 6]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_identical_vectors_tie_to_the_smaller_rank(metric):
    """two identical vectors with different ids: equal distance, equal pairwise rows, equal costs at every step -- the one with
    the smaller rank (the smaller id) goes first"""
    V = np.array([[0.5, 0.5], [3, 1], [3, 1], [-2, 4]], np.float32)
    q = np.array([[0.4, 0.6]], np.float32)
    ids = np.array([9, 8, 3, 5], np.int64)
    oi, od = O.batched_serial_scan(q, V, ids, np.array([0, 4], np.int64), np.zeros((1, 1), np.int64), 4, metric)
    rank = {int(t): i for i, t in enumerate(oi[0].tolist())}
    assert rank[3] + 1 == rank[8] and od[0, rank[3]] == od[0, rank[8]]
    row_of = {9: 0, 8: 1, 3: 2, 5: 3}
    P = DY.pairwise(V[[row_of[int(t)] for t in oi[0]]], metric)
    for lam in (0.0, 0.3, 1.0):
        gi, _, gr = DY.expected(oi[0], od[0], P, 4, lam, metric)
        pos = {int(t): j for j, t in enumerate(gi.tolist())}
        assert pos[3] < pos[8], (lam, gi)
        same(DY.expected(oi[0], od[0], P, 4, lam, metric), DY.brute_force(oi[0], od[0], P, 4, lam, metric))
    # equal costs without equal vectors: lambda = 0 and equal pairwise values
    P = np.array([[0, 2, 2], [2, 0, 1], [2, 1, 0]], np.float32)
    assert DY.expected(np.array([1, 2, 3]), np.array([1, 5, 9], np.float32), P, 3, 0.0, metric)[2].tolist() == [0, 1, 2]


def test_nan_and_infinity_rules():
    ids = np.array([1, 2, 3, 4], np.int64)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # "ignored": candidate 1's value against the first pick is NaN, so its term is dropped: cost = 0.5 * 2 = 1, against
    # 0.5 * 3 - 0.5 * 1 = 1 (rank 2: a tie, the smaller rank wins) and 0.5 * 4 - 0.5 * 8 = -2 (rank 3)
    P = np.array([[0, nan, 1, 8], [nan, 0, 6, 2], [1, 6, 0, 1], [8, 2, 1, 0]], np.float32)
    r = np.array([1, 2, 3, 4], np.float32)
    assert DY.expected(ids, r, P, 4, 0.5, "l2")[2].tolist() == [0, 3, 1, 2]
    # ... then S = {0, 3}: N_1 = min(ignored, 2) = 2 -> 1 - 1 = 0; N_2 = min(1, 1) = 1 -> 1.5 - 0.5 = 1
    same(DY.expected(ids, r, P, 4, 0.5, "l2"), DY.brute_force(ids, r, P, 4, 0.5, "l2"))
    # without rank 3 the first step is the tie 1 == 1: rank 1
    assert DY.expected(ids[:3], r[:3], P[:3, :3], 3, 0.5, "l2")[2].tolist() == [0, 1, 2]
    # "loses": an infinite pairwise value against an infinite distance gives inf - inf = NaN, which loses to every number
    P = np.array([[0, inf, 1], [inf, 0, 1], [1, 1, 0]], np.float32)
    r = np.array([1, inf, 7], np.float32)
    gi, gd, gr = DY.expected(ids[:3], r, P, 3, 0.5, "l2")
    assert gr.tolist() == [0, 2, 1] and np.isinf(gd[2])
    same((gi, gd, gr), DY.brute_force(ids[:3], r, P, 3, 0.5, "l2"))
    # 0 * inf: lambda = 1 makes mu * N NaN for an infinite N: that cost loses too, and when every cost is NaN the smaller rank wins
    P = np.array([[0, inf, inf], [inf, 0, 1], [inf, 1, 0]], np.float32)
    r = np.array([1, 2, 3], np.float32)
    assert DY.expected(ids[:3], r, P, 3, 1.0, "l2")[2].tolist() == [0, 1, 2]
    P = np.array([[0, inf, 2], [inf, 0, 1], [2, 1, 0]], np.float32)
    assert DY.expected(ids[:3], r, P, 2, 1.0, "l2")[2].tolist() == [0, 2]
    same(DY.expected(ids[:3], r, P, 3, 1.0, "l2"), DY.brute_force(ids[:3], r, P, 3, 1.0, "l2"))
    # inner product: -inf relevance with a -inf similarity is NaN as well
    P = np.array([[0, -inf, 1], [-inf, 0, 1], [1, 1, 0]], np.float32)
    r = np.array([5, -inf, -9], np.float32)
    assert DY.expected(ids[:3], r, P, 3, 0.5, "ip")[2].tolist() == [0, 2, 1]
    # -0 and +0 are one cost
    assert not DY.better(np.float32(-0.0), np.float32(0.0), "l2") and not DY.better(np.float32(0.0), np.float32(-0.0), "l2")
    assert not DY.better(nan, nan, "ip") and DY.better(np.float32(-1e30), nan, "ip") and not DY.better(nan, inf, "l2")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_fewer_candidates_than_k(metric):
    ids, dist, P = toy(3, 5, metric, 11)
    gi, gd, gr = DY.expected(ids, dist, P, 6, 0.5, metric)
    assert (gi[3:] == -1).all() and (gr[3:] == -1).all() and sorted(gr[:3].tolist()) == [0, 1, 2]
    assert (gd[3:] == (np.float32(-np.inf) if metric == "ip" else np.float32(np.inf))).all()
    gi, gd, gr = DY.expected(ids[:0], dist[:0], P[:0, :0], 2, 0.5, metric)
    assert gi.tolist() == [-1, -1] and gr.tolist() == [-1, -1] and np.isinf(gd).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_case_builder(metric):
    """case() over a small clustered corpus: every row is what expected() gives for that query alone, the filter and the pids
    form restrict the candidates, lambda = 1 is the oracle's own search"""
    c = RY.corpus(12, 8, 600, metric, 5)
    q = RY.queries(c, 5, 6)
    k, C = 4, 20
    gi, gd, gr = DY.case(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, C, 1.0, metric)
    oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, C, metric, batched_scan=True, num_threads=8)
    np.testing.assert_array_equal(gi, oi[:, :k])
    np.testing.assert_array_equal(gd.view(np.uint32), od[:, :k].view(np.uint32))
    one = DY.case(q[2:3], c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, C, 0.3, metric)
    full = DY.case(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, C, 0.3, metric)
    same([a[2:3] for a in full], one)
    S = c["ids"][::3]
    fi = DY.case(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, C, 0.3, metric, S=S, mode="allow")[0]
    assert np.isin(fi[fi >= 0], S).all()
    pids = np.array([[2, -1, 5]] * 5, np.int64)
    pi = DY.case(q, None, c["vecs"], c["ids"], c["offsets"], None, k, C, 0.3, metric, pids=pids)[0]
    lists = np.repeat(np.arange(8), np.diff(c["offsets"]))
    assert np.isin([lists[np.nonzero(c["ids"] == t)[0][0]] for t in pi[pi >= 0]], [2, 5]).all()
    if metric == "l2":
        sq = DY.case(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, C, 1.0, metric, squared=True)
        np.testing.assert_array_equal(sq[0], gi)
        np.testing.assert_array_equal(np.sqrt(sq[1]).view(np.uint32), gd.view(np.uint32))
