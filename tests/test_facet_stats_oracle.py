"""Facet statistics on the CPU: tests/facet_stats_yardstick.py against hand-written answers, its identities on a random corpus, its
agreement with tests/facet_yardstick.py, the edge lowering of the mirrors (quake_amd/where.py: lower_edges), and the C ABI of
qk_facet_stats_search / qk_facet_stats_scan as far as it can be checked without a GPU."""
import os
import re

import numpy as np
import pytest

import facet_stats_yardstick as FSY
import facet_yardstick as FCY
import range_yardstick as RY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def _check(got, count, missing, vmin, vmax, sums, hist, total):
    np.testing.assert_array_equal(got[0], np.array(count, np.int64))
    np.testing.assert_array_equal(got[1], np.array(missing, np.int64))
    np.testing.assert_array_equal(got[2], np.array(vmin, np.int64))
    np.testing.assert_array_equal(got[3], np.array(vmax, np.int64))
    assert got[4] == sums
    np.testing.assert_array_equal(got[5], np.array(hist, np.int64))
    np.testing.assert_array_equal(got[6], np.array(total, np.int64))


def test_a_value_equal_to_an_edge_lands_in_the_bucket_to_its_right():
    col = {1: 9, 2: 10, 3: 11, 4: 50, 5: 49, 6: -7}
    # edges 10, 50: bucket 0 = v < 10, bucket 1 = 10 <= v < 50, bucket 2 = v >= 50
    _check(FSY.expected([[1, 2, 3, 4, 5, 6]], col, [10, 50]), [6], [0], [-7], [50], [122], [[2, 3, 1]], [6])
    _check(FSY.expected([[2], [4], [5]], col, [10, 50]), [1, 1, 1], [0, 0, 0], [10, 50, 49], [10, 50, 49], [10, 50, 49],
           [[0, 1, 0], [0, 0, 1], [0, 1, 0]], [1, 1, 1])


def test_edges_at_the_ends_of_int64():
    col = {1: I64MIN, 2: I64MIN + 1, 3: 0, 4: I64MAX - 1, 5: I64MAX}
    hits = [[1, 2, 3, 4, 5]]
    s = -2   # the five values add up to -2
    _check(FSY.expected(hits, col, [I64MIN]), [5], [0], [I64MIN], [I64MAX], [s], [[0, 5]], [5])         # nothing lies below INT64_MIN
    _check(FSY.expected(hits, col, [I64MAX]), [5], [0], [I64MIN], [I64MAX], [s], [[4, 1]], [5])         # INT64_MAX itself is right of it
    _check(FSY.expected(hits, col, [I64MIN, I64MAX]), [5], [0], [I64MIN], [I64MAX], [s], [[0, 4, 1]], [5])
    _check(FSY.expected(hits, col, [I64MIN + 1, 0, 1]), [5], [0], [I64MIN], [I64MAX], [s], [[1, 1, 1, 2]], [5])


def test_zero_hits_and_no_edges():
    _check(FSY.expected([[], []], {1: 3}, []), [0, 0], [0, 0], [I64MAX, I64MAX], [I64MIN, I64MIN], [0, 0], [[0], [0]], [0, 0])
    _check(FSY.expected([[]], {1: 3}, [5]), [0], [0], [I64MAX], [I64MIN], [0], [[0, 0]], [0])
    _check(FSY.expected([[1, 1, 2]], {1: 3, 2: 4}, []), [3], [0], [3], [4], [10], [[3]], [3])       # stored twice: counted twice


def test_a_column_with_no_stored_id():
    _check(FSY.expected([[1, 2, 3]], {100: 5}, [0, 9]), [0], [3], [I64MAX], [I64MIN], [0], [[0, 0, 0]], [3])
    _check(FSY.expected([[1, 2, 3], [2]], {2: -4}, [0]), [1, 1], [2, 0], [-4, -4], [-4, -4], [-4, -4], [[1, 0], [1, 0]], [3, 1])


def test_a_sum_beyond_64_bits():
    col = {1: I64MAX, 2: I64MAX, 3: I64MAX, 4: I64MIN}
    got = FSY.expected([[1, 2, 3], [4, 4, 4], [1, 4]], col, [])
    assert got[4] == [3 * I64MAX, 3 * I64MIN, -1]
    # 3 * (2^63 - 1) = 2^64 + (2^63 - 3): hi = 1, lo = 2^63 - 3 as unsigned = the int64 2^63 - 3
    assert FSY.split128(3 * I64MAX) == (1, (1 << 63) - 3)
    # 3 * -2^63 = -2^64 - 2^63: hi = -2, lo = 2^63 as unsigned = the int64 INT64_MIN
    assert FSY.split128(3 * I64MIN) == (-2, I64MIN)
    assert FSY.split128(-1) == (-1, -1) and FSY.split128(0) == (0, 0) and FSY.split128(I64MAX) == (0, I64MAX)
    assert FSY.split128((1 << 64) - 1) == (0, -1)
    out = FSY.expected_cols([[1, 2, 3], [4, 4, 4], [1, 4]], [col], [[]])
    np.testing.assert_array_equal(out[5], [[1, -2, -1]])
    np.testing.assert_array_equal(out[4], [[(1 << 63) - 3, I64MIN, -1]])
    rng = np.random.default_rng(5)
    for _ in range(200):
        x = int(rng.integers(I64MIN, I64MAX, endpoint=True)) * int(rng.integers(0, 1 << 30)) + int(rng.integers(-5, 6))
        hi, lo = FSY.split128(x)
        assert I64MIN <= hi <= I64MAX and I64MIN <= lo <= I64MAX and FSY.join128(hi, lo) == x


def _random_corpus():
    c = RY.corpus(16, 9, 1500, "l2", seed=71)
    q = RY.queries(c, 11, seed=72)
    rng = np.random.default_rng(73)
    ids = c["ids"]
    small = {int(i): int(v) for i, v in zip(ids, rng.integers(-20, 180, size=ids.shape[0])) if rng.random() < 0.9}
    wide = {int(i): int(v) for i, v in zip(ids, rng.integers(I64MIN, I64MAX, size=ids.shape[0], endpoint=True))}
    hits = FCY.hits_search(q, c["cent"], c["vecs"], ids, c["offsets"], 4, 6.0, "l2")
    assert sum(len(h) for h in hits) > 500
    return hits, small, wide, rng


def test_identities_on_a_random_corpus():
    hits, small, wide, rng = _random_corpus()
    for col in (small, wide):
        lo, hi = min(col.values()), max(col.values())
        edges = sorted({int(x) for x in rng.integers(lo, hi, size=40, endpoint=True)})
        count, missing, vmin, vmax, sums, hist, total = FSY.expected(hits, col, edges)
        np.testing.assert_array_equal(hist.sum(1), count)
        np.testing.assert_array_equal(count + missing, total)
        np.testing.assert_array_equal(total, [len(h) for h in hits])
        assert (vmin[count > 0] <= vmax[count > 0]).all() and (missing > 0).any() == (col is small)
        for q in range(len(hits)):
            if count[q]:
                assert int(count[q]) * int(vmin[q]) <= sums[q] <= int(count[q]) * int(vmax[q])   # (Python ints: no wrap)


def test_the_two_yardsticks_agree():
    hits, small, _, _ = _random_corpus()
    vals = sorted(set(small.values()))
    assert 2 <= len(vals) <= 255
    hist = FSY.expected(hits, small, vals)[5]
    fv, fc, fd, _, _ = FCY.expected(hits, small, 256)
    for q in range(len(hits)):
        want = dict(zip(fv[q, :fd[q]].tolist(), fc[q, :fd[q]].tolist()))
        assert hist[q, 0] == 0                                           # no value lies below the smallest one
        assert hist[q, 1:].tolist() == [want.get(v, 0) for v in vals]  # bucket i + 1 = [vals[i], vals[i + 1]) holds vals[i] alone


def test_lower_edges():
    from quake_amd.where import QK_MAX_FACET_EDGES, lower_edges
    assert QK_MAX_FACET_EDGES == 255
    assert lower_edges(["a", "b"], None) == ([], [0, 0])
    assert lower_edges(["a", "b"], [1, 5, 9]) == ([1, 5, 9, 1, 5, 9], [3, 3])                    # one sequence: every column
    assert lower_edges(["a", "b"], (1, 5)) == ([1, 5, 1, 5], [2, 2])
    assert lower_edges(["a", "b"], np.array([1, 5])) == ([1, 5, 1, 5], [2, 2])
    assert lower_edges(["a"], []) == ([], [0])
    assert lower_edges(["a", "b", "c"], {"c": [7], "a": [I64MIN, I64MAX]}) == ([I64MIN, I64MAX, 7], [2, 0, 1])
    assert lower_edges(["a", "b"], [[3, 4], None]) == ([3, 4], [2, 0])                           # one entry per column
    assert lower_edges(["a", "b"], [[], [0]]) == ([0], [0, 1])
    assert lower_edges(["a", "a"], [[1], [2, 3]]) == ([1, 2, 3], [1, 2])                         # the same column twice
    flat, n = lower_edges(["a"], range(255))
    assert n == [255] and flat == list(range(255))
    assert all(type(x) is int for x in lower_edges(["a"], np.arange(3, dtype=np.int32))[0])
    # a tensor or an array stands for its tolist() in every position: alone, as a dict value, as a per-column entry, two-dimensional
    import torch
    t, a = torch.tensor([1, 5]), np.array([3, 4], np.int16)
    assert lower_edges(["a", "b"], t) == ([1, 5, 1, 5], [2, 2])
    assert lower_edges(["a", "b"], {"b": t}) == ([1, 5], [0, 2])
    assert lower_edges(["a", "b"], [t, a]) == ([1, 5, 3, 4], [2, 2]) and lower_edges(["a", "b"], [None, a]) == ([3, 4], [0, 2])
    assert lower_edges(["a", "b"], torch.tensor([[1, 5], [3, 4]])) == ([1, 5, 3, 4], [2, 2])
    assert all(type(x) is int for x in lower_edges(["a", "b"], [t, a])[0])
    for bad, match in (([torch.tensor([2, 2]), None], "strictly ascending"), ([None, torch.tensor([1.5])], "integers"),
                       (torch.tensor(3), "sequence")):
        with pytest.raises(RuntimeError, match=match):
            lower_edges(["a", "b"], bad)
    for bad, match in (([1, 1], "strictly ascending"), ([2, 1], "strictly ascending"), (list(range(256)), "at most 255"),
                       ([1.5], "integers"), ([True], "integers"), (["1"], "integers"), ([1 << 63], "int64"), ([-(1 << 63) - 1], "int64"),
                       (5, "sequence"), ("12", "sequence"), ({"zz": [1]}, "not one of"), ([[1], [2], [3]], "per-column"),
                       ({"a": [3, 3]}, "strictly ascending"), ({"a": 7}, "sequence")):
        with pytest.raises(RuntimeError, match=match):
            lower_edges(["a", "b"], bad)


def test_abi():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    assert re.search(r"^#define\s+QK_MAX_FACET_EDGES\s+255\b", txt, re.M)
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    for name in ("qk_facet_stats_search", "qk_facet_stats_scan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"QK_API\s+int\s+%s\s*\(" % name, txt)
    # search has the parent and nprobe where scan has pids and P; the rest is the same list
    a, b = _lib.SIGNATURES["qk_facet_stats_search"][1], _lib.SIGNATURES["qk_facet_stats_scan"][1]
    assert len(a) == 23 and len(b) == 23 and a[7:] == b[7:]
    assert _lib.header_constant("QK_MAX_FACET_EDGES") == 255
    import quake_amd
    from quake_amd.capi import Context
    assert hasattr(Context, "facet_stats_search") and hasattr(Context, "facet_stats_scan")
    assert hasattr(quake_amd.QuakeIndex, "facet_stats") and hasattr(quake_amd, "FacetStatsResult")


def test_result_conveniences_without_a_gpu():
    import torch

    import quake_amd
    r = quake_amd.FacetStatsResult()
    words = [FSY.split128(x) for x in (3 * I64MAX, 3 * I64MIN, -1, 0)]
    r.sum_hi = torch.tensor([[w[0] for w in words]], dtype=torch.int64)
    r.sum_lo = torch.tensor([[w[1] for w in words]], dtype=torch.int64)
    r.count = torch.tensor([[3, 3, 2, 0]], dtype=torch.int64)
    assert r.sums() == [[3 * I64MAX, 3 * I64MIN, -1, 0]]
    m = r.means()
    assert m.dtype == np.float64 and m.shape == (1, 4)
    assert m[0, 0] == float(I64MAX) and m[0, 1] == float(I64MIN) and m[0, 2] == -0.5 and np.isnan(m[0, 3])
