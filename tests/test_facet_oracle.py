"""Facet counts on the CPU: tests/facet_yardstick.py against hand-written answers, its invariant on the corpora of range search,
and the C ABI of qk_facet_search / qk_facet_scan as far as it can be checked without a GPU."""
import ctypes as C
import os
import re

import numpy as np

import facet_yardstick as FCY
import range_yardstick as RY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def _check(got, values, counts, distinct, missing, total):
    np.testing.assert_array_equal(got[0], np.array(values, np.int64))
    np.testing.assert_array_equal(got[1], np.array(counts, np.int64))
    np.testing.assert_array_equal(got[2], np.array(distinct, np.int64))
    np.testing.assert_array_equal(got[3], np.array(missing, np.int64))
    np.testing.assert_array_equal(got[4], np.array(total, np.int64))


def test_ties_on_count_are_decided_by_the_signed_value():
    col = {1: 2, 2: -3, 3: 2, 4: -3, 5: 9}
    _check(FCY.expected([[1, 2, 3, 4, 5]], col, 3), [[-3, 2, 9]], [[2, 2, 1]], [3], [0], [5])
    _check(FCY.expected([[1, 2, 3, 4, 5]], col, 1), [[-3]], [[2]], [3], [0], [5])


def test_extreme_values_order_as_signed_integers():
    col = {10: -1, 11: I64MIN, 12: I64MAX, 13: 0, 14: -1}
    # -1 twice, the others once: -1 first, then the singletons ascending -- INT64_MIN, 0, INT64_MAX
    _check(FCY.expected([[10, 11, 12, 13, 14]], col, 4), [[-1, I64MIN, 0, I64MAX]], [[2, 1, 1, 1]], [4], [0], [5])
    _check(FCY.expected([[11, 12, 13]], col, 4), [[I64MIN, 0, I64MAX, 0]], [[1, 1, 1, 0]], [3], [0], [3])


def test_ids_without_a_value_are_missing():
    col = {1: 7, 2: 7}
    _check(FCY.expected([[1, 2, 3, 4], [3]], col, 2), [[7, 0], [0, 0]], [[2, 0], [0, 0]], [1, 0], [2, 1], [4, 1])


def test_a_column_with_no_stored_id():
    _check(FCY.expected([[1, 2, 3]], {100: 5}, 2), [[0, 0]], [[0, 0]], [0], [3], [3])
    _check(FCY.expected([[1, 2, 3]], {}, 2), [[0, 0]], [[0, 0]], [0], [3], [3])


def test_n_values_below_equal_and_above_distinct():
    col = {1: 5, 2: 5, 3: 5, 4: 6, 5: 6, 6: 4}
    hits = [[1, 2, 3, 4, 5, 6]]
    _check(FCY.expected(hits, col, 2), [[5, 6]], [[3, 2]], [3], [0], [6])
    _check(FCY.expected(hits, col, 3), [[5, 6, 4]], [[3, 2, 1]], [3], [0], [6])
    _check(FCY.expected(hits, col, 5), [[5, 6, 4, 0, 0]], [[3, 2, 1, 0, 0]], [3], [0], [6])


def test_an_id_stored_twice_counts_twice():
    _check(FCY.expected([[1, 1, 2]], {1: 3, 2: 4}, 2), [[3, 4]], [[2, 1]], [2], [0], [3])


def test_zero_hits():
    _check(FCY.expected([[], []], {1: 3}, 2), [[0, 0], [0, 0]], [[0, 0], [0, 0]], [0, 0], [0, 0], [0, 0])


def test_several_columns_stack():
    v, c, d, m, t = FCY.expected_cols([[1, 2], [2]], [{1: 1, 2: 1}, {2: -1}], 2)
    np.testing.assert_array_equal(v, np.array([[[1, 0], [1, 0]], [[-1, 0], [-1, 0]]], np.int64))
    np.testing.assert_array_equal(c, np.array([[[2, 0], [1, 0]], [[1, 0], [1, 0]]], np.int64))
    np.testing.assert_array_equal(d, np.array([[1, 1], [1, 1]], np.int64))
    np.testing.assert_array_equal(m, np.array([[0, 0], [1, 0]], np.int64))
    np.testing.assert_array_equal(t, np.array([2, 1], np.int64))


def test_counts_plus_missing_equal_total_on_range_corpora():
    for metric, radius in (("l2", 2.6), ("ip", 0.55)):
        c = RY.corpus(16, 12, 1500, metric, seed=5)
        q = RY.queries(c, 9, seed=6)
        rng = np.random.default_rng(7)
        has = rng.random(c["ids"].shape[0]) < 0.8
        col = {int(i): int(v) for i, v in zip(c["ids"][has], rng.integers(-4, 5, size=int(has.sum())))}
        keep = rng.random(c["ids"].shape[0]) < 0.5
        for allowed in (None, FCY.allowed_ids(c["ids"], keep)):
            hits = FCY.hits_search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, radius, metric, allowed)
            lims = RY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 4, radius, metric, S=allowed)[0]
            v, cnt, d, m, t = FCY.expected(hits, col, 256)   # (more than the 9 values: every count is returned)
            assert t.sum() > 0 and m.sum() > 0
            np.testing.assert_array_equal(t, np.diff(lims))
            np.testing.assert_array_equal(cnt.sum(1) + m, t)
            np.testing.assert_array_equal((cnt > 0).sum(1), d)
            if allowed is not None:
                assert all(np.isin(h, allowed).all() for h in hits)
            pids = np.tile(np.array([3, -1, 5, 99], np.int64), (q.shape[0], 1))
            hs = FCY.hits_scan(q, c["vecs"], c["ids"], c["offsets"], pids, radius, metric, allowed)
            v, cnt, d, m, t = FCY.expected(hs, col, 256)
            np.testing.assert_array_equal(cnt.sum(1) + m, t)


# ---- the C ABI, as far as a machine without a GPU can check it ---------------------------------------------------------------
def test_header_declares_the_facet_surface():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    syms = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", txt))
    assert {"qk_facet_search", "qk_facet_scan"} <= syms
    assert re.search(r"^#define\s+QK_MAX_FACET_COLS\s+4\b", txt, re.M)
    assert re.search(r"^#define\s+QK_MAX_FACET_VALUES\s+256\b", txt, re.M)


def test_library_exports_and_binds_the_facet_symbols():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    for s in ("qk_facet_search", "qk_facet_scan"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert len(_lib.SIGNATURES[s][1]) == 19
    assert _lib.header_constant("QK_MAX_FACET_COLS") == 4 and _lib.header_constant("QK_MAX_FACET_VALUES") == 256


def test_facet_calls_with_a_null_context_fail_cleanly():
    """both entry points refuse a null context with an error code and a message; nothing is dereferenced"""
    from quake_amd import _lib
    lib = _lib.load()
    x = np.zeros((1, 4), np.float32)
    out = np.zeros(8, np.int64)
    cols = (C.c_void_p * 1)(None)
    p = lambda a: C.c_void_p(a.ctypes.data)
    st = lib.qk_facet_search(None, None, None, p(x), 1, 1, 1, C.c_float(1.0), None, cols, 1, 1, p(out), p(out), None, None, None, 0, None)
    assert st != 0
    assert b"qk_facet_search" in lib.qk_last_error()
    pids = np.zeros((1, 1), np.int64)
    st = lib.qk_facet_scan(None, None, p(x), 1, p(pids), 1, 1, C.c_float(1.0), None, cols, 1, 1, p(out), p(out), None, None, None, 0, None)
    assert st != 0
    assert b"qk_facet_scan" in lib.qk_last_error()
