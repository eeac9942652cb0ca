"""Attribute filters, the host side (no GPU): quake_amd/where.py lowers the mirrors' (name, op, a[, b]) clauses to the C ABI's
five int64 ops.  The lowering is checked against tests/attr_yardstick.py, which evaluates BOTH forms on its own: whatever the
high-level clause means over the integers, the lowered clause must mean over int64."""
import itertools

import numpy as np
import pytest

import attr_yardstick as AY
from quake_amd.where import EMPTY, OPS, QK_MAX_CLAUSES, lower_where

MIN, MAX = AY.INT64_MIN, AY.INT64_MAX
VALUES = [MIN, MIN + 1, -(1 << 40), -2, -1, 0, 1, 2, 5, 0xF0F0, 1 << 40, MAX - 1, MAX]
# operands: the values, and integers that are no int64
OPERANDS = VALUES + [MIN - 1, MAX + 1, -(1 << 70), 1 << 70]
# ids 0 .. len(VALUES)-1 carry the values; the last two ids have no value
IDS = np.arange(len(VALUES) + 2, dtype=np.int64)
COLS = {"c": {i: v for i, v in enumerate(VALUES)}}


def _check(where):
    low = lower_where(where)
    assert len(low) == len(where)
    for name, op, a, b in low:
        assert MIN <= a <= MAX and MIN <= b <= MAX and op in range(5)
    got = AY.eval_clauses(low, IDS, COLS)
    want = AY.eval_where(where, IDS, COLS)
    np.testing.assert_array_equal(got, want, err_msg=repr(where))
    return got


@pytest.mark.parametrize("op", [o for o in OPS if o not in ("between", "any_bits", "all_bits", "no_bits")])
def test_comparisons_against_the_yardstick(op):
    hit = 0
    for a in OPERANDS:
        hit += int(_check([("c", op, a)]).sum())
    assert hit > 0


def test_between_against_the_yardstick():
    some = 0
    for a, b in itertools.product(OPERANDS, OPERANDS):
        some += int(_check([("c", "between", a, b)]).any())
    assert some > 0


@pytest.mark.parametrize("op", ["any_bits", "all_bits", "no_bits"])
def test_bit_ops_against_the_yardstick(op):
    for a in VALUES + [(1 << 64) - 1, 1 << 63, 0x8000000000000001]:
        _check([("c", op, a)])
    with pytest.raises(RuntimeError, match="64 bits"):
        lower_where([("c", op, 1 << 64)])


def test_the_empty_interval():
    assert lower_where([("c", "<", MIN)]) == [("c", AY.QK_OP_RANGE) + EMPTY]
    assert lower_where([("c", ">", MAX)]) == [("c", AY.QK_OP_RANGE) + EMPTY]
    assert lower_where([("c", "between", 5, 4)]) == [("c", AY.QK_OP_RANGE) + EMPTY]
    assert lower_where([("c", "==", MAX + 1)]) == [("c", AY.QK_OP_RANGE) + EMPTY]
    assert EMPTY[0] > EMPTY[1]
    for where in ([("c", "<", MIN)], [("c", ">", MAX)], [("c", "between", 5, 4)], [("c", ">=", MAX + 1)], [("c", "<=", MIN - 1)]):
        assert not _check(where).any()
    # != lowers to the complement of [a, a]; of the empty interval when a is no int64: every id WITH a value
    assert lower_where([("c", "!=", 7)]) == [("c", AY.QK_OP_NOT_RANGE, 7, 7)]
    got = _check([("c", "!=", MAX + 1)])
    assert got[:len(VALUES)].all() and not got[len(VALUES):].any()
    # saturation, not wrap-around
    assert lower_where([("c", "<", 1 << 70)]) == [("c", AY.QK_OP_RANGE, MIN, MAX)]
    assert lower_where([("c", ">", MIN - 5)]) == [("c", AY.QK_OP_RANGE, MIN, MAX)]
    assert lower_where([("c", "<=", MAX)]) == [("c", AY.QK_OP_RANGE, MIN, MAX)]


def test_missing_values_fail_every_op():
    """SQL's NULL: an id without a value is no candidate, under != and no_bits too"""
    no_value = IDS[len(VALUES):]
    for where in ([("c", "!=", 123456)], [("c", "no_bits", 0)], [("c", "no_bits", -1)], [("c", "<=", MAX)], [("c", ">=", MIN)],
                  [("c", "all_bits", 0)]):
        got = _check(where)
        assert not got[len(VALUES):].any(), where
        for form in (AY.eval_clauses(lower_where(where), no_value, COLS), AY.eval_where(where, no_value, COLS)):
            assert not form.any(), where
    assert _check([("c", "no_bits", 0)])[:len(VALUES)].all()  # ... while every id with a value passes (v & 0) == 0


def test_conjunctions_and_order():
    rng = np.random.default_rng(3)
    pool = [("c", "!=", 0), ("c", ">=", -2), ("c", "<", 1 << 41), ("c", "any_bits", 0xFF), ("c", "no_bits", 1 << 62),
            ("c", "between", MIN, MAX - 1), ("c", "all_bits", 1), ("c", "<=", 1 << 70)]
    base = _check(pool)
    for _ in range(5):
        np.testing.assert_array_equal(_check([pool[i] for i in rng.permutation(len(pool))]), base)


def test_rejections():
    with pytest.raises(RuntimeError, match="at least one clause"):
        lower_where([])
    assert len(lower_where([("c", "==", i) for i in range(QK_MAX_CLAUSES)])) == QK_MAX_CLAUSES == 8
    with pytest.raises(RuntimeError, match="9 clauses"):
        lower_where([("c", "==", i) for i in range(9)])
    with pytest.raises(RuntimeError, match="unknown where op"):
        lower_where([("c", "=~", 1)])
    with pytest.raises(RuntimeError):
        lower_where([("c", "between", 1)])
    with pytest.raises(RuntimeError):
        lower_where([("c", "==", 1, 2)])
    with pytest.raises(RuntimeError):
        lower_where([("c", "==", 1.5)])
    with pytest.raises(RuntimeError):
        lower_where(["c == 1"])


def test_lowering_needs_no_library():
    """quake_amd.where imports nothing of the package: the lowering is usable where the library is not"""
    import ast
    import quake_amd.where as W
    tree = ast.parse(open(W.__file__).read())
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
