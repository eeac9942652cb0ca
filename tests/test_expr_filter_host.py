"""Expression filters, the host side (no GPU): quake_amd/where.py's lower_expr lowers the mirrors' `where` / `any_of` -- an OR of
conjunctions with the value sets "in" / "not_in" -- to the terms of qk_filter_create_expr.  The lowering is checked against
tests/expr_yardstick.py, which evaluates BOTH forms on its own: whatever the high-level expression means over the integers, the
lowered terms must mean over int64."""
import numpy as np
import pytest

import attr_yardstick as AY
import expr_yardstick as EY
from quake_amd.where import (OPS, QK_MAX_CLAUSES, QK_MAX_EXPR_CLAUSES, QK_MAX_SET_VALUES, QK_MAX_TERMS, QK_OP_IN_SET, QK_OP_NOT_IN_SET,
                             lower_expr, lower_where)

MIN, MAX = AY.INT64_MIN, AY.INT64_MAX
VALUES = [MIN, -1, 0, 1, MAX]
# ids 0 .. 4 carry the values in both columns (d: reversed); the last two ids have no value in c, the last none in d
IDS = np.arange(len(VALUES) + 2, dtype=np.int64)
COLS = {"c": {i: v for i, v in enumerate(VALUES)}, "d": {i: v for i, v in enumerate(VALUES[::-1] + [7])}}
NV = len(VALUES)
SETS = [[], [0], [1, 1, 0, 1], [1 << 70, -(1 << 70)], [1 << 70, -1, -(1 << 70), MAX], [MAX, MIN, 0, -1, 1], [5, 3, MAX, -1, 3, MIN],
        [MIN], [MAX, MAX], list(range(-3, 4))[::-1]]


def _check(where=None, any_of=None):
    terms = lower_expr(where=where, any_of=any_of)
    src = [where] if where is not None else list(any_of)
    assert len(terms) == len(src)
    for term, w in zip(terms, src):
        assert len(term) == len(w)
        for name, op, a, b, values in term:
            assert MIN <= a <= MAX and MIN <= b <= MAX and op in range(7)
            assert (values is not None) == (op in (QK_OP_IN_SET, QK_OP_NOT_IN_SET))
            if values is not None:
                assert isinstance(values, tuple) and list(values) == sorted(set(values)) and all(MIN <= v <= MAX for v in values)
    got = EY.eval_expr(terms, IDS, COLS)
    want = EY.eval_any_of(src, IDS, COLS)
    np.testing.assert_array_equal(got, want, err_msg=repr(src))
    return got


@pytest.mark.parametrize("op", ["in", "not_in"])
def test_set_ops_against_the_yardstick(op):
    hit = 0
    for s in SETS:
        got = _check(where=[("c", op, s)])
        assert not got[NV:].any()  # an id without a value fails both
        hit += int(got.sum())
        _check(any_of=[[("d", op, tuple(s))], [("c", "==", 1)]])
    assert hit > 0


def test_what_becomes_of_a_set():
    assert lower_expr(where=[("c", "in", [])]) == [[("c", QK_OP_IN_SET, 0, 0, ())]]
    assert lower_expr(where=[("c", "not_in", [3, 1, 3, 2, 1])]) == [[("c", QK_OP_NOT_IN_SET, 0, 0, (1, 2, 3))]]
    # no int64 equals 2^70: dropped, not wrapped
    assert lower_expr(where=[("c", "in", [1 << 70, 5, -(1 << 70), MAX + 1, MIN - 1, MIN])]) == [[("c", QK_OP_IN_SET, 0, 0, (MIN, 5))]]
    assert lower_expr(where=[("c", "in", np.array([2, 1], np.int64))])[0][0][4] == (1, 2)
    assert lower_expr(where=[("c", "in", range(2, 0, -1))])[0][0][4] == (1, 2)
    # the empty set: `in` matches nothing, `not_in` every id that has a value
    assert not _check(where=[("c", "in", [])]).any()
    got = _check(where=[("c", "not_in", [])])
    assert got[:NV].all() and not got[NV:].any()
    got = _check(where=[("c", "not_in", [1 << 70])])
    assert got[:NV].all() and not got[NV:].any()


@pytest.mark.parametrize("op", OPS)
def test_old_ops_inside_terms(op):
    """every old op keeps lower_where's clause, inside a term of its own and next to a set clause"""
    for a in VALUES + [MAX + 1] + ([] if op.endswith("_bits") else [-(1 << 70)]):  # (a bit mask has to fit 64 bits)
        cl = ("c", op, a, 1) if op == "between" else ("c", op, a)
        assert lower_expr(where=[cl]) == [[lower_where([cl])[0] + (None,)]]
        _check(where=[cl])
        _check(any_of=[[cl], [("d", "in", [MIN, 7])]])
        _check(any_of=[[cl, ("d", "not_in", [0])], [("c", "==", MAX)]])


def test_identities():
    for a in VALUES + [5, 1 << 70]:
        np.testing.assert_array_equal(_check(where=[("c", "in", [a])]), _check(where=[("c", "==", a)]))
        np.testing.assert_array_equal(_check(where=[("c", "not_in", [a])]), _check(where=[("c", "!=", a)]))
    w = [("c", ">=", -1), ("d", "not_in", [0, 1]), ("c", "any_bits", 1)]
    np.testing.assert_array_equal(_check(any_of=[w]), _check(where=w))
    assert lower_expr(any_of=[w]) == lower_expr(where=w)
    for s in SETS:
        np.testing.assert_array_equal(_check(any_of=[[("c", "in", s)], [("c", "not_in", s)]]), _check(where=[("c", "no_bits", 0)]))
    assert _check(where=[("c", "no_bits", 0)])[:NV].all()


def test_term_order_and_clause_order():
    rng = np.random.default_rng(4)
    any_of = [[("c", "in", [MIN, 0, MAX]), ("d", "!=", 0)], [("c", "==", -1), ("d", "not_in", [5]), ("d", ">", 0)], [("d", "==", 7)],
              [("c", "between", 5, 4)]]
    base = _check(any_of=any_of)
    assert 0 < base.sum() < base.shape[0]
    for _ in range(6):
        perm = [[t[i] for i in rng.permutation(len(t))] for t in (any_of[j] for j in rng.permutation(len(any_of)))]
        np.testing.assert_array_equal(_check(any_of=perm), base)


def test_rejections():
    one = [("c", "==", 1)]
    with pytest.raises(RuntimeError, match="exactly one of"):
        lower_expr()
    with pytest.raises(RuntimeError, match="exactly one of"):
        lower_expr(where=one, any_of=[one])
    with pytest.raises(RuntimeError, match="at least one term"):
        lower_expr(any_of=[])
    assert len(lower_expr(any_of=[one] * QK_MAX_TERMS)) == QK_MAX_TERMS == 8
    with pytest.raises(RuntimeError, match="9 terms"):
        lower_expr(any_of=[one] * 9)
    with pytest.raises(RuntimeError, match="at least one clause"):
        lower_expr(any_of=[one, []])
    with pytest.raises(RuntimeError, match="at least one clause"):
        lower_expr(where=[])
    with pytest.raises(RuntimeError, match="9 clauses"):
        lower_expr(any_of=[one, one * 9])
    with pytest.raises(RuntimeError, match="9 clauses"):
        lower_expr(where=[("c", "in", [1])] * 9)
    assert sum(len(t) for t in lower_expr(any_of=[one * QK_MAX_CLAUSES] * 4)) == QK_MAX_EXPR_CLAUSES == 32
    with pytest.raises(RuntimeError, match="33 clauses in total"):
        lower_expr(any_of=[one * 8] * 4 + [one])
    big = np.zeros(QK_MAX_SET_VALUES + 1, np.int64)
    assert lower_expr(where=[("c", "in", big[:-1])])[0][0][4] == (0,)  # (the limit is on the values as given)
    with pytest.raises(RuntimeError, match="%d values" % (QK_MAX_SET_VALUES + 1)):
        lower_expr(where=[("c", "in", big)])
    for bad in (5, "12", None, {1: 2}, {1, 2}, frozenset([1]), iter([1])):
        with pytest.raises(RuntimeError, match="must be a sequence"):
            lower_expr(where=[("c", "in", bad)])
    with pytest.raises(RuntimeError, match="operands must be integers"):
        lower_expr(where=[("c", "in", [1, True])])
    with pytest.raises(RuntimeError, match="operands must be integers"):
        lower_expr(where=[("c", "not_in", [1.5])])
    with pytest.raises(RuntimeError):
        lower_expr(where=[("c", "in", [1], [2])])
    with pytest.raises(RuntimeError, match="unknown where op"):
        lower_expr(any_of=[[("c", "=~", 1)]])
    with pytest.raises(RuntimeError):
        lower_expr(any_of=[one, 5])
    # lower_where is what it was: 4-tuples, and the set ops are unknown to it
    assert lower_where(one) == [("c", AY.QK_OP_RANGE, 1, 1)]
    with pytest.raises(RuntimeError, match="unknown where op"):
        lower_where([("c", "in", [1])])


def test_lowering_needs_no_library():
    """quake_amd.where still imports nothing"""
    import ast
    import quake_amd.where as W
    tree = ast.parse(open(W.__file__).read())
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
