"""Lowering of the mirrors' predicate syntax to the clauses of the C ABI (include/quake_hip.h, "attribute filters").

`where` is a list of (name, op, a[, b]); the ops are "==" "!=" "<" "<=" ">" ">=" "between" "any_bits" "all_bits" "no_bits".  The C
ABI knows five ops over int64: RANGE / NOT_RANGE over a closed interval [a, b] (a > b: empty) and three bit tests.  Operands are
Python integers of any size and are saturated, not wrapped: a comparison with a number outside int64 means what it means over the
integers (x < 2^70 holds for every int64 x, x == 2^70 for none).  Pure Python: importable without the library or a GPU."""

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1

QK_OP_RANGE, QK_OP_NOT_RANGE, QK_OP_ANY_BITS, QK_OP_ALL_BITS, QK_OP_NO_BITS = 0, 1, 2, 3, 4
QK_MAX_CLAUSES = 8

OPS = ("==", "!=", "<", "<=", ">", ">=", "between", "any_bits", "all_bits", "no_bits")
_BIT_OPS = {"any_bits": QK_OP_ANY_BITS, "all_bits": QK_OP_ALL_BITS, "no_bits": QK_OP_NO_BITS}
EMPTY = (1, 0)  # the canonical empty interval


def _interval(lo, hi):
    """[lo, hi] over the integers cut to int64; EMPTY if nothing is left"""
    lo, hi = max(lo, INT64_MIN), min(hi, INT64_MAX)
    return (lo, hi) if lo <= hi else EMPTY


def _int(v, who):
    if isinstance(v, bool) or not hasattr(v, "__index__"):
        raise RuntimeError("%s operands must be integers, got %r" % (who, v))
    return v.__index__()


def lower_where(where, who="[QuakeIndex::make_filter()]"):
    """[(name, op, a[, b]), ...] -> [(name, QK_OP_*, a, b), ...] with a, b inside int64.  RuntimeError: no clause or more than
    QK_MAX_CLAUSES, an unknown op, a malformed clause, a bit mask that does not fit 64 bits."""
    where = list(where)
    if len(where) < 1:
        raise RuntimeError("%s where needs at least one clause" % who)
    if len(where) > QK_MAX_CLAUSES:
        raise RuntimeError("%s where has %d clauses, at most %d are supported" % (who, len(where), QK_MAX_CLAUSES))
    out = []
    for cl in where:
        if not isinstance(cl, (tuple, list)) or len(cl) < 3 or not isinstance(cl[0], str) or not isinstance(cl[1], str):
            raise RuntimeError("%s a where clause is (name, op, a[, b]), got %r" % (who, cl))
        name, op = cl[0], cl[1]
        if op not in OPS:
            raise RuntimeError("%s unknown where op %r (one of %s)" % (who, op, " ".join(OPS)))
        if len(cl) != (4 if op == "between" else 3):
            raise RuntimeError("%s where op %r takes %d operand(s), got %r" % (who, op, 2 if op == "between" else 1, cl))
        a = _int(cl[2], who)
        if op in _BIT_OPS:
            if not INT64_MIN <= a < (1 << 64):
                raise RuntimeError("%s the mask of %r does not fit 64 bits: %d" % (who, op, a))
            out.append((name, _BIT_OPS[op], a - (1 << 64) if a > INT64_MAX else a, 0))
            continue
        if op == "==":
            code, (lo, hi) = QK_OP_RANGE, _interval(a, a)
        elif op == "!=":  # the complement of [a, a]; of nothing, if a is no int64
            code, (lo, hi) = QK_OP_NOT_RANGE, _interval(a, a)
        elif op == "<":
            code, (lo, hi) = QK_OP_RANGE, _interval(INT64_MIN, a - 1)
        elif op == "<=":
            code, (lo, hi) = QK_OP_RANGE, _interval(INT64_MIN, a)
        elif op == ">":
            code, (lo, hi) = QK_OP_RANGE, _interval(a + 1, INT64_MAX)
        elif op == ">=":
            code, (lo, hi) = QK_OP_RANGE, _interval(a, INT64_MAX)
        else:  # between
            code, (lo, hi) = QK_OP_RANGE, _interval(a, _int(cl[3], who))
        out.append((name, code, lo, hi))
    return out
