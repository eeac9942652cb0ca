"""Lowering of the mirrors' predicate syntax to the clauses of the C ABI (include/quake_hip.h, "attribute filters").

`where` is a list of (name, op, a[, b]); the ops are "==" "!=" "<" "<=" ">" ">=" "between" "any_bits" "all_bits" "no_bits".  The C
ABI knows five ops over int64: RANGE / NOT_RANGE over a closed interval [a, b] (a > b: empty) and three bit tests.  Operands are
Python integers of any size and are saturated, not wrapped: a comparison with a number outside int64 means what it means over the
integers (x < 2^70 holds for every int64 x, x == 2^70 for none).  lower_expr adds the OR of up to 8 such conjunctions (`any_of`) and
the value sets ("col", "in" | "not_in", [v, ...]) of qk_filter_create_expr; a set value outside int64 is dropped by the same rule.
lower_edges normalises the histogram edges of facet statistics (QuakeIndex.facet_stats, Context.facet_stats_search), lower_order
the arguments of ordered search (QuakeIndex.ordered_search), lower_diverse those of diversified search (QuakeIndex.diverse_search), lower_maxsim those of multi-vector search
(QuakeIndex.multi_vector_search).
Pure Python: importable without the library or a GPU."""

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1

QK_OP_RANGE, QK_OP_NOT_RANGE, QK_OP_ANY_BITS, QK_OP_ALL_BITS, QK_OP_NO_BITS = 0, 1, 2, 3, 4
QK_OP_IN_SET, QK_OP_NOT_IN_SET = 5, 6
QK_MAX_CLAUSES = 8
QK_MAX_TERMS = 8
QK_MAX_EXPR_CLAUSES = 32
QK_MAX_SET_VALUES = 1 << 20

QK_MAX_FACET_EDGES = 255
QK_MAX_ORDER_K = 1024
QK_ORDER_DESC, QK_ORDER_MISSING_LAST = 1, 2
MISSING = ("exclude", "last")
QK_MAX_FETCH_K = 256
QK_MAXSIM_MAX_TOKENS, QK_MAXSIM_MAX_K = 64, 1024

OPS = ("==", "!=", "<", "<=", ">", ">=", "between", "any_bits", "all_bits", "no_bits")
SET_OPS = ("in", "not_in")  # lower_expr only
_BIT_OPS = {"any_bits": QK_OP_ANY_BITS, "all_bits": QK_OP_ALL_BITS, "no_bits": QK_OP_NO_BITS}
_SET_OPS = {"in": QK_OP_IN_SET, "not_in": QK_OP_NOT_IN_SET}
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


def _values(v, op, who):
    """the operand of a set op: ascending distinct int64 values; a value outside int64 equals no stored value and is dropped"""
    # (a sequence: indexable and sized -- a list, a tuple, a range, an array; not a set, whose order nobody should rely on)
    if isinstance(v, (str, bytes, dict)) or not (hasattr(v, "__getitem__") and hasattr(v, "__len__")):
        raise RuntimeError("%s the operand of %r must be a sequence of integers, got %r" % (who, op, v))
    if len(v) > QK_MAX_SET_VALUES:
        raise RuntimeError("%s the set of %r has %d values, at most %d are supported" % (who, op, len(v), QK_MAX_SET_VALUES))
    return tuple(sorted({x for x in (_int(x, who) for x in v) if INT64_MIN <= x <= INT64_MAX}))


def _lower_term(term, who):
    """one conjunction with the set ops: lower_where's clauses as (name, code, a, b, None), a set clause as (name, code, 0, 0, values)"""
    try:
        term = list(term)
    except TypeError:
        raise RuntimeError("%s a term is a list of where clauses, got %r" % (who, term))
    if len(term) < 1:
        raise RuntimeError("%s where needs at least one clause" % who)
    if len(term) > QK_MAX_CLAUSES:
        raise RuntimeError("%s where has %d clauses, at most %d are supported" % (who, len(term), QK_MAX_CLAUSES))
    out = []
    for cl in term:
        if isinstance(cl, (tuple, list)) and len(cl) >= 2 and isinstance(cl[0], str) and isinstance(cl[1], str) and cl[1] in _SET_OPS:
            if len(cl) != 3:
                raise RuntimeError("%s where op %r takes 1 operand(s), got %r" % (who, cl[1], cl))
            out.append((cl[0], _SET_OPS[cl[1]], 0, 0, _values(cl[2], cl[1], who)))
        else:
            try:
                out.append(lower_where([cl], who)[0] + (None,))
            except RuntimeError as e:  # (the op list of the message: the set ops belong to it here)
                if "unknown where op" in str(e):
                    raise RuntimeError("%s unknown where op %r (one of %s)" % (who, cl[1], " ".join(OPS + SET_OPS)))
                raise
    return out


def lower_expr(where=None, any_of=None, who="[QuakeIndex::make_filter()]"):
    """An OR of conjunctions -> [[(name, QK_OP_*, a, b, values), ...], ...]: `where` is one term, `any_of` a list of terms; a clause
    is lower_where's or (name, "in" | "not_in", [v, ...]).  values: None, or the ascending distinct int64 values of a set op.
    RuntimeError: what lower_where refuses per term, no term or more than QK_MAX_TERMS, more than QK_MAX_EXPR_CLAUSES clauses in
    total, a set operand that is no sequence or holds more than QK_MAX_SET_VALUES values."""
    if (where is None) == (any_of is None):
        raise RuntimeError("%s exactly one of where and any_of must be given" % who)
    if where is not None:
        return [_lower_term(where, who)]
    try:
        any_of = list(any_of)
    except TypeError:
        raise RuntimeError("%s any_of is a list of where lists, got %r" % (who, any_of))
    if len(any_of) < 1:
        raise RuntimeError("%s any_of needs at least one term" % who)
    if len(any_of) > QK_MAX_TERMS:
        raise RuntimeError("%s any_of has %d terms, at most %d are supported" % (who, len(any_of), QK_MAX_TERMS))
    terms = [_lower_term(t, who) for t in any_of]
    total = sum(len(t) for t in terms)
    if total > QK_MAX_EXPR_CLAUSES:
        raise RuntimeError("%s any_of has %d clauses in total, at most %d are supported" % (who, total, QK_MAX_EXPR_CLAUSES))
    return terms


def _is_seq(v):
    return not isinstance(v, (str, bytes, dict)) and hasattr(v, "__getitem__") and hasattr(v, "__len__")


def _edge_list(v, name, who):
    """the edges of one column: None or a sequence of strictly ascending int64 integers, at most QK_MAX_FACET_EDGES"""
    if v is None:
        return []
    if hasattr(v, "tolist"):  # (a tensor, an array: its elements as Python numbers)
        v = v.tolist()
    if not _is_seq(v):
        raise RuntimeError("%s the edges of '%s' must be a sequence of integers, got %r" % (who, name, v))
    if len(v) > QK_MAX_FACET_EDGES:
        raise RuntimeError("%s '%s' has %d edges, at most %d are supported" % (who, name, len(v), QK_MAX_FACET_EDGES))
    out = [_int(x, who + " edges:") for x in v]
    for i, x in enumerate(out):
        if not INT64_MIN <= x <= INT64_MAX:
            raise RuntimeError("%s edge %d of '%s' does not fit int64: %d" % (who, i, name, x))
        if i and out[i - 1] >= x:
            raise RuntimeError("%s the edges of '%s' are not strictly ascending (edge %d)" % (who, name, i))
    return out


def lower_edges(names, edges, who="[QuakeIndex::facet_stats()]"):
    """The histogram edges of facet statistics (include/quake_hip.h, "facet statistics") for the columns `names` ->
    (flat, n_edges): the columns' edges one after the other as a list of Python ints inside int64, and their number per column.
    `edges` is None (no edges: one bucket per column), one sequence of integers applied to every column, a dict name -> sequence
    (a column it does not name has no edges), or a list with one sequence or None per column; a tensor or an array stands for
    its tolist() wherever a sequence may stand.  RuntimeError: edges that are not strictly ascending, more than
    QK_MAX_FACET_EDGES of them, an edge that is no integer or does not fit int64, a dict that names a column not in `names`, a
    per-column list of another length."""
    names = list(names)
    if hasattr(edges, "tolist"):  # (a tensor, an array)
        edges = edges.tolist()
    if edges is None:
        per = [None] * len(names)
    elif isinstance(edges, dict):
        for k in edges:
            if k not in names:
                raise RuntimeError("%s edges names '%s', which is not one of the facet columns" % (who, k))
        per = [edges.get(n) for n in names]
    elif _is_seq(edges) and len(edges) > 0 and all(e is None or _is_seq(e) for e in edges):
        if len(edges) != len(names):
            raise RuntimeError("%s edges has %d per-column entries for %d columns" % (who, len(edges), len(names)))
        per = list(edges)
    else:
        per = [edges] * len(names)
    lists = [_edge_list(e, n, who) for e, n in zip(per, names)]
    return [x for l in lists for x in l], [len(l) for l in lists]


def lower_order(columns, order_by, k, descending=False, missing="exclude", who="[QuakeIndex::ordered_search()]"):
    """The arguments of ordered search (include/quake_hip.h, "ordered search") -> (column name, k, flags): `columns` are the names
    of the index's attribute columns, order_by one of them, 1 <= k <= QK_MAX_ORDER_K, missing "exclude" (hits without a value are
    left out) or "last" (they follow the hits that have one); flags = QK_ORDER_DESC | QK_ORDER_MISSING_LAST as asked.  RuntimeError,
    in this order: a name that is no string, an unknown column, k outside its bounds, another `missing`."""
    if not isinstance(order_by, str):
        raise RuntimeError("%s order_by must be the name of one attribute column, got %r" % (who, order_by))
    if order_by not in columns:
        raise RuntimeError("%s unknown attribute column '%s'" % (who, order_by))
    k = _int(k, who + " k:")
    if not 1 <= k <= QK_MAX_ORDER_K:
        raise RuntimeError("%s k=%d must be between 1 and %d" % (who, k, QK_MAX_ORDER_K))
    if not isinstance(missing, str) or missing not in MISSING:
        raise RuntimeError("%s missing must be 'exclude' or 'last', got '%s'" % (who, missing))
    return order_by, k, (QK_ORDER_DESC if descending else 0) | (QK_ORDER_MISSING_LAST if missing == "last" else 0)


def _to_f32(v):
    """v in [0, 1] rounded to the nearest float32, ties to even (this module imports nothing)"""
    if v == 0.0:
        return v
    e, p = 0, 1.0
    while p > v and e > -126:   # p = 2^e <= v < 2^(e + 1), or the subnormal range
        p /= 2.0
        e -= 1
    ulp = p / 8388608.0          # 2^(e - 23): every step is a scaling by a power of two, so nothing but round() rounds
    return round(v / ulp) * ulp


def lower_diverse(k, fetch_k, lambda_mult=0.5, who="[QuakeIndex::diverse_search()]"):
    """The arguments of diversified search (include/quake_hip.h, "diversified search") -> (k, fetch_k, lambda): 1 <= k <= fetch_k <=
    QK_MAX_FETCH_K, lambda_mult a number in [0, 1]; lambda is lambda_mult rounded to float32, the value qk_diverse_search computes
    with.  RuntimeError, in this order: k or fetch_k no integer, k < 1, fetch_k < k, fetch_k above the limit, a lambda_mult that is
    no number, NaN, or outside [0, 1]."""
    k = _int(k, who + " k:")
    fetch_k = _int(fetch_k, who + " fetch_k:")
    if k < 1:
        raise RuntimeError("%s k=%d must be at least 1" % (who, k))
    if fetch_k < k:
        raise RuntimeError("%s fetch_k=%d must be at least k=%d" % (who, fetch_k, k))
    if fetch_k > QK_MAX_FETCH_K:
        raise RuntimeError("%s fetch_k=%d must not exceed %d" % (who, fetch_k, QK_MAX_FETCH_K))
    if isinstance(lambda_mult, bool) or not isinstance(lambda_mult, (int, float)):
        raise RuntimeError("%s lambda_mult must be a number in [0, 1], got %r" % (who, lambda_mult))
    lam = float(lambda_mult)
    if lam != lam:
        raise RuntimeError("%s lambda_mult is NaN" % who)
    if not 0.0 <= lam <= 1.0:
        raise RuntimeError("%s lambda_mult=%g must lie in [0, 1]" % (who, lam))
    return k, fetch_k, _to_f32(lam)


def lower_maxsim(columns, group_by, k, T, n_tokens=None, missing=None, metric="ip", who="[QuakeIndex::multi_vector_search()]"):
    """The arguments of multi-vector search (include/quake_hip.h, "multi-vector search") -> (column name, k, T, n_tokens, missing):
    `columns` are the names of the index's attribute columns, group_by one of them, 1 <= k <= QK_MAXSIM_MAX_K, 1 <= T <=
    QK_MAXSIM_MAX_TOKENS, n_tokens None (T for every logical query) or a sequence of integers in [0, T] (returned as a list), missing
    the term of a sub-query without a candidate: None means 0.0 for the inner product and is an error for L2, where no value is the
    obvious one.  RuntimeError, in this order: a name that is no string, an unknown column, k outside its bounds, T outside its
    bounds, a bad n_tokens, a `missing` that is no number, NaN, or None under L2."""
    if not isinstance(group_by, str):
        raise RuntimeError("%s group_by must be the name of one attribute column, got %r" % (who, group_by))
    if group_by not in columns:
        raise RuntimeError("%s unknown attribute column '%s'" % (who, group_by))
    k = _int(k, who + " k:")
    if not 1 <= k <= QK_MAXSIM_MAX_K:
        raise RuntimeError("%s k=%d must be between 1 and %d" % (who, k, QK_MAXSIM_MAX_K))
    T = _int(T, who + " T:")
    if not 1 <= T <= QK_MAXSIM_MAX_TOKENS:
        raise RuntimeError("%s T=%d vectors per query must be between 1 and %d" % (who, T, QK_MAXSIM_MAX_TOKENS))
    if n_tokens is not None:
        if isinstance(n_tokens, (str, bytes)) or not hasattr(n_tokens, "__len__") or not hasattr(n_tokens, "__getitem__"):
            raise RuntimeError("%s n_tokens must be a sequence of integers, got %r" % (who, n_tokens))
        n_tokens = [_int(n_tokens[i], who + " n_tokens:") for i in range(len(n_tokens))]
        for i, n in enumerate(n_tokens):
            if not 0 <= n <= T:
                raise RuntimeError("%s n_tokens[%d]=%d must be between 0 and T=%d" % (who, i, n, T))
    is_ip = str(metric).lower() == "ip"
    if missing is None:
        if not is_ip:
            raise RuntimeError("%s missing must be given for the l2 metric: the term of a vector without a match has no default" % who)
        missing = 0.0
    if isinstance(missing, bool) or not isinstance(missing, (int, float)):
        raise RuntimeError("%s missing must be a number, got %r" % (who, missing))
    missing = float(missing)
    if missing != missing:
        raise RuntimeError("%s missing is NaN" % who)
    return group_by, k, T, n_tokens, missing
