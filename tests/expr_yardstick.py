"""The yardstick of expression filters (shared by tests/test_expr_filter_host.py and tests/test_expr_filter.py): an OR of
conjunctions over attribute columns, with value sets, on top of tests/attr_yardstick.py.

A column is a Python dict id -> int.  An expression is evaluated over (ids, columns) in plain numpy / Python integers -- nothing
here knows about masks, tiles, kernels or quake_amd/where.py -- which gives the allowed id set; the search over that set is
attr_yardstick.search / scan.

Two forms are evaluated, independently of each other:
  eval_expr    the C ABI's terms of (name, QK_OP_*, a, b, values) over int64; values: None or any sequence of int64
  eval_any_of  the mirrors' list of `where` lists over the integers, with ("col", "in" | "not_in", [v, ...])"""
import numpy as np

import attr_yardstick as AY

QK_OP_IN_SET, QK_OP_NOT_IN_SET = 5, 6
OP_CODES = dict(AY.OP_CODES, **{"in": QK_OP_IN_SET, "not_in": QK_OP_NOT_IN_SET})


def eval_expr(terms, ids, columns):
    """bool per id: does every clause of SOME term hold -- an id without a value fails every clause, NOT_IN_SET included"""
    ids = np.asarray(ids, np.int64)
    keep = np.zeros(ids.shape[0], bool)
    for term in terms:
        ok = np.ones(ids.shape[0], bool)
        for name, op, a, b, values in term:
            op = OP_CODES[op] if isinstance(op, str) else int(op)
            if op in (QK_OP_IN_SET, QK_OP_NOT_IN_SET):
                has, v = AY._lookup(ids, columns[name])
                member = np.isin(v, np.asarray(list(values), np.int64).reshape(-1))
                ok &= has & (member if op == QK_OP_IN_SET else ~member)
            else:
                ok &= AY.eval_clauses([(name, op, a, b)], ids, columns)
        keep |= ok
    return keep


def eval_any_of(any_of, ids, columns):
    """bool per id: does every (name, op, a[, b]) / (name, "in" | "not_in", values) of SOME list hold, in Python integers"""
    keep = np.zeros(len(ids), bool)
    for where in any_of:
        ok = np.ones(len(ids), bool)
        for cl in where:
            if cl[1] in ("in", "not_in"):
                col, values = columns[cl[0]], {int(x) for x in cl[2]}
                for i, id_ in enumerate(ids):
                    id_ = int(id_)
                    ok[i] = ok[i] and id_ in col and ((int(col[id_]) in values) == (cl[1] == "in"))
            else:
                ok &= AY.eval_where([cl], ids, columns)
        keep |= ok
    return keep
