"""The cases of the random-shape sweep over the entry points that run on the filtered tile form: filtered search, per-query
filters, predicate filters, adaptive probing, range search, grouped search with members and paged search
(tests/test_random_shapes_gpu.py runs them on the device, tests/test_random_features_oracle.py pins on the CPU that the seed set
reaches what the sweep exists for).

feature_case(seed) is the shape the plain sweep draws for that seed -- test_random_shapes_gpu._case on the same 1000 + seed
generator, untouched -- plus what the newer entry points need, drawn from a second generator (77000 + seed) so that the draws of
the existing tests do not move.  SEAM_CASES are four fixed shapes _case cannot draw.  expected() gives every leg's answer, and every
number in it comes from the yardsticks of the entry points' own test files and from the oracle: nothing here computes a distance,
a key or an order.  No clock is read."""
import os

import numpy as np

import adaptive_yardstick as A
import attr_yardstick as AT
import filter_yardstick as FY
import grouped_members_yardstick as GMY
import oracle as O
import paging_yardstick as PY
import range_yardstick as RY

QK_MAX_K = 448
QK_MAX_NPROBE = 8192
QK_GROUPED_PASS_BYTES = 1 << 31
ONE_AT_A_TIME = 48   # the grouped yardstick and PY.ordering work one query at a time: their legs take the first min(Q, 48) queries
PAGES = 3
SELECTIVITIES = [1, 0.5, 0.1, 0.01, 0]
LEGS = ["filtered", "batch", "where", "adaptive", "range", "grouped", "pages"]
# the seeds of test_random_shape_features_after_mutation: 16 of the default set, at least 8 of them with d % 16 != 0 (pinned on the CPU)
MUTATION_SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def default_seeds():
    """0 .. QK_RANDOM_FEATURES - 1 (default 48) and 107, the seed the plain sweep keeps"""
    return sorted(set(range(int(os.environ.get("QK_RANDOM_FEATURES", "48")))) | {107})


def shape_tag(c):
    t = {kk: c[kk] for kk in ("d", "nlist", "metric", "integer", "n", "Q", "nprobe", "k")}
    f = c["f"]
    t.update(sel=f["sel"], mode=f["sets"][0][1], m=f["m"], group_by=f["group_by"], minc=f["min_candidates"], where=f["where"][1:])
    return t


def _features(c, seed):
    """what the newer entry points need on top of a shape, from a generator of its own"""
    rng = np.random.default_rng(77000 + seed)
    ids, n, k, Q = c["ids"], c["n"], c["k"], c["Q"]
    f = {}
    # three id filters: the one every single-filter leg uses, a second one, and the deny-nothing filter -- a per-query table takes
    # no NULL handle (QK_ERR_INVALID), the interface's "unfiltered" entry is a deny filter of the empty set
    f["sel"] = float(rng.choice(SELECTIVITIES))
    sets = [(FY.draw_set(ids, f["sel"], rng), str(rng.choice(["allow", "deny"])))]
    sets.append((FY.draw_set(ids, float(rng.choice(SELECTIVITIES)), rng), "deny" if sets[0][1] == "allow" else "allow"))
    sets.append((np.zeros(0, np.int64), "deny"))
    f["sets"] = sets
    # two columns over ~90 % of the ids each: a few values / about n / 3 values scattered over the int64 range
    card = int(rng.integers(2, 8))
    nh = max(1, int(round(0.9 * n)))
    ha = np.ascontiguousarray(rng.permutation(ids)[:nh])
    hb = np.ascontiguousarray(rng.permutation(ids)[:nh])
    f["cols"] = {"a": (ha, rng.integers(0, card, size=nh).astype(np.int64)),
                 "b": (hb, rng.integers(0, max(1, n // 3), size=nh).astype(np.int64) * 1000003 - 7)}
    lo = int(rng.integers(0, card))
    f["where"] = ("a", "range", lo, min(card - 1, lo + int(rng.integers(0, 2))))
    f["group_by"] = str(rng.choice(["a", "b"]))
    f["m"] = int(rng.choice([1, 2, 3, 16]))
    f["max_nprobe"] = min(4 * c["nprobe"], QK_MAX_NPROBE)
    f["min_candidates"] = int(rng.choice([k, 3 * k]))
    # the table of the per-query legs: the three id filters and the predicate
    f["query_filter"] = rng.integers(0, 4, size=Q).astype(np.int32)
    f["leg_order"] = [LEGS[i] for i in rng.permutation(len(LEGS))]
    # the radius comes from the reference: the median of the finite distances of its unfiltered k-NN answer
    _, od = O.search(c["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], c["nprobe"], k, c["metric"], batched_scan=True, num_threads=8)
    fin = od[np.isfinite(od)]
    f["radius"] = float(np.float32(np.median(fin))) if fin.shape[0] else 0.0
    c["f"] = f
    return c


def feature_case(seed):
    from test_random_shapes_gpu import _case
    return _features(_case(np.random.default_rng(1000 + seed)), seed)


# ---- the seams: shapes _case cannot draw ------------------------------------------------------------------------------------------
# 12 lists, two of them empty, about 1500 rows (the corpus of tests/range_yardstick.py), Q = 20: 16 blocks; 17 blocks, the last one
# ragged; 63 blocks, ragged, several waves per tile; the wide form with a ragged last block
SEAM_CASES = [dict(d=256, metric="l2", k=10), dict(d=260, metric="ip", k=100), dict(d=1000, metric="l2", k=100),
              dict(d=3000, metric="ip", k=10)]


def seam_case(i):
    s = SEAM_CASES[i]
    r = RY.corpus(s["d"], 12, 1500, s["metric"], seed=88000 + i)
    q = RY.queries(r, 20, seed=88100 + i)
    c = dict(d=s["d"], nlist=12, metric=s["metric"], integer=False, n=int(r["ids"].shape[0]), cent=r["cent"], vecs=r["vecs"],
             ids=r["ids"], offsets=r["offsets"], Q=20, nprobe=4, k=s["k"], q=q)
    return _features(c, 900 + i)


# ---- expected values ----------------------------------------------------------------------------------------------------------------
def column_dict(col):
    return {int(i): int(v) for i, v in zip(*col)}


def where_keep(c, ids, cols=None):
    """bool per row of `ids`: the case's predicate, by tests/attr_yardstick.py"""
    cols = c["f"]["cols"] if cols is None else cols
    name, op, a, b = c["f"]["where"]
    return AT.eval_clauses([(name, op, a, b)], ids, {name: column_dict(cols[name])})


def table_sets(c, ids, cols=None):
    """the per-query table as (S, mode) pairs: the three id filters, then the predicate as the allow set it stands for"""
    return list(c["f"]["sets"]) + [(AT.allowed_set(where_keep(c, ids, cols), ids), "allow")]


def refused_legs(c, offsets=None, cols=None):
    """the legs the interface documents a refusal for at this shape (include/quake_hip.h): a page beyond QK_MAX_K; a grouped call
    whose single query exceeds QK_GROUPED_PASS_BYTES by the header's workspace formula"""
    out = set()
    if c["k"] > QK_MAX_K:
        out.add("pages")
    if c["k"] > QK_MAX_K or c["f"]["max_nprobe"] > QK_MAX_NPROBE:
        out.update(("filtered", "batch", "where", "adaptive"))
    offsets = c["offsets"] if offsets is None else offsets
    cols = c["f"]["cols"] if cols is None else cols
    ub = min(c["nprobe"], c["nlist"]) * int(np.diff(offsets).max())
    T = 16
    while T < 2 * min(ub, cols[c["f"]["group_by"]][0].shape[0]):
        T *= 2
    if 12 * ub + 24 * (T + 1) + 12 * c["k"] + 4 * c["k"] * c["f"]["m"] > QK_GROUPED_PASS_BYTES or c["k"] > 8192:
        out.add("grouped")
    return out


def _scatter(Q, k, metric, qf, sets, fn):
    oi = np.full((Q, k), -1, np.int64)
    od = np.full((Q, k), A.pad_of(metric), np.float32)
    for t in np.unique(qf):
        rows = np.nonzero(qf == t)[0]
        oi[rows], od[rows] = fn(rows, *sets[int(t)])
    return oi, od


def _pages(c, q, vecs, ids, offsets, S, mode):
    """PAGES + 1 chained pages of size k as the column slices of the filtered yardstick asked for (PAGES + 1) * k, and the cursor
    behind every page: the key of its last row (PY.key_of of the oracle's canonical value of that pair) and its id, or the exhausted
    cursor where the page is short.  keys: the key of every returned entry (0xFFFFFFFF where padded)"""
    k, metric = c["k"], c["metric"]
    K = (PAGES + 1) * k
    fi, fd = FY.search(q, c["cent"], vecs, ids, offsets, c["nprobe"], K, metric, S, mode)
    order = np.argsort(ids, kind="stable")
    keys = np.full(fi.shape, 0xFFFFFFFF, np.uint32)
    for i in range(q.shape[0]):
        have = fi[i] >= 0
        if have.any():
            rows = order[np.searchsorted(ids[order], fi[i][have])]
            keys[i, have] = PY.key_of(O.pair_values(q[i:i + 1], vecs[rows], metric)[0], metric)
    pages, cursors = [], []
    for p in range(PAGES + 1):
        pages.append((np.ascontiguousarray(fi[:, p * k:(p + 1) * k]), np.ascontiguousarray(fd[:, p * k:(p + 1) * k])))
        last = (p + 1) * k - 1
        cursors.append([(int(keys[i, last]), int(fi[i, last])) if fi[i, last] >= 0 else PY.EXHAUSTED for i in range(q.shape[0])])
    return dict(pages=pages, cursors=cursors, keys=keys, ids=fi)


def expected(c, csr=None, cols=None, legs=LEGS):
    """every leg's expected answer over the case's CSR -- or over csr = (vecs, ids, offsets) and cols, what a mutated store holds"""
    vecs, ids, offsets = (c["vecs"], c["ids"], c["offsets"]) if csr is None else csr
    f = c["f"]
    cols = f["cols"] if cols is None else cols
    q, cent, nprobe, k, metric, Q = c["q"], c["cent"], c["nprobe"], c["k"], c["metric"], c["Q"]
    S, mode = f["sets"][0]
    e = {}
    if "filtered" in legs:
        e["filtered"] = FY.search(q, cent, vecs, ids, offsets, nprobe, k, metric, S, mode)
        e["coarse"] = O.coarse(q, cent, None, nprobe, metric, num_threads=8)[0]
    keep = where_keep(c, ids, cols)
    tsets = table_sets(c, ids, cols)
    if "batch" in legs:
        e["batch"] = _scatter(Q, k, metric, f["query_filter"], tsets, lambda rows, S_, mode_: FY.search(
            np.ascontiguousarray(q[rows]), cent, vecs, ids, offsets, nprobe, k, metric, S_, mode_))
    if "where" in legs:
        e["where"] = AT.search(q, cent, vecs, ids, offsets, nprobe, k, metric, keep)
    if "adaptive" in legs:
        e["adaptive"] = A.search(q, cent, vecs, ids, offsets, nprobe, f["max_nprobe"], f["min_candidates"], k, metric, [(S, mode)])
        e["adaptive_table"] = A.search(q, cent, vecs, ids, offsets, nprobe, f["max_nprobe"], f["min_candidates"], k, metric,
                                       list(f["sets"]) + [keep], f["query_filter"])
    if "range" in legs:
        e["range"] = RY.search(q, cent, vecs, ids, offsets, nprobe, f["radius"], metric)
        e["range_filtered"] = RY.search(q, cent, vecs, ids, offsets, nprobe, f["radius"], metric, S, mode)
    if "grouped" in legs:
        q1 = np.ascontiguousarray(q[:ONE_AT_A_TIME])
        ai, av = cols[f["group_by"]]
        e["grouped"] = GMY.search(q1, cent, vecs, ids, offsets, nprobe, k, f["m"], metric, ai, av)
        e["grouped_filtered"] = GMY.search(q1, cent, vecs, ids, offsets, nprobe, k, f["m"], metric, ai, av, S, mode)
    if "pages" in legs:
        e["pages"] = _pages(c, q, vecs, ids, offsets, np.zeros(0, np.int64), "deny")
        e["pages_filtered"] = _pages(c, q, vecs, ids, offsets, S, mode)
    return e


def resumed_page(c, csr, cursors, S=None, mode="allow"):
    """the page behind `cursors` (a list of (key, id), one per query of the first min(Q, 48)) over csr, by PY.ordering / PY.page"""
    vecs, ids, offsets = csr
    q1 = np.ascontiguousarray(c["q"][:ONE_AT_A_TIME])
    order = PY.ordering(q1, c["cent"], vecs, ids, offsets, c["nprobe"], c["metric"], S=S, mode=mode)
    return PY.page(order, cursors, c["k"])
