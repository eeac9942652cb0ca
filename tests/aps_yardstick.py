"""The yardstick of the recall-target walk (adaptive partition scanning, qk_search_aps) outside the corner its first suite stays in
(shared by tests/test_aps_walk_oracle.py and tests/test_aps_walk.py).

A case is a small dict: the corpus (`kind` + n, d, nlist, seed), the queries (Q), and the call (k, metric, target, fraction,
threshold, use_precomputed).  corpus() builds -- once per corpus -- the CSR arena, the centroids and the queries on top of
helpers.make_ivf / make_queries (nonfinite_yardstick.corpus for the planted classes, the draws of
test_wide_dim.py::test_recall_target_walk for the wide row); expected() is the oracle's walk, computed once per case and handed out
read-only; assert_same() is the one comparison: partitions visited, ids, float32 distance bits (zeros by value on the non-finite
corpora, nonfinite_yardstick.assert_same_answer).

What the sections are for (quake_amd/csrc/qk_aps.hip):
  K_BUCKETS     both sides of every k_aps_update<MAXCH> boundary (2k <= 64 / 128 / 256 / 512 / more) and QK_MAX_K; entries past the
                64 that a wave prefetches; lists shorter than k, so that the running result stays below k (the sentinel radius) and
                an answer is merged from many lists
  LONG_ROUNDS   rounds of more than 64 steps (several ballot words) and the exit without a stop (all M candidates scanned)
  CAPPED        a round's row shorter than the remaining walk (CH < M): state carried over at least three rounds
  SQUARED       the k values run with squared L2 output
  NONFINITE     NaN / Inf / overflow / underflow rows and queries (centroids stay finite)
  WIDE          d = 3072: the per-pair wide scan beyond k = 10
  FIRST_ROUND   the cases run under another length of the first round (the schedule changes no result)
and parent_steps(): one parent with non-identity ids edited under a live context."""
import functools

import numpy as np

import nonfinite_yardstick as NF
import oracle as O
from helpers import make_ivf, make_queries

QK_MAX_K = 448          # include/quake_hip.h
APS_FIRST = 4           # partitions of the first round (qk_aps.hip)
PAIR_BYTES = 1 << 30    # memory of a later round's per-pair results: CH = min(M, max(80, PAIR_BYTES / (Q * k * 12)))


def case(kind, n, d, nlist, Q, k, metric, target, fraction, threshold=0.001, use_precomputed=True, seed=0, **extra):
    return dict(kind=kind, n=n, d=d, nlist=nlist, Q=Q, k=k, metric=metric, target=target, fraction=fraction, threshold=threshold,
                use_precomputed=use_precomputed, seed=seed, **extra)


def case_key(c):
    """every field of the case: two cases are the same one only when all of them agree"""
    return tuple(sorted(c.items()))


def case_id(c):
    tag = c["kind"] + ("-" + c["cls"] if "cls" in c else "")
    return "%s-%s-k%d-t%g-f%g%s" % (tag, c["metric"], c["k"], c["target"], c["fraction"], "" if c["use_precomputed"] else "-exactbeta")


def M_of(c, nlist=None):
    return max(int(np.float32(c["nlist"] if nlist is None else nlist) * np.float32(c["fraction"])), 1)


def round_cap(c):
    """CH of the case: the longest row of a later round"""
    M = M_of(c)
    return min(M, max(80, min(M, PAIR_BYTES // (c["Q"] * c["k"] * 12))))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
BUCKET_K = (33, 64, 65, 128, 129, 256, 257, 448)


def _bucket(k, metric, target=0.9, kind="ivf"):
    # the exact incomplete beta instead of the table on one k of each side of the pools (it matters under L2 only: the IP profile never
    # reads the table, so the flag changes nothing there and is set all the same)
    return case(kind, 30000, 48, 60, 130, k, metric, target, 0.5, use_precomputed=k not in (65, 256), seed=11)


K_BUCKETS = [_bucket(k, m) for m in ("l2", "ip") for k in BUCKET_K] + [_bucket(k, m, kind="short") for m in ("l2", "ip") for k in (129, 448)]
# Lists of about 50 rows, all shorter than k: where the lists above hold 500 rows and a well-separated corpus answers k <= 448 from the
# nearest list alone, every step here merges a whole list into the running result, which stays below k for the first steps.
THIN = [case("ivf", 30000, 48, 600, 130, k, m, 0.9, 0.125, seed=19) for m in ("l2", "ip") for k in (129, 448)]
K_BUCKETS += THIN
SHORT_LISTS, SHORT_CUTS = (3, 17, 22), (0, 4, 9)   # the lists of kind "short" cut to these many rows, queries 0..2 at their centroids


def _long(k, metric, target):
    return case("ivf", 40000, 16, 1200, 48, k, metric, target, 0.5, seed=15)


LONG_ROUNDS = [_long(10, m, t) for m in ("l2", "ip") for t in (0.99, 2.0)] + [_long(129, m, 2.0) for m in ("l2", "ip")]
LONG_STEPS = 64 + APS_FIRST   # a walk past this many lists has a round of more than 64 steps behind it
CAPPED = [case("ivf", 40000, 16, 2000, 512, 256, "l2", t, 0.5, seed=17) for t in (0.99, 2.0)]
SQUARED = [_bucket(k, "l2") for k in (10, 129)]
NONFINITE = [case("nonfinite", 6000, 32, 24, 40, k, m, t, f, seed=23, cls=cls)
             for m in ("l2", "ip") for cls in NF.CLASSES for k in (3, 10) for t, f in ((0.9, 0.5), (2.0, 1.0))]
WIDE = [case("wide", 3000, 3072, 24, 20, 129, m, 0.99, 0.5, seed=31) for m in ("l2", "ip")]
GROUP = [_bucket(k, m, kind=kind) for m in ("l2", "ip") for kind in ("ivf", "short") for k in (129, 448)] + \
        [_long(k, m, 2.0) for m in ("l2", "ip") for k in (10, 129)]
FIRST_ROUND = [_bucket(k, m, t) for m in ("l2", "ip") for k in (10, 129) for t in (0.5, 0.9)]
FIRST_ROUND_LENGTHS = (2, 9)
ALL = K_BUCKETS + LONG_ROUNDS + CAPPED + SQUARED + NONFINITE + WIDE + FIRST_ROUND


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _wide(n, d, nlist, Q, metric, seed):
    """clustered rows in skewed lists -- one empty, two of a handful of rows at most -- and queries around the rows: the draws of
    tests/test_wide_dim.py::test_recall_target_walk, stated here so that the CPU test needs no GPU module"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 0.05
    w[:1] = 0.0
    w[1:3] = 1e-4
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) + 7
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    q = (x[rng.integers(0, n, size=Q)] + 0.05 * rng.standard_normal((Q, d))).astype(np.float32)
    return dict(centroids=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets, q=q, d=d,
                nlist=nlist)


@functools.lru_cache(maxsize=4)
def _corpus(kind, n, d, nlist, Q, metric, seed, cls):
    if kind == "nonfinite":
        c = NF.corpus(cls, metric, n, nlist, d, seed, far_tiny=False)
        q, special = NF.queries(c, Q, seed)
        c = dict(c, q=q, special_q=special)
    elif kind == "wide":
        c = _wide(n, d, nlist, Q, metric, seed)
    else:
        ivf = make_ivf(n, d, nlist, seed=seed, metric=metric)
        q = make_queries(Q, d, seed=seed + 1, like=ivf["x"], metric=metric)
        c = dict(centroids=ivf["centroids"], vecs=ivf["vecs"], ids=ivf["ids"], offsets=ivf["offsets"], q=q, d=d, nlist=nlist)
        if kind == "short":   # the pattern of test_aps_gpu.py::test_aps_first_round_bound_edges
            offs, keep = c["offsets"], np.ones(len(c["ids"]), bool)
            for p, cut in zip(SHORT_LISTS, SHORT_CUTS):
                keep[int(offs[p]) + cut:int(offs[p + 1])] = False
            sizes = np.array([keep[int(offs[p]):int(offs[p + 1])].sum() for p in range(nlist)], np.int64)
            offs2 = np.zeros(nlist + 1, np.int64)
            offs2[1:] = np.cumsum(sizes)
            q = q.copy()
            for t, p in enumerate(SHORT_LISTS):
                q[t] = c["centroids"][p]
            c = dict(c, offsets=offs2, ids=np.ascontiguousarray(c["ids"][keep]), vecs=np.ascontiguousarray(c["vecs"][keep]), q=q)
        else:
            assert kind == "ivf", kind
    _freeze(*c.values())
    return c


def corpus(c):
    """dict: centroids, vecs, ids, offsets (CSR), q, d, nlist (+ the fields of nonfinite_yardstick.corpus and special_q); read-only"""
    return _corpus(c["kind"], c["n"], c["d"], c["nlist"], c["Q"], c["metric"], c["seed"], c.get("cls"))


def oracle_walk(c, co, **kw):
    return O.search_aps(co["q"], co["centroids"], co["vecs"], co["ids"], co["offsets"], c["k"], c["metric"], c["target"],
                        recompute_threshold=c["threshold"], use_precomputed=c["use_precomputed"], initial_search_fraction=c["fraction"],
                        expanded=True, num_threads=8, **kw)


_EXPECTED = {}


def expected(c):
    """(ids, dist, nscanned) of the oracle's walk; computed once per case, read-only"""
    key = case_key(c)
    if key not in _EXPECTED:
        if len(_EXPECTED) >= 8:
            _EXPECTED.pop(next(iter(_EXPECTED)))
        out = oracle_walk(c, corpus(c))
        _freeze(*out)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def device_walk(ctx, parent, s, c, q=None, **kw):
    """the case through capi.Context.search_aps (or a Group's, with s=None)"""
    q = corpus(c)["q"] if q is None else q
    args = (q, c["k"], c["metric"], c["target"])
    kw = dict(dict(recompute_threshold=c["threshold"], use_precomputed=c["use_precomputed"], initial_search_fraction=c["fraction"]), **kw)
    return ctx.search_aps(parent, *args, **kw) if s is None else ctx.search_aps(parent, s, *args, **kw)


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def assert_same(c, got, want, tag=""):
    """partitions visited, ids, float32 distance bits -- all equal.  On the non-finite corpora the sign of a returned zero is not
    compared (nonfinite_yardstick.assert_same_answer)."""
    gi, gd, gn = (_np(a) for a in got[:3])
    oi, od, on = want
    msg = "%s %s" % (case_id(c), tag)
    np.testing.assert_array_equal(gn, on, err_msg=msg + ": partitions visited")
    if c["kind"] == "nonfinite":
        NF.assert_same_answer(gi, gd, oi, od)
    else:
        np.testing.assert_array_equal(gi, oi, err_msg=msg + ": ids")
        np.testing.assert_array_equal(np.ascontiguousarray(gd, np.float32).view(np.uint32), od.view(np.uint32), err_msg=msg + ": distance bits")


def fixed_nprobe_answer(c, co, nscanned, centroid_ids=None, nlist_present=None):
    """the answer of a fixed-nprobe search over each query's first nscanned[q] ranked lists"""
    M = M_of(c, nlist_present)
    pids, _ = O.coarse(co["q"], co["centroids"], centroid_ids, M, c["metric"], num_threads=8)
    Q, k = co["q"].shape[0], c["k"]
    wi, wd = np.empty((Q, k), np.int64), np.empty((Q, k), np.float32)
    for n in np.unique(nscanned):   # the queries of one walk length in one call
        sel = np.nonzero(nscanned == n)[0]
        wi[sel], wd[sel] = O.batched_serial_scan(co["q"][sel], co["vecs"], co["ids"], co["offsets"], pids[sel, :n], k, c["metric"],
                                                 num_threads=8)
    return wi, wd, pids


# ---- one parent, edited under a live context ---------------------------------------------------------------------------------
PARENT_CASE = case("ivf", 20000, 32, 60, 64, 10, "l2", 0.9, 0.5, seed=41)


def parent_steps():
    """The states of section d, each a dict: name, centroids + centroid_ids (the parent's rows, in a fixed non-identity order), vecs /
    ids / offsets (the CSR the oracle reads, laid out afresh), nlist_present, and what the step changes: `replaced` = (p, new
    centroid, ids and rows of list p), `removed` = the list deleted outright."""
    c = PARENT_CASE
    co = corpus(c)
    nlist, d = c["nlist"], c["d"]
    rng = np.random.default_rng(43)
    perm = rng.permutation(nlist).astype(np.int64)
    assert (perm != np.arange(nlist)).sum() > nlist // 2
    cent, offs = co["centroids"], co["offsets"]
    base = dict(centroids=np.ascontiguousarray(cent[perm]), centroid_ids=perm, vecs=co["vecs"], ids=co["ids"], offsets=offs,
                nlist_present=nlist, q=co["q"], d=d, nlist=nlist)
    steps = [dict(base, name="first")]
    # (ii) the centroid most queries rank first moves half way to its nearest neighbour, and its rows with it
    first, _ = O.coarse(co["q"], cent, None, 1, c["metric"])
    p = int(np.bincount(first[:, 0], minlength=nlist).argmax())
    d2 = ((cent - cent[p]) ** 2).sum(1)
    d2[p] = np.inf
    delta = (np.float32(0.5) * (cent[int(d2.argmin())] - cent[p])).astype(np.float32)
    cent2 = cent.copy()
    cent2[p] += delta
    vecs2 = co["vecs"].copy()
    lo, hi = int(offs[p]), int(offs[p + 1])
    vecs2[lo:hi] += delta
    moved = dict(base, centroids=np.ascontiguousarray(cent2[perm]), vecs=vecs2)
    steps.append(dict(moved, name="replaced", replaced=(p, cent2[p].copy(), co["ids"][lo:hi], vecs2[lo:hi].copy())))
    # (iii) a second parent of the same shape on the same context, then the first one again
    other = make_ivf(nlist, d, nlist, seed=44)["centroids"]
    perm2 = np.random.default_rng(45).permutation(nlist).astype(np.int64)
    steps.append(dict(moved, name="second parent", centroids=np.ascontiguousarray(other[perm2]), centroid_ids=perm2, second=True))
    steps.append(dict(moved, name="first parent again"))
    # (iv) one list and its centroid deleted outright: an empty CSR list without a centroid, one list fewer for M
    h = int(np.argsort(-np.bincount(first[:, 0], minlength=nlist), kind="stable")[1])   # (the next most popular first list)
    assert h != p
    keep = np.ones(offs[-1], bool)
    keep[int(offs[h]):int(offs[h + 1])] = False
    csum = np.zeros(keep.shape[0] + 1, np.int64)
    csum[1:] = np.cumsum(keep)
    rows = perm != h
    steps.append(dict(moved, name="list deleted", centroids=np.ascontiguousarray(cent2[perm][rows]), centroid_ids=perm[rows],
                      vecs=np.ascontiguousarray(vecs2[keep]), ids=np.ascontiguousarray(co["ids"][keep]), offsets=csum[offs],
                      nlist_present=nlist - 1, removed=h))
    return steps


def step_walk(st):
    c = PARENT_CASE
    return oracle_walk(c, st, centroid_ids=st["centroid_ids"], nlist_present=st["nlist_present"])
