"""The ten entry points on the key-emission scan -- qk_range_search / _scan, qk_search_grouped_n / qk_scan_grouped_n, qk_facet_search /
_scan, qk_facet_stats_search / _scan, qk_order_search / _scan -- called through Context.lib, where they share their host protocol
(include/quake_hip.h).  What the suites of the five features reach only in part:
  1. a store without lists: the documented padding of every output, in host and device memory, with and without qk_timing;
  2. every optional output NULL in turn: the others unchanged, nothing written outside the documented extent (for range search
     the bytes behind min(cap, lims[Q]) with cap below, at and above the hit count);
  3. which refusal wins when a call has two faults, for every adjacent pair of the order
        handles < nprobe / pids list < metric < NaN radius < the call's own checks, in their order < NULL argument
        < what the front end and the filter refuse
     (between the last two lies the report of an overflow an earlier call left behind, which no call can plant from outside);
  4. Q == 0.
Expected values come from the yardsticks of the features and from the padding the header documents.  One index of 200 rows serves
the whole file.  No assertion reads a clock."""
import ctypes as C

import numpy as np
import pytest
import torch

import facet_stats_yardstick as FSY
import facet_yardstick as FCY
import grouped_members_yardstick as GMY
import order_yardstick as OY
import paging_yardstick as PY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
D, Q, NPROBE, K, M, NV = 8, 3, 3, 4, 2, 3
EDGES = [1, 3]                 # the histogram of facet statistics: 3 buckets
TAIL, SENT = 8, -7             # elements behind every output buffer, and what all of it holds before a call
PIPES = ("range", "grouped", "facet", "stats", "order")
FORMS = ("search", "scan")
ENTRY = {("range", "search"): "qk_range_search", ("range", "scan"): "qk_range_scan",
         ("grouped", "search"): "qk_search_grouped_n", ("grouped", "scan"): "qk_scan_grouped_n",
         ("facet", "search"): "qk_facet_search", ("facet", "scan"): "qk_facet_scan",
         ("stats", "search"): "qk_facet_stats_search", ("stats", "scan"): "qk_facet_stats_scan",
         ("order", "search"): "qk_order_search", ("order", "scan"): "qk_order_scan"}
# the name the messages of the call's body carry (the two grouped bodies speak as the entry points without _n)
WHO = {k: v.replace("_grouped_n", "_grouped") for k, v in ENTRY.items()}
REQUIRED = {"range": (0,), "grouped": (0,), "facet": (0, 1), "stats": (7,), "order": (0,)}   # outputs that must not be NULL
METRIC = {"ip": 0, "l2": 1}
F32 = np.float32


def shapes(pipe, nq, cap=0):
    """(shape, dtype) of every output of the call, in the order of its arguments"""
    i8 = np.int64
    return {"range": [((nq + 1,), i8), ((cap,), i8), ((cap,), F32)],
            "grouped": [((nq, K, M), i8), ((nq, K, M), F32), ((nq, K), i8)],
            "facet": [((1, nq, NV), i8), ((1, nq, NV), i8), ((1, nq), i8), ((1, nq), i8), ((nq,), i8)],
            "stats": [((1, nq), i8)] * 6 + [((1, nq, len(EDGES) + 1), i8), ((nq,), i8)],
            "order": [((nq, K), i8), ((nq, K), F32), ((nq, K), i8), ((nq,), i8), ((nq,), i8), ((nq,), i8)]}[pipe]


class Bufs:
    """the outputs of one call: flat buffers in host (mem 0) or device (mem 1) memory, TAIL elements longer than the output,
    all of it SENT; `null`: the outputs passed as NULL"""

    def __init__(self, pipe, nq, mem, cap=0, null=()):
        self.shp, self.mem, self.null = shapes(pipe, nq, cap), mem, set(null)
        self.flat = []
        for shape, dt in self.shp:
            n = int(np.prod(shape)) + TAIL
            self.flat.append(np.full(n, SENT, dt) if mem == 0 else
                             torch.full((n,), SENT, dtype=torch.float32 if dt == F32 else torch.int64, device="cuda"))
        if mem == 1:
            torch.cuda.synchronize()   # (the fills run on torch's stream, the call on the context's)

    def ptrs(self):
        return [None if j in self.null else _p(b) for j, b in enumerate(self.flat)]

    def read(self):
        """the outputs as numpy arrays of their shapes, behind the assertion that no tail was written"""
        if self.mem == 1:
            torch.cuda.synchronize()   # (a context's stream is its own: device results are read behind a device-wide wait)
        out = []
        for j, ((shape, dt), b) in enumerate(zip(self.shp, self.flat)):
            a = b if self.mem == 0 else b.cpu().numpy()
            n = int(np.prod(shape))
            assert (a[n:] == SENT).all(), "output %d: written behind its end" % j
            out.append(a[:n].reshape(shape))
        return out


def _p(a):
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


def _in(a, mem):
    return a if mem == 0 else torch.from_numpy(a).cuda()


def _same(got, want, tag):
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w, dtype=g.dtype).reshape(g.shape)
        if g.dtype == F32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg="output %d of %s" % (j, tag))


def _untouched(got, which, tag):
    for j in which:
        assert (got[j] == SENT).all(), "output %d of %s was written" % (j, tag)


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def env(ctx):
    """the index (6 lists: one empty, one of 5 rows, one of 7, 200 rows), its parent, a column over about 90 % of the ids, 3
    queries, the lists the coarse step ranks for them, a radius that about half of query 0's probed rows pass; a store without
    lists with a parent without rows; a second store whose column and filter are foreign to the first"""
    from quake_amd.capi import Attr, Filter, Store
    c = RY.corpus(D, 6, 200, "l2", seed=901, empty=1)
    sizes = np.diff(c["offsets"])
    assert sizes.tolist()[:3] == [0, 5, 7] and sizes.sum() == 200

    def store(offsets, ids, vecs):
        s = Store(ctx, D)
        s.build_csr(offsets, ids, vecs)
        return s

    s = store(c["offsets"], c["ids"], c["vecs"])
    parent = store(np.array([0, 6], np.int64), np.arange(6, dtype=np.int64), c["cent"])
    rng = np.random.default_rng(902)
    has = rng.random(200) < 0.9
    col = {int(i): int(i) % 5 for i in c["ids"][has]}
    assert 150 < len(col) < 200

    def attr(st, column):
        a = Attr(st)
        a.set(np.fromiter(column.keys(), np.int64, len(column)), np.fromiter(column.values(), np.int64, len(column)))
        return a

    q = RY.queries(c, Q, seed=903)
    e = dict(c=c, s=s, parent=parent, col=col, attr=attr(s, col), q=q, memo={})
    e["bare"], e["nobody"] = Store(ctx, D), Store(ctx, D)
    e["bare_attr"] = attr(e["bare"], {1: 1})
    e["other"] = store(c["offsets"], c["ids"], c["vecs"])
    e["other_attr"] = attr(e["other"], col)
    e["other_filter"] = Filter(e["other"], c["ids"][:50], "allow")
    for metric in ("l2", "ip"):
        pids = np.ascontiguousarray(RY.probed(q, c["cent"], c["offsets"], NPROBE, metric))
        assert pids.shape == (Q, NPROBE)
        dist0 = np.sort(RY.all_pairs(q[:1], c["vecs"], c["ids"], c["offsets"], pids[:1], metric)[2])
        e[metric] = dict(pids=pids, radius=float(dist0[dist0.shape[0] // 2]))
    yield e
    for k in ("attr", "bare_attr", "other_attr", "other_filter", "s", "parent", "bare", "nobody", "other"):
        e[k].close()


def want(env, pipe, metric):
    """the answer of the good call of `pipe` (both forms: the scan form names the lists the search form probes), computed once"""
    key = (pipe, metric)
    if key not in env["memo"]:
        c, q, col, r = env["c"], env["q"], env["col"], env[metric]["radius"]
        vecs, ids, offs, cent = c["vecs"], c["ids"], c["offsets"], c["cent"]
        if pipe == "range":
            w = RY.search(q, cent, vecs, ids, offs, NPROBE, r, metric)
        elif pipe == "grouped":
            w = GMY.search(q, cent, vecs, ids, offs, NPROBE, K, M, metric, np.fromiter(col.keys(), np.int64, len(col)),
                           np.fromiter(col.values(), np.int64, len(col)))
        elif pipe == "order":
            w = OY.expected(PY.ordering(q, cent, vecs, ids, offs, NPROBE, metric), r, col, K)
        else:
            hits = FCY.hits_search(q, cent, vecs, ids, offs, NPROBE, r, metric)
            w = FCY.expected_cols(hits, [col], NV) if pipe == "facet" else FSY.expected_cols(hits, [col], [EDGES])[:8]
        env["memo"][key] = tuple(np.asarray(a) for a in w)
    return env["memo"][key]


def args(env, pipe, name="l2", **over):
    """the arguments of the good call between the head (handles, x, Q, nprobe or pids) and the outputs, as a dict to override"""
    a = dict(metric=METRIC[name], radius=env[name]["radius"], filter=None, cap=0, k=K, m=M,
             col=env["attr"].h, n_cols=1, n_values=NV, edges=(C.c_int64 * len(EDGES))(*EDGES), n_edges=(C.c_int * 1)(len(EDGES)),
             flags=0, no_cols=False)
    a.update(over)
    return a


def call(ctx, env, pipe, form, a, out_ptrs, mem, s=None, parent=None, x=None, nq=Q, pids=None, P=NPROBE, nprobe=NPROBE, timing=None):
    """one call through Context.lib; returns (status, message).  x / pids: numpy arrays, moved to `mem`; `a`: args()"""
    x = env["q"][:nq] if x is None else x
    xm = _in(np.ascontiguousarray(x), mem) if x is not False else None
    head = [ctx.h]
    if form == "search":
        head += [parent, s, _p(xm), nq, nprobe]
    else:
        pm = _in(np.ascontiguousarray(pids), mem) if pids is not None else None
        head += [s, _p(xm), nq, _p(pm), P]
    harr = None if a["no_cols"] else (C.c_void_p * 4)(a["col"], a["col"], None, None)
    mid = {"range": [a["metric"], a["radius"], a["filter"], a["cap"]],
           "grouped": [a["k"], a["m"], a["metric"], a["col"], a["filter"]],
           "facet": [a["metric"], a["radius"], a["filter"], harr, a["n_cols"], a["n_values"]],
           "stats": [a["metric"], a["radius"], a["filter"], harr, a["n_cols"], a["edges"], a["n_edges"]],
           "order": [a["metric"], a["radius"], a["filter"], a["col"], a["flags"], a["k"]]}[pipe]
    st = getattr(ctx.lib, ENTRY[pipe, form])(*head, *mid, *out_ptrs, mem, C.byref(timing) if timing is not None else None)
    if mem == 1:
        torch.cuda.synchronize()   # (xm / pm stay alive until the call's work is done)
    return st, ctx.lib.qk_last_error().decode("utf-8", "replace") if st != 0 else ""


def good(ctx, env, pipe, form, mem, metric="l2", null=(), cap=None, timing=None):
    """the good call of the index; returns its Bufs"""
    if pipe == "range" and cap is None:
        cap = int(want(env, pipe, metric)[0][Q])
    b = Bufs(pipe, Q, mem, cap or 0, null)
    st, msg = call(ctx, env, pipe, form, args(env, pipe, metric, cap=cap or 0), b.ptrs(), mem, s=env["s"].h, parent=env["parent"].h,
                   pids=env[metric]["pids"], timing=timing)
    assert st == 0, msg
    return b


# ---- 0. the good call answers what the yardsticks say, in both forms and memories ---------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("pipe", PIPES)
def test_good_call(ctx, env, pipe, metric):
    w = want(env, pipe, metric)
    if pipe == "range":
        assert 0 < w[0][Q] < 200 * Q and (np.diff(w[0]) > 0).sum() >= 2     # some rows are hits, not all
    for form in FORMS:
        for mem in (0, 1):
            _same(good(ctx, env, pipe, form, mem, metric).read(), w, (pipe, form, mem, metric))
            assert ctx.last_scan_kernel() == "k_scan (%s)" % {"stats": "facet stats"}.get(pipe, pipe)


# ---- 1. no lists ------------------------------------------------------------------------------------------------------------------------
def padding(pipe, metric, nq):
    worst = -np.inf if metric == "ip" else np.inf
    z = lambda *shape: np.zeros(shape, np.int64)  # noqa: E731
    return {"range": [z(nq + 1)],
            "grouped": [np.full((nq, K, M), -1), np.full((nq, K, M), worst, F32), z(nq, K)],
            "facet": [z(1, nq, NV), z(1, nq, NV), z(1, nq), z(1, nq), z(nq)],
            "stats": [z(1, nq), z(1, nq), np.full((1, nq), I64MAX), np.full((1, nq), I64MIN), z(1, nq), z(1, nq), z(1, nq, 3), z(nq)],
            "order": [np.full((nq, K), -1), np.full((nq, K), worst, F32), z(nq, K), z(nq), z(nq), z(nq)]}[pipe]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("pipe", PIPES)
def test_no_lists(ctx, env, pipe, metric):
    from quake_amd._lib import QkTiming
    bare, nobody = env["bare"], env["nobody"]
    absent = np.array([[0, 3]] * Q, np.int64)
    # a store without lists: every list (no parent), what a parent without rows ranks, lists the store does not have
    ways = (("search", dict(parent=None)), ("search", dict(parent=nobody.h)), ("scan", dict(pids=absent, P=2)))
    pad = padding(pipe, metric, Q)
    a = args(env, pipe, metric, col=env["bare_attr"].h, cap=5)
    for form, kw in ways:
        for mem in (0, 1):
            for timed in (False, True):
                tag = (pipe, metric, form, sorted(kw), mem, timed)
                b = Bufs(pipe, Q, mem, cap=5)
                t = QkTiming()
                t.n_items = t.partitions_scanned = t.scan_bytes = SENT
                ctx.set_timing(1 if timed else 0)
                try:
                    st, msg = call(ctx, env, pipe, form, a, b.ptrs(), mem, s=bare.h, timing=t if timed else None, **kw)
                finally:
                    ctx.set_timing(0)
                assert st == 0, (tag, msg)
                got = b.read()
                _same(got[:len(pad)], pad, tag)
                _untouched(got, range(len(pad), len(got)), tag)              # (range search: no hit, nothing behind lims)
                if timed:
                    assert (t.n_items, t.partitions_scanned, t.scan_bytes) == (0, 0, 0), tag


# ---- 2. optional outputs; the extent of what is written -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["facet", "stats", "order"])
def test_optional_outputs(ctx, env, pipe):
    w = want(env, pipe, "l2")
    optional = [j for j in range(len(w)) if j not in REQUIRED[pipe]]
    assert len(optional) == {"facet": 3, "stats": 7, "order": 5}[pipe]
    for form in FORMS:
        for mem in (0, 1):
            for j in optional:
                got = good(ctx, env, pipe, form, mem, null=(j,)).read()
                rest = [i for i in range(len(w)) if i != j]
                _same([got[i] for i in rest], [w[i] for i in rest], (pipe, form, mem, "without", j))
                _untouched(got, (j,), (pipe, form, mem))
            everything = good(ctx, env, pipe, form, mem, null=optional).read()    # ... and all of them at once
            _same([everything[i] for i in REQUIRED[pipe]], [w[i] for i in REQUIRED[pipe]], (pipe, form, mem, "required only"))
            _untouched(everything, optional, (pipe, form, mem))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_range_prefix(ctx, env, metric):
    lims, ids, dist = want(env, "range", metric)
    total = int(lims[Q])
    assert total > 8
    for form in FORMS:
        for mem in (0, 1):
            for cap in (0, 1, total - 5, total, total + 9):
                n = min(cap, total)
                for no_dist in (False, True):
                    tag = (metric, form, mem, cap, no_dist)
                    got = good(ctx, env, "range", form, mem, metric, null=(2,) if no_dist else (), cap=cap).read()
                    np.testing.assert_array_equal(got[0], lims, err_msg=str(tag))           # exact whatever cap is
                    _same([got[1][:n]], [ids[:n]], tag)
                    assert (got[1][n:] == SENT).all(), tag                                  # nothing behind the prefix
                    if no_dist:
                        _untouched(got, (2,), tag)
                    else:
                        _same([got[2][:n]], [dist[:n]], tag)
                        assert (got[2][n:] == SENT).all(), tag
    # cap == 0 counts: the id and distance buffers may be NULL
    for mem in (0, 1):
        got = good(ctx, env, "range", "search", mem, metric, null=(1, 2), cap=0).read()
        np.testing.assert_array_equal(got[0], lims)


# ---- 3. which refusal wins ---------------------------------------------------------------------------------------------------------------
def own_checks(env, pipe):
    """the faults the body of `pipe` refuses itself, in the order of its checks: (override of args(), NULL outputs, message)"""
    foreign, neg = env["other_attr"].h, (C.c_int * 1)(-1)
    bad_edges = (C.c_int64 * 2)(3, 3)
    return {"range": [(dict(cap=-1), (), "cap must not be negative"), (dict(), (0,), "out_lims is null"),
                      (dict(), (1,), "cap > 0 needs an id buffer")],     # (the calls below have cap = 4)
            "grouped": [(dict(col=None), (), "the group-by column is null"), (dict(col=foreign), (), "the group-by column belongs to another store"),
                        (dict(k=0), (), "k=0 must be at least 1"), (dict(k=8193), (), "k=8193 exceeds 8192"),
                        (dict(m=0), (), "group_size=0 must be at least 1"), (dict(m=17), (), "group_size=17 exceeds QK_MAX_GROUP_SIZE")],
            "facet": [(dict(n_cols=0), (), "n_cols=0 must be at least 1"), (dict(n_cols=5), (), "n_cols=5 exceeds QK_MAX_FACET_COLS"),
                      (dict(n_values=0), (), "n_values=0 must be at least 1"), (dict(n_values=10 ** 6), (), "n_values=1000000 exceeds QK_MAX_FACET_VALUES"),
                      (dict(no_cols=True), (), "facet_by is null"), (dict(col=None), (), "facet column 0 is null"),
                      (dict(col=foreign), (), "facet column 0 belongs to another store")],
            "stats": [(dict(n_cols=0), (), "n_cols=0 must be at least 1"), (dict(n_cols=5), (), "n_cols=5 exceeds QK_MAX_FACET_COLS"),
                      (dict(no_cols=True), (), "facet_by is null"), (dict(col=None), (), "facet column 0 is null"),
                      (dict(col=foreign), (), "facet column 0 belongs to another store"), (dict(n_edges=None), (), "edges without n_edges"),
                      (dict(n_edges=neg), (), r"n_edges\[0\]=-1 is negative"), (dict(edges=bad_edges), (), "the edges of column 0 are not strictly ascending")],
            "order": [(dict(k=0), (), "k=0 must be at least 1"), (dict(k=1025), (), "k=1025 exceeds QK_MAX_ORDER_K"),
                      (dict(flags=4), (), "unknown flags 4"), (dict(col=None), (), "order_by is null"),
                      (dict(col=foreign), (), "the order column belongs to another store")]}[pipe]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pipe", PIPES)
def test_precedence(ctx, env, pipe, form):
    import re
    who = WHO[pipe, form]
    s, parent = env["s"].h, env["parent"].h
    pids = env["l2"]["pids"]
    own = own_checks(env, pipe)
    # the steps of the order as (overrides of args(), NULL outputs, keywords of call(), message); a pair of neighbours makes a call
    bad_list = (dict(nprobe=0), "%s: nprobe must be positive" % who) if form == "search" else (dict(P=0), "%s: bad partition id list" % who)
    steps = [((), (), dict(s=None), "%s: null argument" % who), ((), (), bad_list[0], bad_list[1]),
             (dict(metric=7), (), {}, "Metric type not supported")]
    if pipe != "grouped":
        steps.append((dict(radius=float("nan")), (), {}, "%s: the radius is NaN" % who))
    steps += [(o, null, {}, "%s: %s" % (who, msg)) for o, null, msg in own]
    steps.append(((), REQUIRED[pipe] if pipe != "range" else (), dict(x=False), "%s: null argument" % who))
    steps.append((dict(filter=env["other_filter"].h), (), {}, "another store"))
    for mem in (0, 1):
        for first, second in zip(steps, steps[1:]):
            if any(k in dict(second[0]) and dict(second[0])[k] != v for k, v in dict(first[0]).items()):
                continue                               # (two values of one argument: no call has both faults)
            over = dict(second[0])
            over.update(first[0])
            kw = dict(s=s, parent=parent, pids=pids)
            kw.update(second[2])
            kw.update(first[2])
            cap = over.get("cap", 4 if pipe == "range" else 0)
            b = Bufs(pipe, Q, mem, cap=max(cap, 0), null=set(first[1]) | set(second[1]))
            st, msg = call(ctx, env, pipe, form, args(env, pipe, "l2", **dict(over, cap=cap)), b.ptrs(), mem, **kw)
            assert st != 0 and re.search(first[3], msg), (pipe, form, mem, first[3], "before", second[3], "got", msg)
            got = b.read()
            _untouched(got, range(len(got)), (pipe, form, mem, first[3]))
        # ... and every step alone is refused with its own message
        for over, null, kwx, text in steps:
            kw = dict(s=s, parent=parent, pids=pids)
            kw.update(kwx)
            cap = dict(over).get("cap", 4 if pipe == "range" else 0)
            b = Bufs(pipe, Q, mem, cap=max(cap, 0), null=null)
            st, msg = call(ctx, env, pipe, form, args(env, pipe, "l2", **dict(over, cap=cap)), b.ptrs(), mem, **kw)
            assert st != 0 and re.search(text, msg), (pipe, form, mem, text, "got", msg)
        # the context still answers, and answers the same
        _same(good(ctx, env, pipe, form, mem).read(), want(env, pipe, "l2"), (pipe, form, mem, "after the refusals"))


# ---- 4. Q == 0 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES)
def test_no_queries(ctx, env, pipe):
    for form in FORMS:
        for mem in (0, 1):
            b = Bufs(pipe, 0, mem, cap=4)
            st, msg = call(ctx, env, pipe, form, args(env, pipe, "l2", cap=4), b.ptrs(), mem, s=env["s"].h, parent=env["parent"].h,
                           nq=0, pids=env["l2"]["pids"])
            assert st == 0, (pipe, form, mem, msg)
            got = b.read()
            if pipe == "range":
                assert got[0].tolist() == [0]
            _untouched(got, range(1 if pipe == "range" else 0, len(got)), (pipe, form, mem, "Q == 0"))
