"""The fp16 shadow form of the single-probe search (qk_ctx_set_shadow, quake_amd/csrc/qk_shadow.hip).

The form streams an fp16 mirror of the store, keeps the 32 best approximate keys per segment and finishes exactly in fp32; what it
reports must be the bits every other form reports.  Every case here runs it in forced mode, asserts that it answered (the label),
and compares ids and distance bits with the oracle's batched scan AND with the same call under mode 0.  So that the exact scan a
query falls back to cannot hide a broken fast path, the Gaussian and the integer corpora are fixed, seeded inputs on which a numpy
model of the rule -- top 32 by fp16-rounded keys, then the finish's verification -- passes for every query: the model is checked
on the host first, and the device must then report no fallback at all."""
import numpy as np
import pytest

import oracle as O
from helpers import make_ivf

pytestmark = pytest.mark.gpu

SHADOW = "k_scan (fp16 shadow)"
TILE = ("k_scan", "k_scan (query-sharing)")  # the static choice at one list per query: the tile form, query-sharing where lists are hot
SIZES = [1, 9, 15, 16, 17, 31, 32, 33, 64, 65, 700, 5000]  # rows per list: < k, around a record (32), around the seed sample (64), long
ID_BASE = 1 << 41


def corpus(d, seed, sizes=SIZES, scale=0.5, integer=False):
    """one list per entry of `sizes` around well separated centroids; ids above 2^40, shuffled"""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)
    if integer:
        cent = rng.integers(0, 40, size=(nlist, d)).astype(np.float32)
        parts = [cent[p] + rng.integers(-3, 4, size=(n, d)).astype(np.float32) for p, n in enumerate(sizes)]
    else:
        cent = (scale * rng.standard_normal((nlist, d))).astype(np.float32)
        parts = [(cent[p] + 0.3 * scale * rng.standard_normal((n, d))).astype(np.float32) for p, n in enumerate(sizes)]
    ids = rng.permutation(sum(sizes)).astype(np.int64) + ID_BASE
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    return dict(centroids=cent, vecs=np.ascontiguousarray(np.concatenate(parts, 0)), ids=ids, offsets=offsets, d=d, nlist=nlist,
                integer=integer, scale=scale)


def queries(ivf, per_list, seed):
    """per_list[p] queries next to list p's centroid (so they probe it)"""
    rng = np.random.default_rng(seed)
    out = []
    for p, n in enumerate(per_list):
        if ivf["integer"]:
            out.append(ivf["centroids"][p] + rng.integers(-2, 3, size=(n, ivf["d"])).astype(np.float32))
        else:
            out.append(ivf["centroids"][p] + (0.1 * ivf["scale"] * rng.standard_normal((n, ivf["d"]))).astype(np.float32))
    q = np.concatenate(out, 0).astype(np.float32)
    return np.ascontiguousarray(q[rng.permutation(q.shape[0])])


def stores(ctx, ivf):
    from quake_amd.capi import Store
    s = Store(ctx, ivf["d"])
    s.build_csr(ivf["offsets"], ivf["ids"], ivf["vecs"])
    parent = Store(ctx, ivf["d"])
    parent.build_csr(np.array([0, ivf["nlist"]], np.int64), np.arange(ivf["nlist"], dtype=np.int64), ivf["centroids"])
    return parent, s


def same_bits(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32), err_msg=what + ": distances")


def check(ctx, parent, s, ivf, q, k, metric, label=SHADOW, oracle=True):
    """forced mode against mode 0 and the oracle; returns the counters' change"""
    before = ctx.shadow_stats()
    ctx.set_shadow(2)
    got = ctx.search(parent, s, q, 1, k, metric)
    assert ctx.last_scan_kernel() == label
    ctx.set_shadow(0)
    ref = ctx.search(parent, s, q, 1, k, metric)
    assert ctx.last_scan_kernel() != SHADOW
    ctx.set_shadow(2)
    same_bits(got, ref, "shadow form against mode 0")
    if oracle:
        oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, k, metric, batched_scan=True)
        same_bits(got, (oi, od), "shadow form against the oracle")
    after = ctx.shadow_stats()
    return {key: after[key] - before[key] for key in after}


# ---- the rule on the host ------------------------------------------------------------------------------------------------------------
def _h_dist(a):
    h = a.astype(np.float16).astype(np.float64)
    e = np.abs(a.astype(np.float64) - h)
    e = np.where((h != 0) & (np.abs(h) < 2.0 ** -14), np.maximum(e, np.abs(a.astype(np.float64))), e)
    return h, np.sqrt((e * e).sum(-1))


def model_passes(ivf, q, k, metric):
    """per query: does the finish's verification hold when ONE record keeps the 32 smallest approximate keys of the whole list?
    (The device cuts a list into segments that keep 32 each: every full record's last key is then at least the list's 32nd, so a
    query that passes here passes there.)  The bound is taken 1 % wider than the host function gives it."""
    import ctypes as C
    from quake_amd import _lib
    lib = _lib.load()
    code = {"ip": _lib.QK_METRIC_IP, "l2": _lib.QK_METRIC_L2}[metric]
    xh, xe = _h_dist(ivf["vecs"])
    rho, xmax = float(xe.max()) * 1.002, float(np.sqrt((xh * xh).sum(-1)).max()) * 1.002
    qh, qe = _h_dist(q)
    pid, _ = O.coarse(q, ivf["centroids"], None, 1, metric)
    ok = np.ones(q.shape[0], bool)
    for i in range(q.shape[0]):
        lo, hi = ivf["offsets"][pid[i, 0]], ivf["offsets"][pid[i, 0] + 1]
        if hi - lo <= 32:
            continue  # no full record: nothing was dropped
        rows = ivf["vecs"][lo:hi]
        exact = O.pair_values(q[i:i + 1], rows, metric)[0].astype(np.float64)
        dot = (xh[lo:hi] @ qh[i]).astype(np.float32).astype(np.float64)
        if metric == "l2":
            xn = float(O.row_norms(q[i:i + 1])[0])
            approx = np.maximum(np.float32(xn) + O.row_norms(rows) - 2.0 * dot, 0.0)
        else:
            approx, exact = -dot, -exact
        E = 1.01 * float(lib.qk_shadow_error_bound(code, q.shape[1], C.c_float(float(np.linalg.norm(q[i].astype(np.float64))) * 1.002),
                                                   C.c_float(float(qe[i]) * 1.002), C.c_float(rho), C.c_float(xmax)))
        order = np.argsort(approx, kind="stable")[:32]
        a_k = approx[order[k - 1]]
        cand = order[approx[order] <= a_k + 2 * E]
        tau = np.sort(exact[cand])[k - 1]
        ok[i] = approx[order[31]] > tau + E
    return ok


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric,k,squared", [(128, "l2", 10, False), (16, "l2", 1, False), (48, "ip", 16, False), (256, "l2", 10, True)])
@pytest.mark.parametrize("Q", [1, 17, 1100])
def test_gaussian_lists_of_every_size(d, metric, k, squared, Q):
    from quake_amd.capi import Context
    ivf = corpus(d, seed=100 + d)
    # every list is probed; list 10 (700 rows) by 1, 16, 17 or 40 queries depending on the batch, the long list by the rest
    if Q == 1:
        per = [0] * 10 + [1, 0]
    elif Q == 17:
        per = [1] * 10 + [0, 7]
    else:
        per = [16, 17, 40, 1, 16, 17, 40, 16, 17, 40, 40, 0]
        per[11] = Q - sum(per)
    q = queries(ivf, per, seed=7 * d + Q)
    assert q.shape[0] == Q
    assert model_passes(ivf, q, k, metric).all(), "the fixed inputs must pass the rule's model on the host"
    ctx = Context(0)
    if squared:
        ctx.set_squared_l2(True)
    parent, s = stores(ctx, ivf)
    ctx.set_shadow(2)
    got = ctx.search(parent, s, q, 1, k, metric)
    assert ctx.last_scan_kernel() == SHADOW
    st = ctx.shadow_stats()
    ctx.set_shadow(0)
    ref = ctx.search(parent, s, q, 1, k, metric)
    assert ctx.last_scan_kernel() != SHADOW
    same_bits(got, ref, "shadow form against mode 0")
    if not squared:  # (the oracle reports the square root; mode 0 is the reference for squared distances)
        oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, k, metric, batched_scan=True)
        same_bits(got, (oi, od), "shadow form against the oracle")
    assert st["fallback"] == 0 and st["verified"] == Q and st["candidates"] >= min(k, 1), st
    assert got[0].max() >= ID_BASE
    info = s.shadow_info()
    assert info["valid"] and info["builds"] == 1 and info["bytes"] > 0 and s.device_bytes() > info["bytes"]
    s.close(); parent.close(); ctx.close()


def test_integer_rows_tie_and_order_by_id():
    from quake_amd.capi import Context
    ivf = corpus(64, seed=31, sizes=[500, 40, 800, 33, 1200, 64, 300, 20], integer=True)
    q = queries(ivf, [30, 3, 30, 3, 30, 3, 30, 3], seed=32)
    assert model_passes(ivf, q, 10, "l2").all()
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    st = check(ctx, parent, s, ivf, q, 10, "l2")
    assert st["fallback"] == 0 and st["verified"] == q.shape[0], st
    s.close(); parent.close(); ctx.close()


def test_identical_rows_fall_back_to_the_exact_scan():
    from quake_amd.capi import Context
    # list 0: copies of one row, and enough of them that a wave's segment holds more than 32 (the persistent grid cuts a short
    # list into one-tile segments, whose records are never full): every record is full, its last key equals the k-th, nothing is proved
    ivf = corpus(32, seed=41, sizes=[60000, 50])
    ivf["vecs"][:60000] = ivf["vecs"][0]
    q = queries(ivf, [9, 4], seed=42)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    st = check(ctx, parent, s, ivf, q, 10, "l2")
    assert st["fallback"] >= 9, st
    # every row of the list ties with the seed's bound, so every segment of the list -- a few tiles each, thousands of them --
    # leaves a record for each of the nine queries: far more than the 31 a slot line lists, the finish walks the record chain
    assert st["chained"] >= 9, st
    s.close(); parent.close(); ctx.close()


@pytest.mark.parametrize("rows", [20, 40])
def test_keys_one_ulp_apart_with_equal_images(rows):
    from quake_amd.capi import Context
    ivf = corpus(32, seed=51, sizes=[rows, 50])
    base = ivf["vecs"][0].copy()
    for j in range(rows):  # differences far below the fp16 resolution: one image, exact keys a few ulps apart
        ivf["vecs"][j] = base
        ivf["vecs"][j, j % 32] = np.nextafter(base[j % 32], np.float32(np.inf) if j % 2 else np.float32(-np.inf))
    q = queries(ivf, [6, 2], seed=52)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    check(ctx, parent, s, ivf, q, 10, "l2")
    check(ctx, parent, s, ivf, q, 16, "ip")
    s.close(); parent.close(); ctx.close()


def test_values_near_the_top_of_the_fp16_range():
    from quake_amd.capi import Context
    rng = np.random.default_rng(61)
    ivf = corpus(16, seed=62, sizes=[200, 90])
    ivf["vecs"][:] = (rng.uniform(5.0e4, 6.5e4, size=ivf["vecs"].shape) * rng.choice([-1.0, 1.0], size=ivf["vecs"].shape)).astype(np.float32)
    ivf["centroids"][0], ivf["centroids"][1] = ivf["vecs"][:200].mean(0), ivf["vecs"][200:].mean(0)
    q = (ivf["vecs"][rng.integers(0, 290, 24)] + rng.uniform(-300, 300, size=(24, 16))).astype(np.float32).clip(-65000, 65000)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    check(ctx, parent, s, ivf, q, 10, "l2")
    assert s.shadow_info()["valid"]
    s.close(); parent.close(); ctx.close()


@pytest.mark.parametrize("bad", [65520.0, float("nan"), float("inf")])
def test_a_store_outside_the_range_has_no_shadow(bad):
    from quake_amd.capi import Context
    ivf = corpus(32, seed=71, sizes=[300, 50, 64])
    ivf["vecs"][310, 5] = bad  # one value of list 1
    q = queries(ivf, [20, 0, 12], seed=72)  # (queries that do not probe the list with the value: finite answers)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    ctx.set_shadow(2)
    got = ctx.search(parent, s, q, 1, 10, "l2")
    assert ctx.last_scan_kernel() in TILE
    info = s.shadow_info()
    assert not info["valid"] and info["builds"] == 0 and info["bytes"] == 0
    ctx.set_shadow(0)
    same_bits(got, ctx.search(parent, s, q, 1, 10, "l2"), "no shadow: the tile form's answer")
    s.close(); parent.close(); ctx.close()


def test_queries_outside_the_range_are_answered_exactly():
    from quake_amd.capi import Context
    ivf = corpus(48, seed=81)
    q = queries(ivf, [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 10, 10], seed=82)
    q[3, 7] = np.nan
    q[11, 0] = np.inf
    q[19, 40] = -np.inf
    q[25, 1] = 7.0e4   # finite, beyond the fp16 range
    q[31, 2] = -1.0e30
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    st = check(ctx, parent, s, ivf, q, 10, "l2", oracle=False)
    # the four queries with an infinite or too large value are answered by the exact scan of their list; the NaN query has no
    # nearest list at all (every key of the coarse step is NaN), so there is nothing to scan: it is neither verified nor a fallback
    assert st["fallback"] >= 4 and st["verified"] + st["fallback"] == q.shape[0] - 1, st
    check(ctx, parent, s, ivf, q, 10, "ip", oracle=False)
    s.close(); parent.close(); ctx.close()


def test_ineligible_calls_keep_their_form():
    from quake_amd.capi import Context
    ctx = Context(0)
    ctx.set_shadow(2)
    ivf = corpus(64, seed=91)
    parent, s = stores(ctx, ivf)
    q = queries(ivf, [100] * 11 + [40], seed=92)
    got = ctx.search(parent, s, q, 1, 17, "l2")  # k = 17
    assert ctx.last_scan_kernel() in TILE
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, 17, "l2", batched_scan=True)
    same_bits(got, (oi, od), "k = 17")
    ctx.search(parent, s, q, 2, 10, "l2")  # two lists per query
    assert ctx.last_scan_kernel() != SHADOW
    ctx.search(parent, s, q, 1, 16, "l2")
    assert ctx.last_scan_kernel() == SHADOW
    s.close(); parent.close()
    wide = corpus(272, seed=93, sizes=[64, 700])  # d = 272
    parent, s = stores(ctx, wide)
    q = queries(wide, [500, 600], seed=94)
    got = ctx.search(parent, s, q, 1, 10, "l2")
    assert ctx.last_scan_kernel() in TILE and not s.shadow_info()["valid"]
    oi, od = O.search(q, wide["centroids"], wide["vecs"], wide["ids"], wide["offsets"], 1, 10, "l2", batched_scan=True)
    same_bits(got, (oi, od), "d = 272")
    s.close(); parent.close(); ctx.close()


# ---- staleness -------------------------------------------------------------------------------------------------------------------------
def _snapshot(s, ivf):
    """the store's lists as the oracle's CSR arena"""
    lists = s.list_ids()
    nl = int(max(lists)) + 1 if len(lists) else 0
    pv, pi = [], []
    for p in range(nl):
        if p in set(int(v) for v in lists):
            v, i = s.get_list(p)
        else:
            v, i = np.zeros((0, ivf["d"]), np.float32), np.zeros(0, np.int64)
        pv.append(v)
        pi.append(i)
    return O.csr_from_partitions(pv, pi, ivf["d"])


def test_every_mutation_makes_the_shadow_stale():
    from quake_amd.capi import Context
    ctx = Context(0)
    ivf = corpus(32, seed=111, sizes=[300, 90, 40, 700, 64, 33])
    parent, s = stores(ctx, ivf)
    q = queries(ivf, [8, 8, 8, 8, 8, 8], seed=112)
    rng = np.random.default_rng(113)
    next_id = [ID_BASE + 10 ** 6]

    def near(p, n):  # n new rows next to list p's queries: they enter the answers
        ids = np.arange(next_id[0], next_id[0] + n, dtype=np.int64)
        next_id[0] += n
        return ids, (ivf["centroids"][p] + 0.01 * rng.standard_normal((n, 32))).astype(np.float32)

    def expect(builds, what):
        assert not s.shadow_info()["valid"], what + ": the shadow must be stale"
        ctx.set_shadow(0)
        ref = ctx.search(parent, s, q, 1, 10, "l2")
        vecs, ids, offsets = _snapshot(s, ivf)
        oi, od = O.search(q, ivf["centroids"], vecs, ids, offsets, 1, 10, "l2", batched_scan=True)
        same_bits(ref, (oi, od), what + ": mode 0 sees the change")
        ctx.set_shadow(2)
        got = ctx.search(parent, s, q, 1, 10, "l2")
        assert ctx.last_scan_kernel() == SHADOW, what
        same_bits(got, (oi, od), what + ": the rebuilt shadow sees the change")
        info = s.shadow_info()
        assert info["valid"] and info["builds"] == builds, (what, info)

    ctx.set_shadow(2)
    ctx.search(parent, s, q, 1, 10, "l2")
    assert s.shadow_info()["builds"] == 1
    s.add_entries(0, *near(0, 5))
    expect(2, "add_entries")
    i, v = near(1, 6)
    s.add_batch(i, v, np.full(6, 1, np.int64))
    expect(3, "add_batch")
    assert s.remove_ids(i[:3]) == 3
    expect(4, "remove_ids")
    s.remove_list(2)
    expect(5, "remove_list")
    s.add_list(2)
    s.add_entries(2, *near(2, 12))
    expect(6, "add_list")
    s.refine_lists(np.array([0, 3], np.int64), ivf["centroids"][[0, 3]], "l2", 0)
    expect(7, "refine_lists")
    # many removals from the long list, then growth: a list outgrows its extent and moves, and the abandoned extents are compacted
    c0 = s.counters()
    s.remove_ids(s.get_list_ids(3)[::2])
    expect(8, "remove half of a list")
    big = near(4, 3000)
    s.add_entries(4, *big)
    c1 = s.counters()
    moved = (c1["list_relocations"] - c0["list_relocations"]) + (c1["arena_compactions"] - c0["arena_compactions"]) + \
            (c1["arena_reallocations"] - c0["arena_reallocations"])
    assert moved >= 1 and c1["rows_copied"] > c0["rows_copied"], (c0, c1)  # (rows really changed their place in the arena)
    expect(9, "a list outgrows its extent")
    s.reset()
    assert s.shadow_info() == {"valid": False, "bytes": 0, "builds": 9}
    s.build_csr(ivf["offsets"], ivf["ids"], ivf["vecs"])
    expect(10, "reset + build_csr")
    s.shadow_drop()
    assert s.shadow_info()["bytes"] == 0
    ctx.search(parent, s, q, 1, 10, "l2")
    assert ctx.last_scan_kernel() == SHADOW and s.shadow_info()["builds"] == 11
    s.close(); parent.close(); ctx.close()


# ---- selection -------------------------------------------------------------------------------------------------------------------------
def test_the_feedback_selects_the_form_from_injected_figures():
    from quake_amd.capi import Context
    ivf = make_ivf(60000, 32, 64, seed=121)
    rng = np.random.default_rng(122)
    q = (ivf["x"][rng.integers(0, 60000, 1024)] + 0.05 * rng.standard_normal((1024, 32))).astype(np.float32)
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, 10, "l2", batched_scan=True)

    def run(ctx, parent, s, n):
        labels = []
        for _ in range(n):
            got = ctx.search(parent, s, q, 1, 10, "l2")
            ctx.synchronize()
            labels.append(ctx.last_scan_kernel())
            same_bits(got, (oi, od), labels[-1])
        return labels

    ctx = Context(0)
    ctx.set_form_feedback(True)
    ctx.set_shadow(1)
    parent, s = stores(ctx, ivf)
    # three figures injected, the fourth missing: not admissible, nothing is built
    ctx.set_form_times((1.0, 1.0, 1.0))
    assert set(run(ctx, parent, s, 6)) <= set(TILE) and s.shadow_info()["builds"] == 0
    # the fourth smaller: the shadow is built at the second call, measured twice, then chosen
    ctx.set_shadow_form_time(0.5)
    # (deterministic: call 1 sees the store for the first time; call 2 builds the shadow and opens the comparison with the static
    #  form, measured at calls 2 and 3; the shadow form is measured at calls 4 and 5 and is the winner from call 6 on)
    labels = run(ctx, parent, s, 12)
    assert all(l in TILE for l in labels[:3]) and labels[3:] == [SHADOW] * 9, labels
    assert s.shadow_info()["builds"] == 1
    # a store that changed: the static form at once, the shadow again only after 8 unchanged calls
    s.add_entries(0, np.array([ID_BASE], np.int64), ivf["centroids"][:1])
    vecs, ids, offsets = _snapshot(s, ivf)
    oi, od = O.search(q, ivf["centroids"], vecs, ids, offsets, 1, 10, "l2", batched_scan=True)
    labels = run(ctx, parent, s, 24)  # (the eighth unchanged call rebuilds; the figures of the shape are known: the winner at once)
    assert all(l in TILE for l in labels[:7]) and labels[7:] == [SHADOW] * 17 and s.shadow_info()["builds"] == 2, labels
    # feedback off: the static form whatever shadow exists
    ctx.set_form_feedback(False)
    assert set(run(ctx, parent, s, 3)) <= set(TILE) and s.shadow_info()["valid"]
    # the fourth larger, on a fresh context: measured, not chosen
    ctx2 = Context(0)
    ctx2.set_form_feedback(True)
    ctx2.set_shadow(1)
    ctx2.set_form_times((1.0, 1.0, 1.0))
    ctx2.set_shadow_form_time(2.0)
    # (static form at calls 1 and 2, the shadow form at calls 3 and 4 -- measured twice --, then the static form: the faster one)
    labels = run(ctx2, parent, s, 14)
    assert all(l in TILE for l in labels[:2]) and labels[2:4] == [SHADOW] * 2 and all(l in TILE for l in labels[4:]), labels
    # under 1024 queries the automatic mode does not consider the form
    ctx2.set_shadow_form_time(0.1)
    ctx2.search(parent, s, q[:512], 1, 10, "l2")
    assert ctx2.last_scan_kernel() != SHADOW
    ctx2.close()
    s.close(); parent.close(); ctx.close()


def test_two_contexts_share_a_shadow_right_after_the_build():
    import torch
    from quake_amd.capi import Context
    ivf = corpus(64, seed=131)
    q = queries(ivf, [3] * 10 + [20, 30], seed=132)
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, 10, "l2", batched_scan=True)
    a, b = Context(0), Context(0)
    side = torch.cuda.Stream()
    b.set_stream(side.cuda_stream)
    parent, s = stores(a, ivf)
    a.synchronize()
    a.set_shadow(2)
    b.set_shadow(2)
    # (the building call waits on the host for the conversion -- its scalars come back --, so the other stream needs no event: what
    #  this checks is that nothing else is missing between a build on one stream and the first use on another)
    got_a = a.search(parent, s, q, 1, 10, "l2")   # builds the shadow on a's stream
    got_b = b.search(parent, s, q, 1, 10, "l2")   # first use on another stream, nothing in between
    assert a.last_scan_kernel() == SHADOW and b.last_scan_kernel() == SHADOW and s.shadow_info()["builds"] == 1
    same_bits(got_a, (oi, od), "the building context")
    same_bits(got_b, (oi, od), "the other stream")
    b.close()
    s.close(); parent.close(); a.close()
