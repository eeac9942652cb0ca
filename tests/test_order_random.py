"""Ordered search over random tiny shapes: 36 seeded cases drawn by this file's own generator -- dimension, lists, queries, nprobe,
metric, radius quantile, filter kind, a column of random cardinality and extremes, k, direction, missing policy -- each compared for
exact equality of ids, distance bits, values, count, missing and total with tests/order_yardstick.py.  A failure prints the seed and
the case."""
import numpy as np
import pytest
import torch

import order_yardstick as OY
import paging_yardstick as PY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

N_CASES = 36
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def draw_case(seed):
    rng = np.random.default_rng(9000 + seed)
    d = int(rng.choice([8, 16, 33, 96]))
    nlist = int(rng.integers(1, 13))
    sizes = rng.integers(0, 334, size=nlist).astype(np.int64)       # at most 12 * 333 < 4000 rows
    if rng.random() < 0.3:
        sizes[rng.integers(0, nlist)] = 0
    if sizes.sum() == 0:
        sizes[0] = 1 + int(rng.integers(0, 40))
    n = int(sizes.sum())
    metric = str(rng.choice(["l2", "ip"]))
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = np.repeat(np.arange(nlist), sizes)
    vecs = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ids = (rng.permutation(4 * n)[:n]).astype(np.int64)
    Q = int(rng.choice([1, 2, 17, 65]))
    q = (vecs[rng.integers(0, n, size=Q)] + 0.1 * rng.standard_normal((Q, d))).astype(np.float32)
    use_parent = bool(rng.random() < 0.7)
    nprobe = int(rng.integers(1, nlist + 1))
    card = int(rng.choice([2, 3, max(2, int(np.sqrt(n))), max(2, n)]))
    has = rng.random(n) < rng.choice([1.0, 0.8])
    kind = str(rng.choice(["low", "high", "zero", "full"]))
    if kind == "full":      # anywhere in int64, the extremes among them
        pool = rng.integers(I64MIN, I64MAX, size=card, endpoint=True).astype(np.int64)
        pool[:2] = [I64MIN, I64MAX]
    else:
        base = {"low": I64MIN, "high": I64MAX - card + 1, "zero": -(card // 2)}[kind]
        pool = (np.arange(card, dtype=np.int64) + np.int64(base)).astype(np.int64)
    v = pool[np.arange(n) % card] if card >= n else pool[rng.integers(0, card, size=n)]
    col = {int(i): int(x) for i, x in zip(ids[has], v[has])}
    fkind = str(rng.choice(["none", "none", "allow", "deny", "where"]))
    return dict(seed=seed, d=d, nlist=nlist, sizes=sizes.tolist(), metric=metric, Q=Q, use_parent=use_parent, nprobe=nprobe, card=card,
                kind=kind, quantile=float(rng.choice([0.0, 0.05, 0.5, 1.0])), fkind=fkind, k=int(rng.choice([1, 3, 64, 1000])),
                desc=bool(rng.random() < 0.5), missing_last=bool(rng.random() < 0.5), offsets=offsets, cent=cent,
                vecs=np.ascontiguousarray(vecs), ids=ids, q=np.ascontiguousarray(q), col=col, fdraw=rng.random(n),
                device=bool(rng.random() < 0.5))


def describe(case):
    return {k: v for k, v in case.items() if k not in ("offsets", "cent", "vecs", "ids", "q", "col", "fdraw")}


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_case(ctx, seed):
    from quake_amd.capi import Attr, Filter, Store
    case = draw_case(seed)
    metric, ids, offsets, vecs, q, col = case["metric"], case["ids"], case["offsets"], case["vecs"], case["q"], case["col"]
    s = Store(ctx, case["d"])
    s.build_csr(offsets, ids, vecs)
    parent = None
    if case["use_parent"]:
        parent = Store(ctx, case["d"])
        parent.build_csr(np.array([0, case["nlist"]], np.int64), np.arange(case["nlist"], dtype=np.int64), case["cent"])
    a = Attr(s)
    a.set(np.fromiter(col.keys(), np.int64, len(col)), np.fromiter(col.values(), np.int64, len(col)))
    flt, allowed = None, None
    v0 = np.array([col.get(int(i), 0) for i in ids], np.int64)
    has0 = np.array([int(i) in col for i in ids], bool)
    if case["fkind"] in ("allow", "deny"):
        S = ids[case["fdraw"] < 0.4]
        flt = Filter(s, S, case["fkind"])
        allowed = S if case["fkind"] == "allow" else ids[case["fdraw"] >= 0.4]
    elif case["fkind"] == "where":
        lo = int(np.sort(v0[has0])[has0.sum() // 2]) if has0.any() else 0   # (an element, not np.median: float64 cannot hold these)
        flt = Filter.where(s, [(a, "range", lo, int(I64MAX))])
        allowed = ids[has0 & (v0 >= lo)]
    # the radius: a quantile of the first query's distances (so boundary ties occur), or everything
    pids = RY.probed(q, case["cent"] if parent is not None else None, offsets, case["nprobe"], metric)
    pairs = RY.all_pairs(q, vecs, ids, offsets, pids, metric)
    dist = pairs[2][pairs[0][0]:pairs[0][1]]
    dist = dist[~np.isnan(dist)]
    if case["quantile"] == 1.0 or dist.shape[0] == 0:
        radius = float("inf") if metric == "l2" else float("-inf")
    else:
        srt = np.sort(dist) if metric == "l2" else np.sort(dist)[::-1]
        radius = float(srt[min(dist.shape[0] - 1, int(case["quantile"] * dist.shape[0]))])
    if allowed is not None and allowed.shape[0] == 0:   # (a filter without candidates: no hit)
        order = PY.Order([np.zeros(0, np.int64)] * case["Q"], [np.zeros(0, np.float32)] * case["Q"], [np.zeros(0, np.uint32)] * case["Q"], metric)
    else:
        order = PY.ordering(q, None, vecs, ids, offsets, None, metric, S=allowed, mode="allow", pids=pids)
    want = OY.expected(order, radius, col, case["k"], case["desc"], case["missing_last"])
    xq = torch.from_numpy(q).cuda() if case["device"] else q
    try:
        got = ctx.order_search(parent, s, xq, case["nprobe"], radius, metric, a, case["k"], case["desc"], case["missing_last"], filter=flt)
        if case["device"]:
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
        for name, g, w in zip(OY.NAMES, got, want):
            if name == "dist":
                g, w = g.view(np.uint32), w.view(np.uint32)
            np.testing.assert_array_equal(g, w, err_msg=name)
    except Exception:
        print("seed", seed, "case", describe(case), "radius", radius)
        raise
    finally:
        if flt is not None:
            flt.close()
        a.close()
        s.close()
        if parent is not None:
            parent.close()
