"""Facet counts over random tiny shapes: 40 seeded cases drawn by this file's own generator -- dimension, lists, queries, nprobe,
metric, radius quantile, filter kind, columns and n_values -- each compared for exact equality of all five outputs with
tests/facet_yardstick.py.  A failure prints the seed and the case."""
import numpy as np
import pytest
import torch

import facet_yardstick as FCY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

N_CASES = 40
NAMES = ("values", "counts", "distinct", "missing", "total")


def draw_case(seed):
    rng = np.random.default_rng(1000 + seed)
    d = int(rng.choice([1, 3, 16, 33, 100]))
    nlist = int(rng.integers(1, 13))
    sizes = rng.integers(0, 301, size=nlist).astype(np.int64)
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
    # small integers in low dimensions: equal distances are common, and the radius below is one of them
    vecs = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32) if d > 3 else rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    ids = (rng.permutation(4 * n)[:n]).astype(np.int64)
    Q = int(rng.choice([1, 2, 17, 65]))
    q = (vecs[rng.integers(0, n, size=Q)] + (0.1 * rng.standard_normal((Q, d)) if d > 3 else 0)).astype(np.float32)
    use_parent = bool(rng.random() < 0.7)
    nprobe = int(rng.integers(1, nlist + 1))
    n_cols = int(rng.integers(1, 5))
    cols = []
    for _ in range(n_cols):
        card = int(rng.choice([1, 3, max(2, int(np.sqrt(n))), n]))
        has = rng.random(n) < rng.choice([1.0, 0.8])
        base = rng.choice(np.array([np.iinfo(np.int64).min, -2, -1, 0, np.iinfo(np.int64).max - card - 1], np.int64))
        v = base + (np.arange(n, dtype=np.int64) if card == n else rng.integers(0, card, size=n))
        cols.append({int(i): int(x) for i, x in zip(ids[has], v[has])})
    fkind = str(rng.choice(["none", "none", "allow", "deny", "where", "in"]))
    return dict(seed=seed, d=d, nlist=nlist, sizes=sizes.tolist(), metric=metric, Q=Q, use_parent=use_parent, nprobe=nprobe, n_cols=n_cols,
                n_values=int(rng.choice([1, 2, 16, 255, 256])), quantile=float(rng.choice([0.0, 0.05, 0.5, 1.0])), fkind=fkind,
                offsets=offsets, cent=cent, vecs=np.ascontiguousarray(vecs), ids=ids, q=np.ascontiguousarray(q), cols=cols,
                fdraw=rng.random(n), device=bool(rng.random() < 0.5))


def describe(case):
    return {k: v for k, v in case.items() if k not in ("offsets", "cent", "vecs", "ids", "q", "cols", "fdraw")}


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
    metric, ids, offsets, vecs, q = case["metric"], case["ids"], case["offsets"], case["vecs"], case["q"]
    s = Store(ctx, case["d"])
    s.build_csr(offsets, ids, vecs)
    parent = None
    if case["use_parent"]:
        parent = Store(ctx, case["d"])
        parent.build_csr(np.array([0, case["nlist"]], np.int64), np.arange(case["nlist"], dtype=np.int64), case["cent"])
    attrs = []
    for col in case["cols"]:
        a = Attr(s)
        a.set(np.fromiter(col.keys(), np.int64, len(col)), np.fromiter(col.values(), np.int64, len(col)))
        attrs.append(a)
    # the filter and its allowed id set
    flt, allowed = None, None
    col0 = case["cols"][0]
    v0 = np.array([col0.get(int(i), 0) for i in ids], np.int64)
    has0 = np.array([int(i) in col0 for i in ids], bool)
    if case["fkind"] in ("allow", "deny"):
        S = ids[case["fdraw"] < 0.4]
        flt = Filter(s, S, case["fkind"])
        allowed = S if case["fkind"] == "allow" else ids[case["fdraw"] >= 0.4]
    elif case["fkind"] == "where":
        lo = int(np.sort(v0[has0])[has0.sum() // 2]) if has0.any() else 0   # (an element, not np.median: float64 cannot hold these)
        flt = Filter.where(s, [(attrs[0], "range", lo, int(np.iinfo(np.int64).max))])
        allowed = ids[has0 & (v0 >= lo)]
    elif case["fkind"] == "in":
        vs = np.unique(v0[has0])[::2]
        vs = vs if vs.shape[0] else np.array([12345], np.int64)
        flt = Filter.expr(s, [[(attrs[0], "in", vs)], [(attrs[0], "range", 1, 0)]])   # (the second term is the empty interval)
        allowed = ids[has0 & np.isin(v0, vs)]
    # the radius: a quantile of the distances the call can see (so boundary ties occur), or everything
    pids = RY.probed(q, case["cent"] if parent is not None else None, offsets, case["nprobe"], metric)
    pairs = RY.all_pairs(q, vecs, ids, offsets, pids, metric)
    dist = pairs[2][~np.isnan(pairs[2])]
    if case["quantile"] == 1.0 or dist.shape[0] == 0:
        radius = float("inf") if metric == "l2" else float("-inf")
    else:
        srt = np.sort(dist) if metric == "l2" else np.sort(dist)[::-1]
        radius = float(srt[min(dist.shape[0] - 1, int(case["quantile"] * dist.shape[0]))])
    hits = FCY.hits_scan(q, vecs, ids, offsets, pids, radius, metric, allowed)
    want = FCY.expected_cols(hits, case["cols"], case["n_values"])
    xq = torch.from_numpy(q).cuda() if case["device"] else q
    try:
        got = ctx.facet_search(parent, s, xq, case["nprobe"], radius, metric, attrs, n_values=case["n_values"], filter=flt)
        if case["device"]:
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
        for name, g, w in zip(NAMES, got, want):
            np.testing.assert_array_equal(g, w, err_msg=name)
    except Exception:
        print("seed", seed, "case", describe(case), "radius", radius)
        raise
    finally:
        if flt is not None:
            flt.close()
        for a in attrs:
            a.close()
        s.close()
        if parent is not None:
            parent.close()
