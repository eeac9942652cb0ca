"""Facet statistics over random tiny shapes: 36 seeded cases drawn by this file's own generator -- dimension, lists, queries,
nprobe, metric, radius quantile, filter kind, 1-4 columns with random cardinalities and extremes, 0-255 random edges per column --
each compared for exact equality of all eight outputs with tests/facet_stats_yardstick.py.  A failure prints the seed and the case."""
import numpy as np
import pytest
import torch

import facet_stats_yardstick as FSY
import facet_yardstick as FCY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

N_CASES = 36
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def draw_case(seed):
    rng = np.random.default_rng(7000 + seed)
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
    n_cols = int(rng.integers(1, 5))
    cols, edges = [], []
    for _ in range(n_cols):
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
        cols.append({int(i): int(x) for i, x in zip(ids[has], v[has])})
        ne = int(rng.choice([0, 1, 2, 16, 100, 255]))
        if rng.random() < 0.5:  # edges among the values themselves, and next to them
            cand = {int(x) + int(o) for x in pool[:400] for o in (-1, 0, 1) if I64MIN <= int(x) + int(o) <= I64MAX}
        else:
            cand = {int(x) for x in rng.integers(I64MIN, I64MAX, size=300, endpoint=True)}
        cand = sorted(cand)
        pick = sorted(rng.choice(len(cand), size=min(ne, len(cand)), replace=False).tolist()) if ne else []
        edges.append([cand[i] for i in pick])
    fkind = str(rng.choice(["none", "none", "allow", "deny", "where"]))
    return dict(seed=seed, d=d, nlist=nlist, sizes=sizes.tolist(), metric=metric, Q=Q, use_parent=use_parent, nprobe=nprobe, n_cols=n_cols,
                n_edges=[len(e) for e in edges], quantile=float(rng.choice([0.0, 0.05, 0.5, 1.0])), fkind=fkind, offsets=offsets, cent=cent,
                vecs=np.ascontiguousarray(vecs), ids=ids, q=np.ascontiguousarray(q), cols=cols, edges=edges, fdraw=rng.random(n),
                device=bool(rng.random() < 0.5), no_edges=bool(rng.random() < 0.15))


def describe(case):
    return {k: v for k, v in case.items() if k not in ("offsets", "cent", "vecs", "ids", "q", "cols", "fdraw", "edges")}


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
        flt = Filter.where(s, [(attrs[0], "range", lo, int(I64MAX))])
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
    hits = FCY.hits_scan(q, vecs, ids, offsets, pids, radius, metric, allowed)
    edges = None if case["no_edges"] else case["edges"]
    want = FSY.expected_cols(hits, case["cols"], [[] for _ in case["cols"]] if edges is None else edges)
    xq = torch.from_numpy(q).cuda() if case["device"] else q
    try:
        got = ctx.facet_stats_search(parent, s, xq, case["nprobe"], radius, metric, attrs, edges=edges, filter=flt)
        if case["device"]:
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
        for name, g, w in zip(FSY.NAMES, got, want):
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
