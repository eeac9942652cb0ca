"""Diversified search over random tiny shapes: 36 seeded cases drawn by this file's own generator -- dimension, lists, copies of
rows, queries, the list form (parent, every list, pids with -1), nprobe, metric, the distance domain, filter kind, fetch_k, k,
lambda, host or device buffers -- each compared for exact equality of ids, distance bits and ranks with
tests/diverse_yardstick.py, nothing left out.  A failure prints the seed and the case."""
import numpy as np
import pytest
import torch

import diverse_yardstick as DY
import range_yardstick as RY

pytestmark = pytest.mark.gpu

N_CASES = 36


def draw_case(seed):
    rng = np.random.default_rng(9500 + seed)
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
    dup = float(rng.choice([0.0, 0.2, 0.6]))
    ncopy = int(dup * n)
    if ncopy:       # exact copies of rows anywhere in the store, under their own ids
        dst, src = rng.permutation(n)[:ncopy], rng.integers(0, n, size=ncopy)
        vecs[dst] = vecs[src]
    ids = (rng.permutation(4 * n)[:n]).astype(np.int64)
    Q = int(rng.choice([1, 2, 17, 65]))
    q = (vecs[rng.integers(0, n, size=Q)] + 0.1 * rng.standard_normal((Q, d))).astype(np.float32)
    form = str(rng.choice(["parent", "parent", "flat", "pids"]))
    nprobe = int(rng.integers(1, nlist + 1))
    pids = None
    if form == "pids":
        P = int(rng.integers(1, nlist + 1))
        pids = np.stack([rng.permutation(nlist)[:P] for _ in range(Q)]).astype(np.int64)
        pids[rng.random(pids.shape) < 0.2] = -1
    C_ = int(rng.choice([1, 2, 5, 17, 64, 65, 100, 256]))
    k = int(rng.choice(sorted({v for v in (1, 2, min(10, C_), C_) if v <= C_})))
    return dict(seed=seed, d=d, nlist=nlist, sizes=sizes.tolist(), metric=metric, Q=Q, form=form, nprobe=nprobe, dup=dup, C=C_, k=k,
                lam=float(rng.choice([0.0, 0.1, 0.3, 0.5, 0.75, 1.0])), squared=bool(metric == "l2" and rng.random() < 0.3),
                fkind=str(rng.choice(["none", "none", "allow", "deny", "where"])), offsets=offsets, cent=cent,
                vecs=np.ascontiguousarray(vecs), ids=ids, q=np.ascontiguousarray(q), pids=pids, fdraw=rng.random(n),
                device=bool(rng.random() < 0.5))


def describe(case):
    return {k: v for k, v in case.items() if k not in ("offsets", "cent", "vecs", "ids", "q", "fdraw", "pids")}


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
    k, C_, lam = case["k"], case["C"], case["lam"]
    s = Store(ctx, case["d"])
    s.build_csr(offsets, ids, vecs)
    parent = None
    if case["form"] == "parent":
        parent = Store(ctx, case["d"])
        parent.build_csr(np.array([0, case["nlist"]], np.int64), np.arange(case["nlist"], dtype=np.int64), case["cent"])
    a, flt, allowed = None, None, None
    if case["fkind"] in ("allow", "deny"):
        S = ids[case["fdraw"] < 0.4]
        flt = Filter(s, S, case["fkind"])
        allowed = S if case["fkind"] == "allow" else ids[case["fdraw"] >= 0.4]
    elif case["fkind"] == "where":
        a = Attr(s)
        a.set(ids, ids % 7)
        flt = Filter.where(s, [(a, "range", 2, 5)])
        allowed = ids[(ids % 7 >= 2) & (ids % 7 <= 5)]
    if allowed is not None and allowed.shape[0] == 0:   # (a filter without candidates: nothing for the oracle to search)
        prep = [(np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros((0, 0), np.float32))] * case["Q"]
    else:
        # the lists of every query as pids, whatever the form: the coarse step of a search, every list, or the drawn rows
        pids = (RY.probed(q, case["cent"], offsets, case["nprobe"], metric) if case["form"] == "parent"
                else np.ascontiguousarray(np.broadcast_to(np.arange(case["nlist"], dtype=np.int64), (case["Q"], case["nlist"])))
                if case["form"] == "flat" else case["pids"])
        prep = DY.prepare(q, None, vecs, ids, offsets, None, C_, metric, S=allowed, mode="allow", pids=pids, squared=case["squared"])
    want = DY.expected_batch(prep, k, lam, metric)
    xq = torch.from_numpy(q).cuda() if case["device"] else q
    ctx.set_squared_l2(case["squared"])
    try:
        if case["form"] == "pids":
            xp = torch.from_numpy(case["pids"]).cuda() if case["device"] else case["pids"]
            got = ctx.diverse_scan(s, xq, xp, k, C_, lam, metric, filter=flt)
        else:
            got = ctx.diverse_search(parent, s, xq, case["nprobe"], k, C_, lam, metric, filter=flt)
        if case["device"]:
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
        for name, g, w in zip(DY.NAMES, got, want):
            if name == "dist":
                g, w = g.view(np.uint32), w.view(np.uint32)
            np.testing.assert_array_equal(g, w, err_msg=name)
    except Exception:
        print("seed", seed, "case", describe(case), "candidates per query", [p[0].shape[0] for p in prep])
        raise
    finally:
        ctx.set_squared_l2(False)
        if flt is not None:
            flt.close()
        if a is not None:
            a.close()
        s.close()
        if parent is not None:
            parent.close()
