"""Multi-vector search on random shapes: 40 seeded draws of (d, lists, rows, T, k, metric, column, filter, radius, ragged tokens,
entry point, memory) against tests/maxsim_yardstick.py, bit for bit on every output.  No draw is excluded."""
import numpy as np
import pytest
import torch

import filter_yardstick as FY
import grouped_yardstick as GY
import maxsim_yardstick as MY

pytestmark = pytest.mark.gpu

SEEDS = list(range(7000, 7040))


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


def draw(seed):
    rng = np.random.default_rng(seed)
    d = int(rng.choice([8, 12, 16, 24, 32, 40, 64, 100, 128, 160]))
    nlist = int(rng.integers(1, 21))
    n = int(rng.choice([0, 1, 17, 300, 1000, 3000])) if rng.random() < 0.5 else int(rng.integers(0, 3001))
    T = int(rng.integers(1, 9))
    L = int(rng.integers(1, 7))
    k = int(rng.integers(1, 51))
    metric = "l2" if rng.random() < 0.5 else "ip"
    assign = np.sort(rng.integers(0, nlist, size=n)) if rng.random() < 0.7 else np.sort(rng.choice(nlist, size=n, p=_skew(rng, nlist)))
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    vecs = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ids = rng.permutation(max(n, 1) * 2)[:n].astype(np.int64)
    q3 = (cent[rng.integers(0, nlist, size=L * T)] + 0.5 * rng.standard_normal((L * T, d))).astype(np.float32).reshape(L, T, d)
    kind = int(rng.integers(0, 4))
    has = rng.random(n) < (1.0, 0.6, 0.95, 0.0)[kind]
    col_ids = ids[has]
    col_vals = (col_ids % 23 - 11, col_ids.copy(), rng.integers(-(1 << 63), (1 << 63) - 1, size=col_ids.shape[0], dtype=np.int64),
                col_ids)[kind].astype(np.int64)
    nprobe = int(rng.integers(1, nlist + 1))
    P = int(rng.integers(1, nlist + 1))
    pids = np.stack([rng.permutation(nlist)[:P] for _ in range(L * T)]).astype(np.int64)
    pids[rng.random(pids.shape) < 0.1] = -1
    return dict(d=d, nlist=nlist, n=n, T=T, L=L, k=k, metric=metric, offsets=offsets, cent=cent, vecs=vecs, ids=ids, q3=q3,
                col_ids=col_ids, col_vals=col_vals, nprobe=nprobe, pids=pids, search=bool(rng.random() < 0.5), device=bool(rng.random() < 0.5),
                filtered=bool(rng.random() < 0.5), with_radius=bool(rng.random() < 0.5), ragged=bool(rng.random() < 0.5),
                missing=float(rng.choice([0.0, -1.5, 3.0, 100.0])), rng=rng)


def _skew(rng, nlist):
    w = rng.random(nlist) ** 3 + 1e-3
    return w / w.sum()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_shape(ctx, seed):
    from quake_amd.capi import Attr, Filter, Store
    c = draw(seed)
    rng, metric, L, T = c["rng"], c["metric"], c["L"], c["T"]
    S = FY.draw_set(c["ids"], 0.5, rng) if c["filtered"] and c["n"] > 0 else None
    nt = [int(v) for v in rng.integers(0, T + 1, size=L)] if c["ragged"] else None
    pids = GY.probed(c["q3"].reshape(L * T, -1), c["cent"], c["offsets"], c["nprobe"], metric) if c["search"] else c["pids"]
    radius = None
    if c["with_radius"] and c["n"] > 0:
        _, _, val = GY.candidates(c["q3"].reshape(L * T, -1), c["vecs"], c["ids"], c["offsets"], pids, metric)
        if val.shape[0]:
            with np.errstate(invalid="ignore"):
                dist = np.sqrt(val) if metric == "l2" else val
            radius = float(np.quantile(dist, 0.2 if metric == "l2" else 0.8))
    want = MY.scan(c["q3"], c["vecs"], c["ids"], c["offsets"], pids, c["k"], metric, c["col_ids"], c["col_vals"], radius=radius, n_tokens=nt,
                   missing=c["missing"], S=S, mode="allow")
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    parent = Store(ctx, c["d"])
    parent.build_csr(np.array([0, c["nlist"]], np.int64), np.arange(c["nlist"], dtype=np.int64), c["cent"])
    a = Attr(s)
    if c["col_ids"].shape[0]:
        a.set(c["col_ids"], c["col_vals"])
    f = Filter(s, S, "allow") if S is not None else None
    try:
        r = radius if radius is not None else (float("inf") if metric == "l2" else float("-inf"))
        x = torch.from_numpy(c["q3"]).cuda() if c["device"] else c["q3"]
        if c["search"]:
            got = ctx.maxsim_search(parent, s, x, c["nprobe"], r, metric, a, c["k"], c["missing"], nt, f)
        else:
            got = ctx.maxsim_scan(s, x, torch.from_numpy(pids).cuda() if c["device"] else pids, r, metric, a, c["k"], c["missing"], nt, f)
        if c["device"]:
            torch.cuda.synchronize()   # (the context's stream is its own: device results are read behind a device-wide wait)
        got = [g.cpu().numpy() if torch.is_tensor(g) else g for g in got]
        MY.assert_equal(got, want, "seed %d %s" % (seed, {k: c[k] for k in ("d", "nlist", "n", "T", "L", "k", "metric", "search", "device")}))
    finally:
        if f is not None:
            f.close()
        a.close()
        s.close()
        parent.close()
