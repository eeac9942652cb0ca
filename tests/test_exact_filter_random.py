"""Seeded sweep of exact filtered search (qk_search_filtered_exact): random list sizes, dimensions, filters, k and batch sizes,
every answer bit for bit the yardstick's (tests/exact_filter_yardstick.py) and, for k <= QK_MAX_K, the all-lists route's
qk_search_filtered(parent = NULL).  A seed is a case: a failure names it."""
import numpy as np
import pytest
import torch

import exact_filter_yardstick as E
import filter_yardstick as Y
from test_filtered_search import _eq, _np

pytestmark = pytest.mark.gpu

QK_MAX_K = 448
SEEDS = list(range(36))


def _case(seed):
    rng = np.random.default_rng(9000 + seed)
    d = int(rng.choice([3, 8, 16, 20, 33, 64, 100, 128, 200]))
    metric = "l2" if rng.random() < 0.5 else "ip"
    nlist = int(rng.integers(1, 40))
    sizes = np.where(rng.random(nlist) < 0.2, 0, rng.integers(1, int(rng.choice([20, 300, 3000])), size=nlist)).astype(np.int64)
    sizes[int(rng.integers(0, nlist))] += int(rng.integers(1, 50))  # never an empty store: that case has a test of its own
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    if rng.random() < 0.3:
        vecs = np.round(vecs)  # ties
    ids = rng.permutation(4 * n)[:n].astype(np.int64) + (int(rng.choice([0, 1 << 33])) if rng.random() < 0.3 else 0)
    Q = int(rng.choice([1, 2, 16, 17, 47, 130]))
    q = rng.standard_normal((Q, d)).astype(np.float32)
    k = int(rng.choice([1, 2, 10, 64, 65, 100, 448, 449, 1000, 3000]))
    kind = str(rng.choice(["allow", "deny", "range"]))
    sel = float(rng.choice([0, 0.003, 0.05, 0.5, 1]))
    if kind == "range":
        lo = int(np.quantile(ids, rng.random() * 0.8))
        S, mode = np.arange(lo, lo + max(1, int(sel * 4 * n)), dtype=np.int64), "allow"
    else:
        S, mode = Y.draw_set(ids, sel, rng), kind
    return dict(d=d, metric=metric, vecs=vecs, ids=ids, offsets=offsets, q=q, k=k, S=S, mode=mode,
                device=bool(rng.random() < 0.5), tag="d%d-%s-n%d-Q%d-k%d-%s%g" % (d, metric, n, Q, k, kind, sel))


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_case(ctx, seed):
    from quake_amd.capi import Filter, Store
    c = _case(seed)
    s = Store(ctx, c["d"])
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    f = Filter(s, c["S"], c["mode"])
    x = torch.from_numpy(c["q"]).cuda() if c["device"] else c["q"]
    oi, od = E.search(c["q"], c["vecs"], c["ids"], c["offsets"], c["k"], c["metric"], c["S"], c["mode"])
    for call in range(2):
        gi, gd = ctx.search_exact(s, x, c["k"], c["metric"], f)
        ctx.synchronize()  # (device buffers are complete behind the context's stream)
        _eq(gi, gd, oi, od, (seed, c["tag"], call))
    assert f.exact_info()["builds"] == 1 and f.exact_info()["rows"] == E.candidates(c["ids"], c["S"], c["mode"])
    if c["k"] <= QK_MAX_K:
        ai, ad = ctx.search(None, s, x, 1, c["k"], c["metric"], filter=f)
        ctx.synchronize()
        _eq(gi, gd, _np(ai), _np(ad), (seed, c["tag"], "all lists"))
    f.close()
    s.close()
