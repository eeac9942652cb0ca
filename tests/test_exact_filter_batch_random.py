"""Seeded sweep of exact filtered search with one filter per query (qk_search_filtered_exact_batch): random list sizes,
dimensions, filter families (id sets, deny sets, predicates, empty ones), k and batch sizes; several calls per store with random
subsets of the filters, rows added and removed in between, under a random pool_rows that forces evictions.  Every answer is bit
for bit the yardstick's (tests/exact_filter_batch_yardstick.py) on the store's contents of that moment, and the pool stays within
its budget.  A seed is a case: a failure names it."""
import numpy as np
import pytest
import torch

import attr_yardstick as AY
import exact_filter_batch_yardstick as B
import filter_yardstick as Y
import oracle as O
from test_filtered_search import _eq, _np

pytestmark = pytest.mark.gpu

SEEDS = list(range(40))


def _r16(n):
    return (int(n) + 15) // 16 * 16


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


def _csr_of(s, d):
    lists = sorted(int(p) for p in s.list_ids())
    pv, pi = zip(*[s.get_list(p) for p in lists])
    return O.csr_from_partitions(pv, pi, d)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_case(ctx, seed):
    from quake_amd.capi import Attr, Filter, Store
    rng = np.random.default_rng(12000 + seed)
    d = int(rng.choice([3, 8, 16, 20, 33, 64, 100, 128, 160]))
    metric = "l2" if rng.random() < 0.5 else "ip"
    nlist = int(rng.integers(1, 30))
    sizes = np.where(rng.random(nlist) < 0.2, 0, rng.integers(1, int(rng.choice([20, 300, 1500])), size=nlist)).astype(np.int64)
    sizes[int(rng.integers(0, nlist))] += int(rng.integers(1, 50))
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    if rng.random() < 0.3:
        vecs = np.round(vecs)  # ties
    universe = rng.permutation(4 * n + 400).astype(np.int64)  # the store's ids, then the ids later adds draw from
    ids, spare = universe[:n].copy(), list(universe[n:])
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    column = {int(i): int(v) for i, v in zip(universe, rng.integers(0, 6, size=universe.shape[0])) if rng.random() < 0.9}
    attr = Attr(s)
    attr.set(np.fromiter(column.keys(), np.int64), np.fromiter(column.values(), np.int64))
    F = int(rng.integers(1, 21))
    defs, handles = [], []
    for j in range(F):
        kind = str(rng.choice(["allow", "deny", "where", "empty"]))
        if kind == "where":
            lo = int(rng.integers(0, 6))
            hi = lo + int(rng.integers(0, 2))
            defs.append(("where", lo, hi))
            handles.append(Filter.where(s, [(attr, "range", lo, hi)]))
        else:
            S = np.zeros(0, np.int64) if kind == "empty" else Y.draw_set(universe, float(rng.choice([0.003, 0.05, 0.3])), rng)
            mode = "allow" if kind == "empty" else kind
            defs.append((S, mode))
            handles.append(Filter(s, S, mode))

    def specs_now(cur_ids):
        return [(cur_ids[AY.eval_clauses([("a", "range", f[1], f[2])], cur_ids, {"a": column})], "allow") if isinstance(f[0], str) else f
                for f in defs]

    for call in range(4):
        cur_vecs, cur_ids, cur_off = _csr_of(s, d)
        specs = specs_now(cur_ids)
        counts = B.candidates(cur_ids, specs)
        sub = sorted(rng.permutation(F)[: int(rng.integers(1, F + 1))])
        Q = int(rng.choice([1, 2, 16, 17, 40]))
        k = int(rng.choice([1, 2, 10, 64, 100, 448, 449, 600]))
        q = rng.standard_normal((Q, d)).astype(np.float32)
        qf = rng.integers(0, len(sub), size=Q).astype(np.int32)
        need = sum(_r16(counts[j]) for j in sub)
        pool_rows = 0 if rng.random() < 0.25 else need + int(rng.integers(0, 64))  # holds this call, rarely the one before too
        dev = bool(rng.random() < 0.5)
        x = torch.from_numpy(q).cuda() if dev else q
        qfx = torch.from_numpy(qf).cuda() if dev else qf
        tag = (seed, call, "d%d-%s-n%d-F%d/%d-Q%d-k%d-B%d" % (d, metric, cur_ids.shape[0], len(sub), F, Q, k, pool_rows))
        gi, gd = ctx.search_exact_batch(s, x, k, metric, [handles[j] for j in sub], qfx, pool_rows=pool_rows)
        ctx.synchronize()  # (device buffers are complete behind the context's stream)
        oi, od = B.search(q, cur_vecs, cur_ids, cur_off, k, metric, [specs[j] for j in sub], qf)
        _eq(gi, gd, oi, od, tag)
        assert ((_np(gi) >= 0).sum(axis=1) == np.array([min(k, counts[sub[f]]) for f in qf])).all(), tag
        info = s.exact_pool_info()
        assert info["slots"] >= len(sub) and info["rows"] >= need, (tag, info)
        if pool_rows:
            assert info["rows"] <= pool_rows and info["cap_rows"] <= max(2 * pool_rows, 1024), (tag, info)
        # rows leave and arrive between the calls
        if cur_ids.shape[0] > 8 and rng.random() < 0.7:
            s.remove_ids(rng.permutation(cur_ids)[: int(rng.integers(1, max(2, cur_ids.shape[0] // 10)))])
        if rng.random() < 0.7:
            m = int(rng.integers(1, 100))
            new = np.array([spare.pop() for _ in range(m)], np.int64)
            s.add_entries(int(rng.choice(sorted(int(p) for p in s.list_ids()))), new, rng.standard_normal((m, d)).astype(np.float32))
    for f in handles:
        f.close()
    attr.close()
    s.close()
