"""Expression-filter probe: what an OR of conjunctions with value sets costs to make and to re-derive, next to the conjunction
filter (qk_filter_create_where) on the same clauses and to the id-set filter over the same candidates.  One JSON line per
measurement to stdout and to --out:

    python scripts/expr_filter_probe.py [--n 10000000] [--nlist 4096] [--reps 7] [--out profiles/expr_filter_probe.jsonl]

The store and the columns are scripts/attr_filter_probe.py's: n x 16 floats in nlist lists of random lengths, "table" -- ids a
permutation of 0 .. n-1 -- and "sorted" -- the same ids times 1 000 003 --, eight columns of independent uniform values in
[0, 2^20) for every id.  `create` is the host wall clock around the call and a synchronise; `rebuild` is a one-query filtered
search that has to re-derive the mask first (after a qk_attr_set of one id) minus the same search with nothing to do; medians
over --reps.  Three families of records:
  what = "generality"  one term of nc = 1 / 4 / 8 range clauses at selectivity 0.5: qk_filter_create_expr against
                       qk_filter_create_where on the same clauses, alternating (expr_* / where_*)
  what = "set"         IN_SET of 2 / 16 / 1024 / 65 536 / 2^20 values drawn from [0, 2^20) on column 0, against the only other
                       route: evaluate on the host (numpy isin, host_eval_ms, one shot) and qk_filter_create over the resulting ids
                       (ids_create_ms; the sum is the route's cost)
  what = "terms"       1 / 2 / 4 / 8 terms of 2 range clauses, columns t and t + 3 (mod 8): "fail" -- every term passes ~1 %
                       of the rows, so most rows walk every term -- and "pass" -- the first term passes ~90 %
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/expr_filter_probe.py ...` for the kernels' own times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VMAX = 1 << 20


def median_ms(fn, reps):
    return float(np.median([fn() for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/expr_filter_probe.jsonl")
    ap.add_argument("--layouts", default="table,sorted")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expr_filter_probe.py measures on the GPU; none found")
    from quake_amd.capi import Attr, Context, Filter, Store
    ctx = Context(0)
    n, nlist, d = args.n, args.nlist, 16
    rng = np.random.default_rng(7)
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sizes = rng.multinomial(n, rng.dirichlet(np.full(nlist, 8.0)))
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    g = torch.Generator(device="cuda").manual_seed(1)
    vecs = torch.randn(n, d, device="cuda", generator=g)
    cent = torch.randn(nlist, d, generator=torch.Generator().manual_seed(2))
    q = torch.randn(1, d, generator=torch.Generator().manual_seed(3)).numpy()
    vals = [rng.integers(0, VMAX, n) for _ in range(8)]
    for layout in args.layouts.split(","):
        step = 1 if layout == "table" else 1_000_003
        ids = rng.permutation(n).astype(np.int64) * step
        s = Store(ctx, d)
        s.build_csr(offsets, torch.from_numpy(ids).cuda(), vecs)
        parent = Store(ctx, d)
        parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
        cols = []
        for v in vals:
            a = Attr(s)
            a.set(ids, v)
            ctx.synchronize()
            assert a.info()["layout"] == layout, a.info()
            cols.append(a)

        def call_ms(f):
            t0 = time.perf_counter()
            ctx.search(parent, s, q, 1, 10, "l2", filter=f)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def touch_column():
            cols[0].set(ids[:1], vals[0][:1])  # (the same value: a new version, the same candidates)
            ctx.synchronize()

        def rebuild_ms(f):
            def one():
                touch_column()
                return call_ms(f)
            call_ms(f)
            dirty = median_ms(one, args.reps)
            return dirty - median_ms(lambda: call_ms(f), args.reps)

        def create_ms(make):
            """median over --reps of making (and closing) the filter; returns (ms, the last filter, open)"""
            ts, f = [], None
            for _ in range(args.reps):
                if f is not None:
                    f.close()
                t0 = time.perf_counter()
                f = make()
                ctx.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts)), f

        # ---- the cost of generality: one term without sets against the conjunction filter, alternating
        for nc in (1, 4, 8):
            t = int(round(VMAX * 0.5 ** (1.0 / nc)))
            keep = np.ones(n, bool)
            for v in vals[:nc]:
                keep &= v < t
            cl = [(cols[i], "range", 0, t - 1) for i in range(nc)]
            rec = dict(what="generality", layout=layout, n=n, nlist=nlist, clauses=nc, candidates=int(keep.sum()))
            for rnd in range(2):  # (where, expr, where, expr: the second round is the one reported next to the first)
                for kind, make in (("where", lambda: Filter.where(s, cl)), ("expr", lambda: Filter.expr(s, [cl]))):
                    ms, f = create_ms(make)
                    assert f.info()["rows_allowed"] == int(keep.sum())
                    rec["%s_create_ms_%d" % (kind, rnd)] = ms
                    rec["%s_rebuild_ms_%d" % (kind, rnd)] = rebuild_ms(f)
                    f.close()
            emit(rec)
        # ---- sets: IN_SET on column 0 against host evaluation + qk_filter_create
        for ns in (2, 16, 1024, 65536, 1 << 20):
            sv = rng.permutation(VMAX)[:ns].astype(np.int64)
            t0 = time.perf_counter()
            keep = np.isin(vals[0], sv)
            S = ids[keep]
            host_eval = (time.perf_counter() - t0) * 1e3
            ms, f = create_ms(lambda: Filter.expr(s, [[(cols[0], "in", sv)]]))
            assert f.info()["rows_allowed"] == int(keep.sum())
            rb = rebuild_ms(f)
            db = f.info()["device_bytes"]
            f.close()
            ims, fi = create_ms(lambda: Filter(s, S, "allow"))
            idb = fi.info()["device_bytes"]
            fi.close()
            emit(dict(what="set", layout=layout, n=n, nlist=nlist, set_values=ns, candidates=int(keep.sum()), expr_create_ms=ms,
                      expr_rebuild_ms=rb, host_eval_ms=host_eval, ids_create_ms=ims, expr_device_bytes=db, ids_device_bytes=idb))
        # ---- terms: 2 clauses each, most rows failing every term / most rows passing the first
        for mode, p_first, p_rest in (("fail", 0.01, 0.01), ("pass", 0.9, 0.01)):
            for nt in (1, 2, 4, 8):
                keep = np.zeros(n, bool)
                terms = []
                for t_ in range(nt):
                    thr = int(round(VMAX * (p_first if t_ == 0 else p_rest) ** 0.5))
                    c0, c1 = t_, (t_ + 3) % 8  # (eight different pairs of the eight columns)
                    keep |= (vals[c0] < thr) & (vals[c1] < thr)
                    terms.append([(cols[c0], "range", 0, thr - 1), (cols[c1], "range", 0, thr - 1)])
                ms, f = create_ms(lambda: Filter.expr(s, terms))
                assert f.info()["rows_allowed"] == int(keep.sum())
                emit(dict(what="terms", layout=layout, n=n, nlist=nlist, mode=mode, terms=nt, candidates=int(keep.sum()),
                          expr_create_ms=ms, expr_rebuild_ms=rebuild_ms(f)))
                f.close()
        for a in cols:
            a.close()
        s.close()
        parent.close()


if __name__ == "__main__":
    main()
