"""Attribute-filter probe: what a predicate filter costs to make and to re-derive, next to the id-set filter over the same
candidates.  One JSON line per measurement to stdout and to --out:

    python scripts/attr_filter_probe.py [--n 10000000] [--nlist 4096] [--reps 7] [--out profiles/attr_filter_probe.jsonl]

The mask build reads the stored ids and the columns, never the vectors, so the store is n x 16 floats in nlist lists of random
lengths.  Two stores: "table" -- ids a permutation of 0 .. n-1, every column a direct table -- and "sorted" -- the same ids times
1 000 003, every column sorted pairs.  Eight columns hold independent uniform values in [0, 2^20) for every id; a filter of nc
clauses at selectivity s asks each of its columns for `value < t` with t chosen so that the conjunction passes the fraction s.
Per (layout, nc, s):
  where_create_ms   qk_filter_create_where, host wall clock around the call and a synchronise (one mask build, no sort)
  where_rebuild_ms  a one-query filtered search that has to re-derive the mask first (after a qk_attr_set of one id) minus the
                    same search with nothing to do -- host wall clock around call + synchronise, medians over --reps
  ids_create_ms     qk_filter_create over exactly the ids the predicate allows (host sort + upload + one mask build)
  ids_rebuild_ms    the same difference for that filter after a store change (one row added to a list)
The id-set filter and k_filter_build are the parent commit's, unchanged on this tree.
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/attr_filter_probe.py ...` for the kernels' own times."""
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
    ts = []
    for _ in range(reps):
        ts.append(fn())
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/attr_filter_probe.jsonl")
    ap.add_argument("--layouts", default="table,sorted")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attr_filter_probe.py measures on the GPU; none found")
    from quake_amd.capi import Attr, Context, Filter, Store
    ctx = Context(0)
    n, nlist, d = args.n, args.nlist, 16
    rng = np.random.default_rng(7)
    out = open(args.out, "w") if args.out else None

    lib = os.path.basename(os.environ.get("QUAKE_HIP_LIB", "") or "libquake_hip.so")  # (a side build: A/B runs)

    def emit(rec):
        line = json.dumps(dict(rec, lib=lib))
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
            t0 = time.perf_counter()
            a = Attr(s)
            a.set(ids, v)
            ctx.synchronize()
            info = a.info()
            assert info["layout"] == layout, info
            cols.append(a)
            emit(dict(what="column", layout=layout, n=n, set_ms=(time.perf_counter() - t0) * 1e3, device_bytes=info["device_bytes"]))
        next_id = [int(ids.max()) + step]

        def call_ms(f):
            t0 = time.perf_counter()
            ctx.search(parent, s, q, 1, 10, "l2", filter=f)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def touch_column():
            cols[0].set(ids[:1], vals[0][:1])  # (the same value: a new version, the same candidates)
            ctx.synchronize()

        def touch_store():
            s.add_entries(0, np.array([next_id[0]], np.int64), np.zeros((1, d), np.float32))
            next_id[0] += step
            s.publish()
            ctx.synchronize()

        def rebuild_ms(f, touch):
            def one():
                touch()
                return call_ms(f)
            call_ms(f)
            dirty = median_ms(one, args.reps)
            steady = median_ms(lambda: call_ms(f), args.reps)
            return dirty - steady, steady

        for sel in (0.5, 0.001):
            for nc in (1, 4, 8):
                t = int(round(VMAX * sel ** (1.0 / nc)))
                keep = np.ones(n, bool)
                for v in vals[:nc]:
                    keep &= v < t
                t0 = time.perf_counter()
                fw = Filter.where(s, [(cols[i], "range", 0, t - 1) for i in range(nc)])
                ctx.synchronize()
                where_create = (time.perf_counter() - t0) * 1e3
                assert fw.info()["rows_allowed"] == int(keep.sum())
                where_rebuild, steady = rebuild_ms(fw, touch_column)
                S = ids[keep]
                t0 = time.perf_counter()
                fi = Filter(s, S, "allow")
                ctx.synchronize()
                ids_create = (time.perf_counter() - t0) * 1e3
                ids_rebuild, _ = rebuild_ms(fi, touch_store)
                emit(dict(what="filter", layout=layout, n=n, nlist=nlist, clauses=nc, selectivity=sel, candidates=int(keep.sum()),
                          where_create_ms=where_create, where_rebuild_ms=where_rebuild, ids_create_ms=ids_create,
                          ids_rebuild_ms=ids_rebuild, steady_call_ms=steady, where_device_bytes=fw.info()["device_bytes"],
                          ids_device_bytes=fi.info()["device_bytes"], rebuilds=fw.info()["rebuilds"]))
                fw.close()
                fi.close()
        for a in cols:
            a.close()
        s.close()
        parent.close()


if __name__ == "__main__":
    main()
