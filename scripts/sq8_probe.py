"""Cost and recall of quantized search against search() and funnel search on one index.  One JSON line per measurement to stdout
and --out:

    python scripts/sq8_probe.py [--n 10000000] [--d 128] [--metric l2] [--nlist 4096] [--q 1024] [--nprobe 1,8,16] [--k 10]
        [--prefix 64] [--reps 5] [--out profiles/sq8_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows).  All calls run on the same index in one process.  Medians
over --reps calls after two warm-up calls; the phases of a call from HIP events (qk_timing), the whole call on the host clock
behind a synchronisation.
  search   qk_search at k: the yardstick; scan_bytes = unique probed rows x d x 4
  funnel   qk_funnel_search at (--prefix, fetch_k = k)
  sq8      qk_sq8_search at fetch_k = k, 2k, 4k (as far as QK_MAX_K allows): scan / merge ms of the candidate search, `finish_ms` =
           total_ms minus the phases up to the merge (the finish kernel plus the query coding between the coarse step and the
           grouping), scan_bytes (code bytes of the unique probed rows), recall@k against search()'s own answer at the same nprobe,
           `mirror_bytes` and `build_ms` (the first call after sq8_drop minus the median call: range, encode and their host waits)
The probe asserts nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np

PHASES = ("coarse_ms", "group_ms", "scan_ms", "merge_ms", "total_ms")


def timed(ctx, fn, reps):
    for _ in range(2):
        fn()
    rows, wall = [], []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        tm = fn()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(tm)
    rec = {p: float(np.median([r[p] for r in rows])) for p in PHASES}
    rec["wall_ms"] = float(np.median(wall))
    rec["scan_bytes"] = int(rows[-1]["scan_bytes"])
    rec["finish_ms"] = rec["total_ms"] - rec["coarse_ms"] - rec["group_ms"] - rec["scan_ms"] - rec["merge_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,8,16")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--prefix", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from quake_amd import capi
    from quake_amd._lib import QK_MAX_K
    from scripts.filter_probe import corpus
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(n=args.n, d=args.d, metric=args.metric, nlist=args.nlist, q=args.q, k=args.k, **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, args.metric, seed=1234)
    q = qall[: args.q].contiguous()
    k, metric = args.k, args.metric

    def recall(got, truth):
        ctx.synchronize()
        got = got.cpu().numpy()
        return sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth)) / max(1, int((truth >= 0).sum()))

    for nprobe in [int(v) for v in args.nprobe.split(",")]:
        srec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2], args.reps)
        emit(dict(case="search", nprobe=nprobe, kernel=ctx.last_scan_kernel(), **srec))
        truth = ctx.search(parent, s, q, nprobe, k, metric)[0]
        ctx.synchronize()
        truth = truth.cpu().numpy()
        dp = min(args.prefix, args.d)
        rec = timed(ctx, lambda: ctx.funnel_search(parent, s, q, nprobe, k, k, dp, metric, timing=True)[2], args.reps)
        emit(dict(case="funnel", nprobe=nprobe, prefix_dim=dp, fetch_k=k, kernel=ctx.last_scan_kernel(), **rec,
                  total_ms_vs_search=rec["total_ms"] / srec["total_ms"], recall_at_k=recall(ctx.funnel_search(parent, s, q, nprobe, k, k, dp, metric)[0], truth)))
        for fk in (k, 2 * k, 4 * k):
            if fk > QK_MAX_K:
                continue
            s.sq8_drop()
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.sq8_search(parent, s, q, nprobe, k, fk, metric)
            ctx.synchronize()
            first = (time.perf_counter() - t0) * 1e3
            rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, timing=True)[2], args.reps)
            emit(dict(case="sq8", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, mirror_bytes=s.sq8_info()["bytes"],
                      build_ms=first - rec["wall_ms"], bytes_vs_search=rec["scan_bytes"] / max(1, srec["scan_bytes"]),
                      scan_ms_vs_search=rec["scan_ms"] / srec["scan_ms"], total_ms_vs_search=rec["total_ms"] / srec["total_ms"],
                      recall_at_k=recall(ctx.sq8_search(parent, s, q, nprobe, k, fk, metric)[0], truth)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
