"""Cost and recall of funnel search against search() on one index.  One JSON line per measurement to stdout and --out:

    python scripts/funnel_probe.py [--n 10000000] [--d 768] [--metric ip] [--nlist 4096] [--q 1024] [--nprobe 1] [--k 100]
        [--prefix 64,128,256,384] [--fetch 100,200,448] [--reps 5] [--cases search,funnel] [--tag branch] [--out profiles/funnel_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows: they carry NO Matryoshka structure, so the recall figures
say how a prefix of such rows ranks, not what a trained embedding gives).  All calls run on the same index in one process; the
yardstick of the parent commit is its own qk_search: run this script with --cases search --tag parent from a checkout of the parent
(its package loads its own library) before and after the run on this tree.
Medians over --reps calls after two warm-up calls; the phases of a call from HIP events (qk_timing), the whole call on the host
clock behind a synchronisation.
  search   qk_search at k: the yardstick; scan_bytes = unique probed rows x d x 4
  funnel   qk_funnel_search at (prefix_dim, fetch_k, k): scan / merge ms of the candidate search, `finish_ms` = total_ms minus the
           phases up to the merge (the finish kernel plus the query prefix preparation between the coarse step and the grouping),
           scan_bytes (prefix bytes of the unique probed rows) and their ratio to search()'s, recall@k against search()'s own answer
The probe asserts nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

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
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--metric", default="ip")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=1)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--prefix", default="64,128,256,384")
    ap.add_argument("--fetch", default="100,200,448")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="search,funnel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="branch", help="which tree / library the run belongs to (parent: run from the parent commit's tree)")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from quake_amd import capi
    from scripts.filter_probe import corpus
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = dict(lib=os.environ.get("QUAKE_HIP_LIB") or "libquake_hip.so", tag=args.tag, n=args.n, d=args.d,
                   metric=args.metric, nlist=args.nlist, q=args.q, nprobe=args.nprobe, k=args.k, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, args.metric, seed=1234)
    q = qall[: args.q].contiguous()
    nprobe, k, metric = args.nprobe, args.k, args.metric
    srec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2], args.reps)
    emit(dict(case="search", kernel=ctx.last_scan_kernel(), **srec))
    if "funnel" not in args.cases.split(","):
        return
    truth = ctx.search(parent, s, q, nprobe, k, metric)[0]
    ctx.synchronize()
    truth = truth.cpu().numpy()
    for dp in [int(v) for v in args.prefix.split(",")]:
        if dp > args.d:
            continue
        for fk in [int(v) for v in args.fetch.split(",")]:
            if fk < k:
                continue
            rec = timed(ctx, lambda: ctx.funnel_search(parent, s, q, nprobe, k, fk, dp, metric, timing=True)[2], args.reps)
            got = ctx.funnel_search(parent, s, q, nprobe, k, fk, dp, metric)[0]
            ctx.synchronize()
            got = got.cpu().numpy()
            hit = sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth))
            emit(dict(case="funnel", prefix_dim=dp, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec,
                      finish_ms=rec["total_ms"] - rec["coarse_ms"] - rec["group_ms"] - rec["scan_ms"] - rec["merge_ms"],
                      bytes_vs_search=rec["scan_bytes"] / max(1, srec["scan_bytes"]), scan_ms_vs_search=rec["scan_ms"] / srec["scan_ms"],
                      total_ms_vs_search=rec["total_ms"] / srec["total_ms"], recall_at_k=hit / max(1, int((truth >= 0).sum()))))
    if out:
        out.close()


if __name__ == "__main__":
    main()
