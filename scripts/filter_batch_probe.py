"""Per-query filter probe: what the per-lane mask word costs and what one batched call buys over one call per filter.  One JSON
line per measurement to stdout and to --out:

    python scripts/filter_batch_probe.py [--n 10000000] [--nlist 4096] [--q 1024] [--reps 7] [--tenants 16]
                                         [--union 16,256,1024] [--out profiles/filter_batch_probe.jsonl] [--single-only]

Corpus: n x 128 L2, k 10 (scripts/filter_probe.py's bench128), nprobe 1 and 8.
  word     one filter for the whole batch, at selectivity 1 and at uniform selectivity 0.1, through the single-filter entry point
           (qk_search_filtered) and through the per-query one with F = 1 (qk_search_filtered_batch): the scan kernel's device time
           (qk_timing.scan_ms: HIP events around the kernel) and the whole call's, medians over --reps calls after two warm-ups.
  tenants  --tenants filters, whole id ranges of 1 / tenants of the build order each, the --q queries spread evenly over them: one
           per-query call against one single-filter call per tenant with its q / tenants queries (the sums of the calls' scan_ms /
           total_ms, and the wall clock of the whole loop behind a synchronisation).
  union    F filters (uniform ids, selectivity 1 / F each): the device time of the first per-query call (it builds the union: HIP
           events around the call) next to a steady one, and the wall clock of qk_filter_batch's host side.
--single-only measures only what a tree without the per-query entry points has (run it on the parent commit for the yardstick).
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/filter_batch_probe.py ...` for k_filter_union's own
time and to see that a second call with unchanged filters does not launch it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filter_probe import corpus, draw, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tenants", type=int, default=16)
    ap.add_argument("--union", default="16,256,1024")
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-only", action="store_true")
    args = ap.parse_args()
    from quake_amd import capi
    Filter = capi.Filter
    batch = hasattr(capi, "QK_MAX_BATCH_FILTERS") and not args.single_only
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = dict(tree="per-query" if hasattr(capi, "QK_MAX_BATCH_FILTERS") else "single-filter only", n=args.n, q=args.q, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    d, metric, k, nprobes = 128, "l2", 10, [1, 8]
    s, parent, offsets, qall = corpus(ctx, args.n, d, args.nlist, metric, seed=1234)
    Q = args.q
    q = qall[:Q].contiguous()
    oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(99)

    # ---- the per-lane word ---------------------------------------------------------------------------------------------------
    zeros = torch.zeros(Q, dtype=torch.int32, device="cuda")
    for sel in (1.0, 0.1):
        f = Filter(s, draw(args.n, sel, "uniform", rng), "allow")
        for nprobe in nprobes:
            sc, tot, _ = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=(oi, od), filter=f)[2], args.reps)
            emit(dict(case="word", entry="single", selectivity=sel, nprobe=nprobe, scan_ms=sc, total_ms=tot, kernel=ctx.last_scan_kernel()))
            if batch:
                sc, tot, _ = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=(oi, od), filters=[f],
                                                           query_filter=zeros)[2], args.reps)
                emit(dict(case="word", entry="per-query F=1", selectivity=sel, nprobe=nprobe, scan_ms=sc, total_ms=tot,
                          kernel=ctx.last_scan_kernel()))
        f.close()

    # ---- what batching buys --------------------------------------------------------------------------------------------------
    T = args.tenants
    per = Q // T
    bounds = np.linspace(0, args.n, T + 1).astype(np.int64)
    fs = [Filter(s, np.arange(bounds[t], bounds[t + 1], dtype=np.int64), "allow") for t in range(T)]
    qf = (torch.arange(Q, device="cuda", dtype=torch.int32) % T).contiguous()
    qs = [q[torch.nonzero(qf == t).reshape(-1)].contiguous() for t in range(T)]
    outs = [(torch.empty((qs[t].shape[0], k), dtype=torch.int64, device="cuda"),
             torch.empty((qs[t].shape[0], k), dtype=torch.float32, device="cuda")) for t in range(T)]
    for nprobe in nprobes:
        def loop():
            tms = [ctx.search(parent, s, qs[t], nprobe, k, metric, timing=True, out=outs[t], filter=fs[t])[2] for t in range(T)]
            return dict(scan_ms=sum(t["scan_ms"] for t in tms), total_ms=sum(t["total_ms"] for t in tms))
        sc, tot, _ = timed(ctx, loop, args.reps)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            loop()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.reps
        emit(dict(case="tenants", entry="%d single-filter calls of %d queries" % (T, per), tenants=T, nprobe=nprobe, scan_ms=sc,
                  total_ms=tot, wall_ms=wall, kernel=ctx.last_scan_kernel()))
        if batch:
            fn = lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=(oi, od), filters=fs, query_filter=qf)[2]
            sc, tot, _ = timed(ctx, fn, args.reps)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3 / args.reps
            emit(dict(case="tenants", entry="one per-query call", tenants=T, nprobe=nprobe, scan_ms=sc, total_ms=tot, wall_ms=wall,
                      kernel=ctx.last_scan_kernel()))
    for f in fs:
        f.close()

    # ---- the union -----------------------------------------------------------------------------------------------------------
    if batch:
        for F in [int(v) for v in args.union.split(",") if v]:
            perm = rng.permutation(args.n).astype(np.int64)
            cut = np.linspace(0, args.n, F + 1).astype(np.int64)
            fs = [Filter(s, np.sort(perm[cut[i]:cut[i + 1]]), "allow") for i in range(F)]
            qf = (torch.arange(Q, device="cuda", dtype=torch.int32) % F).contiguous()
            fn = lambda: ctx.search(parent, s, q, 1, k, metric, timing=True, out=(oi, od), filters=fs, query_filter=qf)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            e0.record()
            t0 = time.perf_counter()
            first = fn()[2]
            host_first = (time.perf_counter() - t0) * 1e3
            e1.record()
            torch.cuda.synchronize()
            dev_first = e0.elapsed_time(e1)
            e0.record()
            t0 = time.perf_counter()
            steady = fn()[2]
            host_steady = (time.perf_counter() - t0) * 1e3
            e1.record()
            torch.cuda.synchronize()
            dev_steady = e0.elapsed_time(e1)
            ctx.set_stream(None)
            emit(dict(case="union", F=F, first_call_device_ms=dev_first, steady_call_device_ms=dev_steady,
                      first_call_host_ms=host_first, steady_call_host_ms=host_steady, first_scan_ms=first["scan_ms"],
                      steady_scan_ms=steady["scan_ms"], kernel=ctx.last_scan_kernel()))
            for f in fs:
                f.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
