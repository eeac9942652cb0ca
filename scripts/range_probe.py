"""Range-search probe on the bench corpus shape.  One JSON line per measurement to stdout and to --out:

    python scripts/range_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--reps 7] [--out profiles/range_probe.jsonl]
                                  [--baseline-only]

For nprobe 1 and 8: the k = 10 search and the k = 449 search of the same batch (the wide-k path: it launches the very key-emission
kernel a range search launches) -- these two lines need nothing a tree without range search lacks, so --baseline-only runs on the
parent commit for the yardstick -- then range_search at four radii: "0" (half the smallest nearest-neighbour distance of the batch:
about no hit), "10" (the median 10th-neighbour distance of the k = 10 search), "1000" (found from there by bisection on count-only
calls until the mean hits per query are about 1000) and the infinite radius.  Per line: the phases of the call from HIP events
(qk_timing: coarse_ms, group_ms = pair offsets, scan_ms = the emission scan, merge_ms = counting + compaction, total_ms), the
whole call on the host clock behind a synchronisation (wall_ms), medians over --reps calls after two warm-up calls; the hits, the
algorithmic bytes of the probed lists with the rate scan_bytes / scan_ms, the query passes, and how many calls the cap=None
protocol of the wrapper needed (cap_calls: 1 = the first guess held).
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/range_probe.py ...` for the per-kernel summary."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.filter_probe import corpus  # noqa: E402  (the same seeded corpus)

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
    rec["scan_gbps"] = rec["scan_bytes"] / max(rec["scan_ms"], 1e-9) / 1e6
    rec["n_items"] = int(rows[-1]["n_items"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    from quake_amd import capi
    ctx = capi.Context(0)
    if not hasattr(ctx, "range_search") and not args.baseline_only:
        sys.exit("this tree has no range search: run with --baseline-only")
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = dict(tag=args.tag, n=args.n, d=args.d, nlist=args.nlist, q=args.q, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, "l2", seed=1234)
    q = qall[: args.q].contiguous()
    Q = args.q
    for nprobe in (1, 8):
        d10 = None
        for k in (10, 449):
            oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
            od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
            rec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, "l2", timing=True, out=(oi, od))[2], args.reps)
            emit(dict(case="search_k%d" % k, nprobe=nprobe, kernel=ctx.last_scan_kernel(), **rec))
            if k == 10:
                d10 = od.clone()
        if args.baseline_only:
            continue

        def count(r):
            lims = ctx.range_search(parent, s, q, nprobe, r, "l2", cap=0)[0]
            return int(lims[Q]) / Q

        r10 = float(d10[:, 9][torch.isfinite(d10[:, 9])].median())
        lo, hi = r10, r10
        while count(hi) < 1000 and hi < 1e30:
            lo, hi = hi, hi * 1.25
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if count(mid) < 1000 else (lo, mid)
        radii = [("0", 0.5 * float(d10[:, 0].min())), ("10", r10), ("1000", hi), ("inf", float("inf"))]
        for name, r in radii:
            lims, gi, gd = ctx.range_search(parent, s, q, nprobe, r, "l2")  # the wrapper's own capacity protocol
            cap_calls = ctx.last_range_calls
            total = int(lims[Q])
            bi = torch.empty((max(total, 1),), dtype=torch.int64, device="cuda")
            bd = torch.empty((max(total, 1),), dtype=torch.float32, device="cuda")
            del gi, gd
            rec = timed(ctx, lambda: ctx.range_search(parent, s, q, nprobe, r, "l2", timing=True, out=(bi, bd))[3], args.reps)
            rec["merge_share"] = rec["merge_ms"] / max(rec["total_ms"], 1e-9)
            emit(dict(case="range_" + name, nprobe=nprobe, radius=r, hits_total=total, hits_per_query=total / Q, cap_calls=cap_calls,
                      kernel=ctx.last_scan_kernel(), **rec))
            del bi, bd
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
