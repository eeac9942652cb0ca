"""Cost of grouped search with members (group_size) on the bench corpus shape.  One JSON line per measurement to stdout and --out:

    python scripts/grouped_members_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--reps 7]
        [--cases old,m1,m4,m16,followup] [--nprobes 1,8] [--tree DIR] [--tag TAG] [--out profiles/grouped_members_probe.jsonl]

The shape of scripts/grouped_probe.py: 10M x 128 L2, nlist 4096, 1024 queries, k = 10, about n, n / 8 and 1000 groups (group =
id // block), medians over --reps calls after two warm-up calls, the phases of the call from HIP events (qk_timing; the member
rounds are part of merge_ms of their pass) and the whole call on the host clock behind a synchronisation.
  old        qk_search_grouped, the one-row entry point.  --tree DIR imports quake_amd from another checkout (one that may not know
             group_size at all): run this case on the parent commit and on this tree, alternating, to see whether the one-row call moved
  m1/m4/m16  qk_search_grouped_n at group_size 1, 4, 16; ratio_to_m1 of total_ms is reported with every m > 1 line
  followup   the workaround at one shape (nprobe 8, n / 8 groups): after the one-row call, one filtered search with k = 4 per
             returned group under where=[(col, "range", g, g)] -- timed for --followup-queries queries (each costs k filter builds and
             searches) and reported per query and scaled to the batch
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/grouped_members_probe.py ...` for the kernel digest (a
traced run's timings differ: keep the two apart)."""
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
    rec["total_ms_min"] = float(min(r["total_ms"] for r in rows))
    rec["total_ms_max"] = float(max(r["total_ms"] for r in rows))
    rec["n_items"] = int(rows[-1]["n_items"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="old,m1,m4,m16,followup")
    ap.add_argument("--nprobes", default="1,8")
    ap.add_argument("--followup-queries", type=int, default=8)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from quake_amd import capi
    from scripts.filter_probe import corpus  # (the same seeded corpus)
    cases = args.cases.split(",")
    ctx = capi.Context(0)
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
    Q, n, k = args.q, args.n, 10
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    blocks = [("n", 1), ("n/8", 8), ("1000", max(1, n // 1000))]
    cols = {}
    for name, block in blocks:
        cols[name] = capi.Attr(s)
        cols[name].set(ids, ids // block)
    ctx.synchronize()
    og = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    for nprobe in [int(v) for v in args.nprobes.split(",")]:
        for name, block in blocks:
            col = cols[name]
            base = None
            for case in cases:
                if case == "old":
                    oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
                    od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
                    rec = timed(ctx, lambda: ctx.search_grouped(parent, s, q, nprobe, k, "l2", col, timing=True, out=(oi, od, og))[3], args.reps)
                    emit(dict(case="old", groups=name, nprobe=nprobe, **rec))
                elif case[0] == "m" and case[1:].isdigit():
                    m = int(case[1:])
                    oi = torch.empty((Q, k, m), dtype=torch.int64, device="cuda")
                    od = torch.empty((Q, k, m), dtype=torch.float32, device="cuda")
                    rec = timed(ctx, lambda: ctx.search_grouped(parent, s, q, nprobe, k, "l2", col, timing=True, out=(oi, od, og),
                                                                group_size=m)[3], args.reps)
                    if m == 1:
                        base = rec["total_ms"]
                    rec["ratio_to_m1"] = rec["total_ms"] / base if base else None
                    rec["members_found"] = float((oi >= 0).float().mean().item())
                    emit(dict(case="members", m=m, groups=name, nprobe=nprobe, **rec))
            if "followup" in cases and nprobe == 8 and name == "n/8":
                nq = min(args.followup_queries, Q)
                ctx.synchronize()
                t0 = time.perf_counter()
                gi, gd, gg = ctx.search_grouped(parent, s, q[:nq], nprobe, k, "l2", col)
                ctx.synchronize()
                groups, live = gg.cpu().numpy(), gi.cpu().numpy() >= 0
                calls = 0
                for i in range(nq):
                    for j in range(k):
                        if not live[i, j]:
                            continue
                        g = int(groups[i, j])
                        f = capi.Filter.where(s, [(col, "range", g, g)])
                        ctx.search(parent, s, q[i:i + 1], nprobe, 4, "l2", filter=f)
                        ctx.synchronize()
                        f.close()
                        calls += 1
                wall = (time.perf_counter() - t0) * 1e3
                emit(dict(case="followup_filtered_searches", groups=name, nprobe=nprobe, queries=nq, calls=calls, wall_ms=wall,
                          wall_ms_per_query=wall / nq, wall_ms_scaled_to_batch=wall / nq * Q))
    for c in cols.values():
        c.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
