"""Grouped-search probe on the bench corpus shape.  One JSON line per measurement to stdout and to --out:

    python scripts/grouped_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--reps 7] [--out profiles/grouped_probe.jsonl]

For nprobe 1, 8 and 32 and for about n, n / 8 and 1000 groups (group = id // block: ids are in build order, so the rows of a group
are neighbours in a list, like the chunks of a document) the k = 10 grouped search: the phases of the call from HIP events
(qk_timing: coarse_ms, group_ms = pair offsets + clearing the tables, scan_ms = the emission scan, merge_ms = reduction +
selection, total_ms), the whole call on the host clock behind a synchronisation (wall_ms), medians over --reps calls after two
warm-up calls, the query passes, and the one-off cost of deriving the row values (rowvals_ms: the first call minus a later one).
Next to them, per nprobe, on the same tree: the plain search at k = 449 (the wide-k path: emission + selection without the
reduction), the fused search at k = 10, and today's workaround -- search at k = 80 and de-duplication on the host -- with the share of
queries for which it returns fewer than 10 groups or another group set than the exact call.
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/grouped_probe.py ...` for the per-kernel summary (a
traced run's timings differ: keep the two apart)."""
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
    rec["n_items"] = int(rows[-1]["n_items"])
    return rec


def dedup_host(ids, groups_of, k):
    """the workaround: the first k distinct groups of an oversampled result, on the host; rows padded with -1"""
    ids = ids.cpu().numpy()
    g = groups_of(ids)
    out = np.full((ids.shape[0], k), -1, np.int64)
    for i in range(ids.shape[0]):
        live = ids[i] >= 0
        _, first = np.unique(g[i][live], return_index=True)
        first = np.sort(first)[:k]
        out[i, :first.shape[0]] = g[i][live][first]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from quake_amd import capi
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
    oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    og = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    for nprobe in (1, 8, 32):
        for kk in (10, 449):
            pi = torch.empty((Q, kk), dtype=torch.int64, device="cuda")
            pd = torch.empty((Q, kk), dtype=torch.float32, device="cuda")
            rec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, kk, "l2", timing=True, out=(pi, pd))[2], args.reps)
            emit(dict(case="search_k%d" % kk, nprobe=nprobe, kernel=ctx.last_scan_kernel(), **rec))
        p80 = torch.empty((Q, 80), dtype=torch.int64, device="cuda")
        d80 = torch.empty((Q, 80), dtype=torch.float32, device="cuda")
        for name, block in blocks:
            col = cols[name]
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.search_grouped(parent, s, q, nprobe, k, "l2", col, out=(oi, od, og))
            ctx.synchronize()
            first_ms = (time.perf_counter() - t0) * 1e3
            builds = col.group_info()["builds"]
            rec = timed(ctx, lambda: ctx.search_grouped(parent, s, q, nprobe, k, "l2", col, timing=True, out=(oi, od, og))[3], args.reps)
            assert col.group_info()["builds"] == builds == 1
            rec["merge_share"] = rec["merge_ms"] / max(rec["total_ms"], 1e-9)
            exact = og.cpu().numpy().copy()
            exact_ids = oi.cpu().numpy()
            emit(dict(case="grouped_k10", groups=name, nprobe=nprobe, kernel=ctx.last_scan_kernel(), first_call_ms=first_ms,
                      rowvals_ms=max(first_ms - rec["wall_ms"], 0.0) if nprobe == 1 else None,
                      full_rows=float((exact_ids[:, -1] >= 0).mean()), **rec))
            # the workaround: k = 80 and de-duplication on the host (timed as a whole: search, copy back, numpy)
            wall = []
            for _ in range(3):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.search(parent, s, q, nprobe, 80, "l2", out=(p80, d80))
                ctx.synchronize()
                got = dedup_host(p80, lambda a: np.where(a >= 0, a // block, -1), k)
                wall.append((time.perf_counter() - t0) * 1e3)
            n_exact = (exact_ids >= 0).sum(axis=1)
            short = ((got >= 0).sum(axis=1) < np.minimum(n_exact, k))
            wrong = np.array([set(got[i][got[i] >= 0].tolist()) != set(exact[i][exact_ids[i] >= 0].tolist()) for i in range(Q)])
            emit(dict(case="search_k80_dedup_host", groups=name, nprobe=nprobe, wall_ms=float(np.median(wall)),
                      share_fewer_groups=float(short.mean()), share_wrong_group_set=float(wrong.mean())))
    for c in cols.values():
        c.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
