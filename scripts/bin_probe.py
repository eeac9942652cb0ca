"""Cost and recall of binary search against search() and quantized search on one index.  One JSON line per measurement to stdout
and --out:

    python scripts/bin_probe.py [--n 10000000] [--d 128] [--metric l2] [--nlist 4096] [--q 1024] [--nprobe 1,8,16] [--k 10]
        [--reps 5] [--label product] [--only-bin] [--out profiles/bin_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows, not trained embeddings).  All calls run on the same index in
one process, the forms of one nprobe one after the other.  Medians over --reps calls after two warm-up calls; the phases of a call
from HIP events (qk_timing), the whole call on the host clock behind a synchronisation.
  search     qk_search at k: the yardstick; scan_bytes = unique probed rows x d x 4
  sq8        qk_sq8_search at fetch_k = min(4k, 448); sq8_deep: qk_sq8_search_deep at fetch_k = min(40k, 4096)
  bin        qk_bin_search at fetch_k = k, 4k, 10k, 40k (capped at 4096): `select_ms` = scan_ms (k_bin_select), `finish_ms` =
             total_ms minus the phases up to the select (the exact finish), scan_bytes (code bytes of every query's probed rows),
             recall@k against search()'s own answer at the same nprobe, `mirror_bytes` and `build_ms` (the first call after
             bin_drop minus the median call: range, encode and their host waits)
--label names the library the lines come from (the A/B of the LDS key cache: QUAKE_HIP_LIB selects a side build); --only-bin skips
the other forms.  The probe asserts nothing about time."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="product")
    ap.add_argument("--only-bin", action="store_true")
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
        line = json.dumps(dict(n=args.n, d=args.d, metric=args.metric, nlist=args.nlist, q=args.q, k=args.k, label=args.label, **rec))
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
        truth = ctx.search(parent, s, q, nprobe, k, metric)[0]
        ctx.synchronize()
        truth = truth.cpu().numpy()
        if not args.only_bin:
            emit(dict(case="search", nprobe=nprobe, kernel=ctx.last_scan_kernel(), **srec))
            for case, fk, deep in (("sq8", min(4 * k, QK_MAX_K), False), ("sq8_deep", min(40 * k, 4096), True)):
                if deep and fk <= QK_MAX_K:
                    continue
                rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, timing=True, deep=deep)[2], args.reps)
                emit(dict(case=case, nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, total_ms_vs_search=rec["total_ms"] / srec["total_ms"],
                          recall_at_k=recall(ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, deep=deep)[0], truth)))
            s.sq8_drop()
        for fk in sorted({min(m * k, 4096) for m in (1, 4, 10, 40)}):
            s.bin_drop()
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.bin_search(parent, s, q, nprobe, k, fk, metric)
            ctx.synchronize()
            first = (time.perf_counter() - t0) * 1e3
            rec = timed(ctx, lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, timing=True)[2], args.reps)
            info = s.bin_info()
            emit(dict(case="bin", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, select_ms=rec["scan_ms"],
                      mirror_bytes=info["bytes"], cache_rows=info["cache_rows"], build_ms=first - rec["wall_ms"],
                      bytes_vs_search=rec["scan_bytes"] / max(1, srec["scan_bytes"]), scan_ms_vs_search=rec["scan_ms"] / srec["scan_ms"],
                      total_ms_vs_search=rec["total_ms"] / srec["total_ms"],
                      recall_at_k=recall(ctx.bin_search(parent, s, q, nprobe, k, fk, metric)[0], truth)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
