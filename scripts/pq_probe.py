"""Cost and recall of product-quantized search against search(), quantized search and binary search on one index.  One JSON line per
measurement to stdout and --out:

    python scripts/pq_probe.py [--n 10000000] [--d 128] [--metric l2] [--nlist 4096] [--q 1024] [--nprobe 1,8,16] [--k 10]
        [--m 16,32] [--fetch 10,40,100,400] [--train-rows 65536] [--niter 10] [--reps 5] [--out profiles/pq_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows, not trained embeddings).  All calls run on the same index in
one process.  Medians over --reps calls after two warm-up calls; the phases of a call from HIP events (qk_timing), the whole call
on the host clock behind a synchronisation.
  search     qk_search at k: the yardstick; scan_bytes = unique probed rows x d x 4
  sq8 / bin  qk_sq8_search (deep from fetch_k > 448) and qk_bin_search at every --fetch >= k, with recall@k against search()
  pq_train   per M: qk_store_pq_train on --train-rows rows, `train_ms` on the host clock
  pq         per M, nprobe and --fetch >= k: `table_ms` = group_ms (k_pq_lut), `select_ms` = scan_ms (k_pq_select), `finish_ms` =
             total_ms minus the phases up to the select, scan_bytes (code bytes of every query's probed rows), recall@k against
             search()'s own answer at the same nprobe, `mirror_bytes` and `encode_ms` (the first call after pq_drop minus the median call)
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
    ap.add_argument("--m", default="16,32")
    ap.add_argument("--fetch", default="10,40,100,400")
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--niter", type=int, default=10)
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
    nprobes = [int(v) for v in args.nprobe.split(",")]
    fetches = [f for f in (int(v) for v in args.fetch.split(",")) if f >= k]

    def recall(got, truth):
        ctx.synchronize()
        got = got.cpu().numpy()
        return sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth)) / max(1, int((truth >= 0).sum()))

    srec, truth = {}, {}
    for nprobe in nprobes:
        srec[nprobe] = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2], args.reps)
        t = ctx.search(parent, s, q, nprobe, k, metric)[0]
        ctx.synchronize()
        truth[nprobe] = t.cpu().numpy()
        emit(dict(case="search", nprobe=nprobe, kernel=ctx.last_scan_kernel(), **srec[nprobe]))
        for fk in fetches:
            deep = fk > QK_MAX_K
            rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, timing=True, deep=deep)[2], args.reps)
            emit(dict(case="sq8", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, total_ms_vs_search=rec["total_ms"] / srec[nprobe]["total_ms"],
                      recall_at_k=recall(ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, deep=deep)[0], truth[nprobe])))
            rec = timed(ctx, lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, timing=True)[2], args.reps)
            emit(dict(case="bin", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, total_ms_vs_search=rec["total_ms"] / srec[nprobe]["total_ms"],
                      recall_at_k=recall(ctx.bin_search(parent, s, q, nprobe, k, fk, metric)[0], truth[nprobe])))
    s.sq8_drop()
    s.bin_drop()
    for M in [int(v) for v in args.m.split(",")]:
        ctx.synchronize()
        t0 = time.perf_counter()
        s.pq_train(ctx, M, max_rows=args.train_rows, niter=args.niter, seed=7)
        ctx.synchronize()
        emit(dict(case="pq_train", M=M, train_rows=args.train_rows, niter=args.niter, train_ms=(time.perf_counter() - t0) * 1e3))
        for nprobe in nprobes:
            for fk in fetches:
                s.pq_drop()
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.pq_search(parent, s, q, nprobe, k, fk, metric)
                ctx.synchronize()
                first = (time.perf_counter() - t0) * 1e3
                rec = timed(ctx, lambda: ctx.pq_search(parent, s, q, nprobe, k, fk, metric, timing=True)[2], args.reps)
                emit(dict(case="pq", M=M, nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, table_ms=rec["group_ms"], select_ms=rec["scan_ms"],
                          mirror_bytes=s.pq_info()["bytes"], encode_ms=first - rec["wall_ms"],
                          bytes_vs_search=rec["scan_bytes"] / max(1, srec[nprobe]["scan_bytes"]), scan_ms_vs_search=rec["scan_ms"] / srec[nprobe]["scan_ms"],
                          total_ms_vs_search=rec["total_ms"] / srec[nprobe]["total_ms"],
                          recall_at_k=recall(ctx.pq_search(parent, s, q, nprobe, k, fk, metric)[0], truth[nprobe])))
    if out:
        out.close()


if __name__ == "__main__":
    main()
