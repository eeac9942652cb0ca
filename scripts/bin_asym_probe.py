"""Cost and recall of asymmetric binary search (binary_search with asymmetric=True: 1-bit rows, 4-bit queries, two factors per row)
against search(), binary search (Hamming) and quantized search on one index.  One JSON line per measurement to stdout and --out:

    python scripts/bin_asym_probe.py [--n 10000000] [--d 128] [--metric l2] [--nlist 4096] [--q 1024] [--nprobe 1,8] [--k 10]
        [--reps 5] [--out profiles/bin_asym_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows, not trained embeddings).  All calls run on the same index in
one process.  Medians over --reps calls after two warm-up calls; the phases of a call from HIP events (qk_timing), the whole call on
the host clock behind a synchronisation.  recall@k is against search()'s own answer at the same nprobe.
  search     qk_search at k: the yardstick
  sq8        qk_sq8_search at fetch_k = min(4k, 448)
  bin        qk_bin_search at fetch_k = 10, 40, 100, 400, 1000 (those not below k): `select_ms` = scan_ms (k_bin_select)
  asym       qk_bin_search_asym at the same fetch_k, rescore_k = 0: `select_ms` = scan_ms (k_bin_select_asym)
  build      the one-off builds: the first Hamming call (sign mirror) and the first asymmetric call (row factors) on the host clock
The probe asserts nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np

PHASES = ("coarse_ms", "group_ms", "scan_ms", "merge_ms", "total_ms")
FETCH = (10, 40, 100, 400, 1000)


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
    rec["total_ms_min"], rec["total_ms_max"] = float(min(r["total_ms"] for r in rows)), float(max(r["total_ms"] for r in rows))
    rec["select_ms"] = rec["scan_ms"]
    rec["tail_ms"] = rec["total_ms"] - rec["coarse_ms"] - rec["group_ms"] - rec["scan_ms"] - rec["merge_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,8")
    ap.add_argument("--k", type=int, default=10)
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
        line = json.dumps(dict(n=args.n, d=args.d, metric=args.metric, nlist=args.nlist, q=args.q, k=args.k,
                               corpus="clustered Gaussians, not trained embeddings", **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, args.metric, seed=1234)
    q = qall[: args.q].contiguous()
    k, metric = args.k, args.metric
    for name, asym in (("sign mirror", False), ("row factors", True)):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.bin_search(parent, s, q[:1], 1, 1, 1, metric, asymmetric=asym)
        ctx.synchronize()
        emit(dict(case="build", what=name, first_call_ms=(time.perf_counter() - t0) * 1e3, mirror_bytes=s.bin_info()["bytes"],
                  factor_bytes=s.bin_asym_info()["bytes"]))

    for nprobe in [int(v) for v in args.nprobe.split(",")]:
        truth = ctx.search(parent, s, q, nprobe, k, metric)[0]
        ctx.synchronize()
        truth = truth.cpu().numpy()

        def recall(call):
            got = call()[0]
            ctx.synchronize()
            got = got.cpu().numpy()
            return sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth)) / max(1, int((truth >= 0).sum()))

        srec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2], args.reps)
        emit(dict(case="search", nprobe=nprobe, kernel=ctx.last_scan_kernel(), **srec))
        fk8 = min(4 * k, QK_MAX_K)
        rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk8, metric, timing=True)[2], args.reps)
        emit(dict(case="sq8", nprobe=nprobe, fetch_k=fk8, kernel=ctx.last_scan_kernel(), **rec,
                  recall_at_k=recall(lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk8, metric))))
        for fk in FETCH:
            if fk < k:
                continue
            for case, asym in (("bin", False), ("asym", True)):
                rec = timed(ctx, lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, timing=True, asymmetric=asym)[2], args.reps)
                emit(dict(case=case, nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec,
                          recall_at_k=recall(lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, asymmetric=asym))))
    if out:
        out.close()


if __name__ == "__main__":
    main()
