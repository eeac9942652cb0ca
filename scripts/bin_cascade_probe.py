"""Cost and recall of rescored binary search (binary_search with rescore_k: bits -> int8 -> float32) against search(), binary search
and quantized search on one index.  One JSON line per measurement to stdout and --out:

    python scripts/bin_cascade_probe.py [--n 10000000] [--d 768] [--metric ip] [--nlist 4096] [--q 1024] [--nprobe 1] [--k 100]
        [--reps 5] [--out profiles/bin_cascade_probe.jsonl]

The seeded corpus of scripts/filter_probe.py (clustered Gaussian rows, not trained embeddings).  All calls run on the same index in
one process.  Medians over --reps calls after two warm-up calls; the phases of a call from HIP events (qk_timing), the whole call on
the host clock behind a synchronisation.  recall@k is against search()'s own answer at the same nprobe, taken from two separate
calls (`recall_at_k`, `recall_at_k_repeat`: the results are defined bit for bit, so the two agree unless something is wrong).
  search     qk_search at k: the yardstick
  sq8        qk_sq8_search at fetch_k = min(4k, 448)
  bin        qk_bin_search at fetch_k = k, 2k, 448, 400, 1000, 4096: `select_ms` = scan_ms (k_bin_select), `tail_ms` = total_ms minus
             the phases up to the select = the exact finish over fetch_k candidates
  cascade    qk_bin_search_rescored at fetch_k = 400, 1000, 4096 x rescore_k = k, 2k, 448: `tail_ms` = k_sq8_rerank + the exact finish
             over rescore_k candidates.  The two are not separated by events of their own: `finish_ms_est` is the tail of the `bin`
             call at fetch_k = rescore_k in the same job (the same finish kernel over as many candidates), `rerank_ms_est` the
             difference, `rerank_gather_gbps` = `rerank_candidates` (an upper bound: min(q x fetch_k, probed rows)) x
             (64 ceil(d / 64) + 4) bytes over it.
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
    rec["total_ms_min"], rec["total_ms_max"] = float(min(r["total_ms"] for r in rows)), float(max(r["total_ms"] for r in rows))
    rec["tail_ms"] = rec["total_ms"] - rec["coarse_ms"] - rec["group_ms"] - rec["scan_ms"] - rec["merge_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--metric", default="ip")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", default="1")
    ap.add_argument("--k", type=int, default=100)
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
    k, metric, d = args.k, args.metric, args.d
    row_bytes = 64 * ((d + 63) // 64) + 4

    for nprobe in [int(v) for v in args.nprobe.split(",")]:
        truth = ctx.search(parent, s, q, nprobe, k, metric)[0]
        ctx.synchronize()
        truth = truth.cpu().numpy()

        def recall(call):
            both = []
            for _ in range(2):
                got = call()[0]
                ctx.synchronize()
                got = got.cpu().numpy()
                both.append(sum(len(set(g[g >= 0].tolist()) & set(t[t >= 0].tolist())) for g, t in zip(got, truth)) / max(1, int((truth >= 0).sum())))
            return dict(recall_at_k=both[0], recall_at_k_repeat=both[1])

        srec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2], args.reps)
        emit(dict(case="search", nprobe=nprobe, kernel=ctx.last_scan_kernel(), **srec))
        fk8 = min(4 * k, QK_MAX_K)
        rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk8, metric, timing=True)[2], args.reps)
        emit(dict(case="sq8", nprobe=nprobe, fetch_k=fk8, kernel=ctx.last_scan_kernel(), **rec, total_ms_vs_search=rec["total_ms"] / srec["total_ms"],
                  **recall(lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk8, metric))))
        rks = sorted({k, 2 * k, QK_MAX_K})
        bins = {}
        for fk in sorted(set(rks) | {400, 1000, 4096}):
            if fk < k:
                continue
            rec = timed(ctx, lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, timing=True)[2], args.reps)
            bins[fk] = rec
            emit(dict(case="bin", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec, select_ms=rec["scan_ms"],
                      total_ms_vs_search=rec["total_ms"] / srec["total_ms"], **recall(lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric))))
        for fk in (400, 1000, 4096):
            for rk in rks:
                if not k <= rk <= fk:
                    continue
                rec = timed(ctx, lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, timing=True, rescore_k=rk)[2], args.reps)
                rerank = rec["tail_ms"] - bins[rk]["tail_ms"]
                # (candidates: at most fetch_k per query and at most the probed rows, which scan_bytes counts at 16 ceil(d / 128) bytes)
                cands = min(args.q * fk, rec["scan_bytes"] // (16 * ((d + 127) // 128)))
                emit(dict(case="cascade", nprobe=nprobe, fetch_k=fk, rescore_k=rk, kernel=ctx.last_scan_kernel(), **rec, select_ms=rec["scan_ms"],
                          finish_ms_est=bins[rk]["tail_ms"], rerank_ms_est=rerank,
                          rerank_candidates=cands, rerank_gather_gbps=cands * row_bytes / max(rerank, 1e-6) / 1e6,
                          total_ms_vs_search=rec["total_ms"] / srec["total_ms"], total_ms_vs_bin=rec["total_ms"] / bins[fk]["total_ms"],
                          **recall(lambda: ctx.bin_search(parent, s, q, nprobe, k, fk, metric, rescore_k=rk))))
    if out:
        out.close()


if __name__ == "__main__":
    main()
