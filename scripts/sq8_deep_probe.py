"""Cost and recall of deep quantized search (deep=True: candidates by counting) against search() and the pool form on one index.
One JSON line per measurement to stdout and --out:

    python scripts/sq8_deep_probe.py [--n 10000000] [--d 128] [--metric l2] [--nlist 4096] [--q 1024] [--nprobe 1,8,16] [--k 10]
        [--reps 5] [--out profiles/sq8_deep_probe.jsonl]

The seeded corpus and the timing of scripts/sq8_probe.py (medians over --reps calls after two warm-up calls, phases from HIP events).
  search   qk_search at k: the yardstick of time and recall
  pool     qk_sq8_search at fetch_k = k, 2k, 4k as far as QK_MAX_K allows
  deep     qk_sq8_search_deep at fetch_k = k, 2k, 4k, 1000, 4096: scan_ms = bound + pass A + cut + pass B, finish_ms = resolve + exact
           finish (+ the query coding), recall@k against search()'s own answer at the same nprobe
The tie path of the resolve is a branch inside k_sq8_resolve, not a launch: a call that does not need it pays nothing a separate
figure could show.  The probe asserts nothing about time."""
import argparse
import json
import os
import sys


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from quake_amd import capi
    from quake_amd._lib import QK_MAX_K
    from scripts.filter_probe import corpus
    from scripts.sq8_probe import timed
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
        for deep, fks in ((False, (k, 2 * k, 4 * k)), (True, (k, 2 * k, 4 * k, 1000, 4096))):
            for fk in sorted(set(f for f in fks if f >= k and (deep or f <= QK_MAX_K))):
                rec = timed(ctx, lambda: ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, timing=True, deep=deep)[2], args.reps)
                emit(dict(case="deep" if deep else "pool", nprobe=nprobe, fetch_k=fk, kernel=ctx.last_scan_kernel(), **rec,
                          total_ms_vs_search=rec["total_ms"] / srec["total_ms"],
                          recall_at_k=recall(ctx.sq8_search(parent, s, q, nprobe, k, fk, metric, deep=deep)[0], truth)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
