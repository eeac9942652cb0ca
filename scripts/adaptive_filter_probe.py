"""Adaptive-probing probe: what probing until min_candidates candidates buys a selective filter, and what it costs when it has
nothing to adapt.  One JSON line per measurement to stdout and to --out:

    python scripts/adaptive_filter_probe.py [--n 1000000] [--nlist 1024] [--q 1024] [--reps 7] [--out profiles/adaptive_filter_probe.jsonl]
                                            [--equal-n 10000000] [--equal-nlist 4096] [--equal-rounds 5] [--skip-recall] [--skip-equal]

recall   Seeded, one GPU, n x 128 L2, k 10: id filters of selectivity 0.5 / 0.1 / 0.01 / 0.001 (uniform ids), each alone, and one
         per-query batch that spreads the queries evenly over the four.  Per case: fixed nprobe 8, fixed nprobe 128 and the
         adaptive call (8, 128) with min_candidates k and 4k.  Recorded: the share of short rows (fewer than k results), recall@10
         against the exact filtered top-10 (the filtered search over ALL lists), mean / max nprobed, partitions_scanned, and the
         phase times of qk_timing (HIP events; medians over --reps calls after two warm-ups).
equal    The cost at max_nprobe == nprobe on scripts/filter_probe.py's bench128 shape (equal-n x 128, k 10, nprobe 1 and 8, uniform
         selectivity 0.1): qk_search_filtered next to the adaptive call, the median total_ms of --reps calls, --equal-rounds times
         over (the rounds' spread is the run-to-run spread).  The filtered half uses nothing a tree without the adaptive call
         lacks: run the script from the parent commit's tree for the yardstick."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filter_probe import corpus, draw  # noqa: E402

PHASES = ("coarse_ms", "group_ms", "scan_ms", "merge_ms", "total_ms")


def fixed_call(ctx, parent, s, q, nprobe, k, metric, kw, out=None):
    """one fixed-nprobe filtered search -> ((ids, dist), timing)"""
    r = ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=out, **kw)
    return r[:2], r[2]


def adaptive_call(ctx, parent, s, q, nprobe, max_nprobe, k, metric, mc, kw, nprobed=True):
    """one adaptive search -> ((ids, dist, nprobed, None), timing)"""
    r = ctx.search_adaptive(parent, s, q, nprobe, max_nprobe, k, metric, min_candidates=mc, probed=False, nprobed=nprobed, **kw)
    return r[:4], r[4]


def timed(fn, reps):
    """medians of every phase over reps calls after two warm-ups; fn returns (result tuple, timing dict)"""
    for _ in range(2):
        fn()
    tms = []
    for _ in range(reps):
        res, tm = fn()
        tms.append(tm)
    return res, {p: float(np.median([t[p] for t in tms])) for p in PHASES}, tms[-1]


def recall_rows(got, exact):
    """(share of rows with fewer than k results, recall@k against the exact rows: found / available)"""
    got, exact = got.cpu().numpy(), exact.cpu().numpy()
    short = float(((got >= 0).sum(1) < got.shape[1]).mean())
    hit = avail = 0
    for g, e in zip(got, exact):
        e = e[e >= 0]
        avail += e.shape[0]
        hit += np.isin(e, g[g >= 0]).sum()
    return short, float(hit / max(avail, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--equal-n", type=int, default=10_000_000)
    ap.add_argument("--equal-nlist", type=int, default=4096)
    ap.add_argument("--equal-rounds", type=int, default=5)
    ap.add_argument("--skip-recall", action="store_true")
    ap.add_argument("--skip-equal", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from quake_amd import capi
    adaptive = hasattr(capi.Context, "search_adaptive")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(tree="adaptive" if adaptive else "fixed nprobe only", **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    d, metric, k, Q = 128, "l2", 10, args.q
    if adaptive and not args.skip_recall:
        s, parent, offsets, qall = corpus(ctx, args.n, d, args.nlist, metric, seed=1234)
        q = qall[:Q].contiguous()
        rng = np.random.default_rng(99)
        sels = [0.5, 0.1, 0.01, 0.001]
        fs = [capi.Filter(s, draw(args.n, sel, "uniform", rng), "allow") for sel in sels]
        qf = (torch.arange(Q, device="cuda", dtype=torch.int32) % len(fs)).contiguous()
        torch.cuda.synchronize()  # (the context runs on its own stream: torch's inputs are complete before it reads them)
        cases = [("selectivity %g" % sel, dict(filter=f)) for sel, f in zip(sels, fs)] + [("mixed per query", dict(filters=fs, query_filter=qf))]
        n0, nmax = 8, 128
        for name, kw in cases:
            exact = ctx.search(parent, s, q, args.nlist, k, metric, **kw)[0]  # every list: the exact filtered top-k
            for nprobe in (n0, nmax):
                (gi, _), tm, last = timed(lambda: fixed_call(ctx, parent, s, q, nprobe, k, metric, kw), args.reps)
                short, rec = recall_rows(gi, exact)
                emit(dict(section="recall", case=name, call="fixed", nprobe=nprobe, n=args.n, nlist=args.nlist, q=Q, k=k, short_rows=short,
                          recall_at_k=rec, mean_nprobed=float(nprobe), max_nprobed=nprobe, partitions_scanned=int(last["partitions_scanned"]),
                          kernel=ctx.last_scan_kernel(), **tm))
            for mc in (k, 4 * k):
                (gi, _, gn, _), tm, last = timed(lambda: adaptive_call(ctx, parent, s, q, n0, nmax, k, metric, mc, kw), args.reps)
                short, rec = recall_rows(gi, exact)
                emit(dict(section="recall", case=name, call="adaptive", nprobe=n0, max_nprobe=nmax, min_candidates=mc, n=args.n,
                          nlist=args.nlist, q=Q, k=k, short_rows=short, recall_at_k=rec, mean_nprobed=float(gn.float().mean().item()),
                          max_nprobed=int(gn.max().item()), partitions_scanned=int(last["partitions_scanned"]),
                          kernel=ctx.last_scan_kernel(), **tm))
        for f in fs:
            f.close()
        s.close()
        parent.close()

    if not args.skip_equal:
        s, parent, offsets, qall = corpus(ctx, args.equal_n, d, args.equal_nlist, metric, seed=1234)
        q = qall[:Q].contiguous()
        rng = np.random.default_rng(99)
        f = capi.Filter(s, draw(args.equal_n, 0.1, "uniform", rng), "allow")
        oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for rnd in range(args.equal_rounds):
            for nprobe in (1, 8):
                _, tm, _ = timed(lambda: fixed_call(ctx, parent, s, q, nprobe, k, metric, dict(filter=f), out=(oi, od)), args.reps)
                emit(dict(section="equal", call="qk_search_filtered", round=rnd, nprobe=nprobe, n=args.equal_n, nlist=args.equal_nlist, q=Q,
                          k=k, selectivity=0.1, **tm))
                if adaptive:
                    _, tm, _ = timed(lambda: adaptive_call(ctx, parent, s, q, nprobe, nprobe, k, metric, k, dict(filter=f), nprobed=False),
                                     args.reps)
                    emit(dict(section="equal", call="qk_search_filtered_adaptive", round=rnd, nprobe=nprobe, max_nprobe=nprobe,
                              n=args.equal_n, nlist=args.equal_nlist, q=Q, k=k, selectivity=0.1, **tm))
        f.close()
        s.close()
        parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
