"""Exact filtered search probe: what the exact call costs next to the probed calls and to the all-lists route, and what recall the
probed calls reach against it.  One JSON line per measurement to stdout and to --out:

    python scripts/exact_filter_probe.py [--shape recall|tenant|all] [--q 1024] [--reps 7] [--process NAME]
                                         [--all-lists-only] [--out profiles/exact_filter_probe.jsonl]

Shapes: recall = the corpus of adaptive_filter_probe.py's `recall` section (1M x 128 L2, 1024 lists, k 10) with uniform id sets of
selectivity 0.5 / 0.1 / 0.01 / 0.001; tenant = filter_probe.py's 10M x 128 shape (4096 lists) with id RANGES of 0.01 and 0.001.
Per filter: total_ms (HIP events through qk_timing, the median of --reps calls after two warm-ups) and recall@10 against the
exact answer of the fixed nprobe 8 call and of the adaptive call (8, 128); total_ms of the all-lists route
qk_search_filtered(parent = NULL); of the exact call in steady state; of its first use after a store change (mask build + gather
+ search) and behind a mask that is already current (gather + search: minus the steady call, the gather alone); the candidate
rows and the bytes of the candidate store.  --all-lists-only measures the all-lists route alone and uses nothing a tree without
the exact call lacks: run it from the parent commit's tree, alternating processes, for the comparison.  --process names the
process in every line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adaptive_filter_probe import recall_rows  # noqa: E402
from filter_probe import corpus, draw  # noqa: E402

SHAPES = {"recall": dict(n=1_000_000, nlist=1024, how="uniform", sels=[0.5, 0.1, 0.01, 0.001]),
          "tenant": dict(n=10_000_000, nlist=4096, how="ranges", sels=[0.01, 0.001])}


def median_total(fn, reps):
    for _ in range(2):
        fn()
    return float(np.median([fn()["total_ms"] for _ in range(reps)]))


def touch(s, nlist):
    """a table change that moves no row: an empty list comes and goes"""
    s.add_list(nlist + 7)
    s.remove_list(nlist + 7)
    s.publish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--process", default="tree")
    ap.add_argument("--all-lists-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from quake_amd import capi
    if not args.all_lists_only and not hasattr(capi.Context, "search_exact"):
        sys.exit("this tree has no exact filtered search: run with --all-lists-only")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(process=args.process, pid=os.getpid(), **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    d, metric, k, Q = 128, "l2", 10, args.q
    for shape, sh in SHAPES.items():
        if args.shape not in ("all", shape):
            continue
        n, nlist = sh["n"], sh["nlist"]
        s, parent, offsets, qall = corpus(ctx, n, d, nlist, metric, seed=1234)
        q = qall[:Q].contiguous()
        oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
        od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
        rng = np.random.default_rng(99)
        torch.cuda.synchronize()
        for sel in sh["sels"]:
            f = capi.Filter(s, draw(n, sel, sh["how"], rng), "allow")
            base = dict(shape=shape, n=n, nlist=nlist, d=d, q=Q, k=k, filter=sh["how"], selectivity=sel, rows=f.info()["rows_allowed"])
            all_lists = median_total(lambda: ctx.search(None, s, q, 1, k, metric, timing=True, out=(oi, od), filter=f)[2], args.reps)
            emit(dict(call="all lists (parent = NULL)", total_ms=all_lists, kernel=ctx.last_scan_kernel(), **base))
            if args.all_lists_only:
                f.close()
                continue
            ctx.synchronize()
            exact = oi.clone()
            steady = median_total(lambda: ctx.search_exact(s, q, k, metric, f, timing=True, out=(oi, od))[2], args.reps)
            ctx.synchronize()
            assert torch.equal(oi, exact), "the exact call and the all-lists route differ"
            info = f.exact_info()
            emit(dict(call="exact, steady", total_ms=steady, kernel=ctx.last_scan_kernel(), candidate_rows=info["rows"],
                      candidate_bytes=info["device_bytes"], **base))
            first, behind_mask = [], []
            for _ in range(3):
                touch(s, nlist)
                first.append(ctx.search_exact(s, q, k, metric, f, timing=True, out=(oi, od))[2]["total_ms"])
                touch(s, nlist)
                f.candidate_rows(ctx)  # (the mask is current again, the candidate store is not)
                behind_mask.append(ctx.search_exact(s, q, k, metric, f, timing=True, out=(oi, od))[2]["total_ms"])
            emit(dict(call="exact, first call after a store change", total_ms=float(np.median(first)),
                      gather_and_search_ms=float(np.median(behind_mask)), gather_ms=float(np.median(behind_mask)) - steady,
                      builds=f.exact_info()["builds"], **base))
            fixed = median_total(lambda: ctx.search(parent, s, q, 8, k, metric, timing=True, out=(oi, od), filter=f)[2], args.reps)
            ctx.synchronize()
            short, rec = recall_rows(oi, exact)
            emit(dict(call="fixed nprobe 8", total_ms=fixed, recall_at_k=rec, short_rows=short, **base))
            tms = []
            for i in range(2 + args.reps):
                gi, _, _, _, tm = ctx.search_adaptive(parent, s, q, 8, 128, k, metric, filter=f, probed=False)
                tms.append(tm["total_ms"])
            ctx.synchronize()
            short, rec = recall_rows(gi, exact)
            emit(dict(call="adaptive (8, 128)", total_ms=float(np.median(tms[2:])), recall_at_k=rec, short_rows=short, **base))
            f.close()
        s.close()
        parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
