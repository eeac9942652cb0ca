"""Cost of multi-vector rerank on the workload of scripts/maxsim_probe.py.  One JSON line per measurement to stdout and --out:

    python scripts/maxsim_rerank_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--shapes 32x32,128x8,2048x8] [--cands 100,1000]
        [--doc-rows 32] [--k 10] [--reps 7] [--cases rerank,emission,host] [--tag TAG] [--out profiles/maxsim_rerank_probe.jsonl]

10M x 128 L2, nlist 4096 (the seeded corpus of scripts/filter_probe.py); the document column gives --doc-rows consecutive ids one
value.  A shape LxT is L logical queries of T sub-queries (the query set repeated where L * T exceeds it).  The candidates of a
logical query are the documents of the nearest rows of its sub-queries (qk_search, nprobe 8), filled up with further documents to C
distinct values.  Medians over --reps calls after two warm-up calls; phases from HIP events (qk_timing), the call on the host clock.
  rerank    qk_maxsim_rerank: scan_ms = the sweep, merge_ms = score + select; gathered_tb_s = scan_bytes / merge_ms (the gather of
            k_funnel_finish is on record with 0.8 TB/s); mfma_tflops = gathered rows x padded tokens x padded d x 2 / merge_ms, the
            executed fp32 MFMA work
  emission  the route without it, measured in the same job: qk_maxsim_search at radius +inf and nprobe 1 -- every (token, row) pair
            of the probed list through the tables (it scores the probed rows only, not whole documents)
  host      the host route: the caller's own map document -> ids (no call returns the ids that share a column value),
            Store.get_vectors, float32 matmul, maximum per token, sum -- wall clock only, C = the smallest of --cands
The probe asserts nothing about time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

PHASES = ("scan_ms", "merge_ms", "total_ms")


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
    rec["scan_bytes"] = int(rows[-1]["scan_bytes"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--shapes", default="32x32,128x8,2048x8")
    ap.add_argument("--cands", default="100,1000")
    ap.add_argument("--doc-rows", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="rerank,emission,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="rerank")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from quake_amd import capi
    from scripts.filter_probe import corpus  # (the same seeded corpus)
    cases = args.cases.split(",")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(tag=args.tag, n=args.n, d=args.d, nlist=args.nlist, doc_rows=args.doc_rows, **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, _, qall = corpus(ctx, args.n, args.d, args.nlist, "l2", seed=1234)
    ids = torch.arange(args.n, device="cuda", dtype=torch.int64)
    doc = capi.Attr(s)
    doc.set(ids, ids // args.doc_rows)
    ctx.synchronize()
    ndocs = args.n // args.doc_rows
    dpad = (args.d + 15) // 16 * 16
    cands = [int(c) for c in args.cands.split(",")]
    for shape in args.shapes.split(","):
        L, T = (int(v) for v in shape.split("x"))
        q = qall.repeat((L * T + qall.shape[0] - 1) // qall.shape[0], 1)[: L * T].contiguous()
        q3 = q.reshape(L, T, args.d)
        tpad = (T + 15) // 16 * 16
        near = ctx.search(parent, s, q, 8, 64, "l2")[0]
        ctx.synchronize()
        for C in cands:
            base = dict(shape=shape, L=L, T=T, C=C)
            # C distinct documents per logical query: those of its nearest rows first, then the documents behind the first one
            cand = torch.empty((L, C), dtype=torch.int64, device="cuda")
            for l in range(L):
                d0 = torch.unique(near[l * T:(l + 1) * T].reshape(-1).clamp_min(0) // args.doc_rows)[:C]
                fill = (d0[0] + 1 + torch.arange(2 * C, device="cuda")) % ndocs
                cand[l] = torch.cat([d0, fill[~torch.isin(fill, d0)]])[:C]
            torch.cuda.synchronize()
            if "rerank" in cases:
                rec = timed(ctx, lambda: ctx.maxsim_rerank(s, q3, "l2", doc, cand, args.k, 100.0, timing=True)[5], args.reps)
                rows = rec["scan_bytes"] / (dpad * 4)
                rec["gathered_tb_s"] = rec["scan_bytes"] / (rec["merge_ms"] * 1e-3) / 1e12
                rec["mfma_tflops"] = rows * tpad * dpad * 2 / (rec["merge_ms"] * 1e-3) / 1e12
                emit(dict(case="rerank", k=args.k, **base, **rec))
            if "host" in cases and C == min(cands) and L * C <= 20000:
                wall = []
                for _ in range(3):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    rid = (cand.cpu().numpy()[:, :, None] * args.doc_rows + np.arange(args.doc_rows)).reshape(-1)
                    v = s.get_vectors(rid)[0].reshape(L, C, args.doc_rows, args.d)
                    qh = q3.cpu().numpy()
                    sim = np.einsum("ltd,lcrd->lctr", qh, v)
                    d2 = (qh * qh).sum(-1)[:, None, :, None] + (v * v).sum(-1)[:, :, None, :] - 2 * sim
                    sc = np.sqrt(np.maximum(d2, 0)).min(-1).sum(-1)
                    np.argsort(sc, axis=1)[:, : args.k]
                    wall.append((time.perf_counter() - t0) * 1e3)
                emit(dict(case="host_route", k=args.k, vectors_to_host=int(rid.shape[0]), wall_ms=float(np.median(wall)), **base))
        if "emission" in cases and L * T <= 4096:
            rec = timed(ctx, lambda: ctx.maxsim_search(parent, s, q3, 1, float("inf"), "l2", doc, args.k, 100.0, timing=True)[5], args.reps)
            emit(dict(case="emission_route", k=args.k, shape=shape, L=L, T=T, nprobe=1, radius="inf", **rec))
    doc.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
