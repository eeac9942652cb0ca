"""Cost of multi-vector search on the facet workload.  One JSON line per measurement to stdout and --out:

    python scripts/maxsim_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--nprobe 8] [--radius 14.708] [--shapes 32x32,128x8]
        [--doc-rows 32] [--k 10] [--reps 7] [--cases range,facet,maxsim,host,wide] [--tag TAG] [--out profiles/maxsim_probe.jsonl]

The workload of scripts/facet_probe.py: 10M x 128 L2, nlist 4096 (the seeded corpus of scripts/filter_probe.py),
nprobe 8, the radius that keeps about 1.6 % of the probed rows.  The document column gives --doc-rows consecutive ids one value
(id // 32: 312 500 documents).  A shape LxT is L logical queries of T sub-queries, the first L * T queries of the corpus' query
set.  All calls run on the same index in the same process.  Medians over --reps calls after two warm-up calls, the phases of a
call from HIP events (qk_timing) and the whole call on the host clock behind a synchronisation.
  range   qk_range_search with cap = 0 over the L * T sub-queries: the same emission scan -- the floor; `tail_ms` of every other
          record is its total_ms minus this one's
  facet   qk_facet_search of the document column over the same sub-queries, n_values = 10: the nearest existing aggregation
  maxsim  qk_maxsim_search, k = --k, missing = the radius
  host    the route without it: range_search with ids and distances, both to the host, Attr.get, a numpy group-by per logical
          query (minimum per (document, sub-query), sums in sub-query order, the k smallest) -- wall clock only
  wide    maxsim and range at radius +inf and nprobe 1: every probed row is a hit
A call the library refuses is recorded with its message (`refused`) and the probe goes on.  The probe asserts nothing about
time; it checks the maxsim call's rows against the host route's."""
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


def host_group_by(rl, ri, rd, vals, found, L, T, k, missing):
    """(groups [L, k], scores [L, k]) by numpy: the definition of the header for L2, padding 0 / +inf"""
    groups = np.zeros((L, k), np.int64)
    scores = np.full((L, k), np.inf, np.float32)
    for l in range(L):
        per_t = []
        for t in range(T):
            a, b = rl[l * T + t], rl[l * T + t + 1]
            f = found[a:b]
            g, d = vals[a:b][f], rd[a:b][f]
            u, inv = np.unique(g, return_inverse=True)
            best = np.full(u.shape[0], np.inf, np.float32)
            np.minimum.at(best, inv, d)
            per_t.append((u, best))
        docs = np.unique(np.concatenate([u for u, _ in per_t] + [np.zeros(0, np.int64)]))
        s = np.zeros(docs.shape[0], np.float32)
        for u, best in per_t:
            term = np.full(docs.shape[0], np.float32(missing), np.float32)
            term[np.searchsorted(docs, u)] = best
            s = (s + term).astype(np.float32)
        o = np.lexsort((docs, s))[:k]
        groups[l, :o.shape[0]], scores[l, :o.shape[0]] = docs[o], s[o]
    return groups, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--radius", type=float, default=14.708)
    ap.add_argument("--shapes", default="32x32,128x8")
    ap.add_argument("--doc-rows", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="range,facet,maxsim,host,wide")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="tables_per_logical_query")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from quake_amd import capi
    from quake_amd._lib import QuakeHipError
    from scripts.filter_probe import corpus  # (the same seeded corpus)
    cases = args.cases.split(",")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = dict(tag=args.tag, lib=os.path.basename(os.environ.get("QUAKE_HIP_LIB") or "libquake_hip.so"), n=args.n, d=args.d,
                   nlist=args.nlist, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, "l2", seed=1234)
    ids = torch.arange(args.n, device="cuda", dtype=torch.int64)
    doc = capi.Attr(s)
    doc.set(ids, ids // args.doc_rows)
    ctx.synchronize()
    k, inf = args.k, float("inf")
    for shape in args.shapes.split(","):
        L, T = (int(v) for v in shape.split("x"))
        q = qall[: L * T].contiguous()
        q3 = q.reshape(L, T, args.d)
        for nprobe, radius, wide in ((args.nprobe, args.radius, False), (1, inf, True)):
            if wide and "wide" not in cases:
                continue
            base = dict(shape=shape, L=L, T=T, nprobe=nprobe, radius=radius if not wide else "inf")
            lims = ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0)[0]
            ctx.synchronize()
            hits = int(lims[L * T].item())
            emit(dict(case="setup", hits=hits, documents=args.n // args.doc_rows, **base))
            range_total = None
            if "range" in cases:
                rec = timed(ctx, lambda: ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0, timing=True, out=(None, None))[3], args.reps)
                range_total = rec["total_ms"]
                emit(dict(case="range_count_only", **base, **rec))

            def tail(rec):
                return {} if range_total is None else dict(tail_ms=rec["total_ms"] - range_total)

            if "facet" in cases and not wide:
                rec = timed(ctx, lambda: ctx.facet_search(parent, s, q, nprobe, radius, "l2", [doc], 10, timing=True)[5], args.reps)
                emit(dict(case="facet_search", n_values=10, **base, **rec, **tail(rec)))
            res = {}
            if "maxsim" in cases:
                missing = radius if not wide else 100.0

                def call():
                    o = ctx.maxsim_search(parent, s, q3, nprobe, radius, "l2", doc, k, missing, timing=True)
                    res["out"] = o
                    return o[5]

                try:
                    rec = timed(ctx, call, args.reps)
                except QuakeHipError as err:   # a shape the call refuses is a finding: recorded, and the probe goes on
                    res.pop("out", None)
                    emit(dict(case="maxsim_search", k=k, refused=str(err), **base))
                else:
                    ctx.synchronize()
                    o = res["out"]
                    assert int(o[4].sum().item()) == hits
                    emit(dict(case="maxsim_search", k=k, n_groups_mean=float(o[3].float().mean().item()), **base, **rec, **tail(rec)))
            if "host" in cases and not wide:
                wall = []
                for _ in range(3):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    rl, ri, rd = ctx.range_search(parent, s, q, nprobe, radius, "l2")
                    ctx.synchronize()
                    rl, ri, rd = rl.cpu().numpy(), ri.cpu().numpy(), rd.cpu().numpy()
                    vals, found = doc.get(ri)
                    hg, hs = host_group_by(rl, ri, rd, np.asarray(vals), np.asarray(found, bool), L, T, k, radius)
                    wall.append((time.perf_counter() - t0) * 1e3)
                if "out" in res:
                    assert (res["out"][0].cpu().numpy() == hg).all() and (res["out"][1].cpu().numpy() == hs).all()
                emit(dict(case="host_route", k=k, ids_to_host=int(ri.shape[0]), wall_ms=float(np.median(wall)), **base))
    doc.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
