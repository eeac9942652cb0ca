"""Cost of facet counts on the bench corpus shape.  One JSON line per measurement to stdout and --out:

    python scripts/facet_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--nprobe 8] [--keep 0.01] [--reps 7]
        [--cases range,facet,host] [--tag TAG] [--out profiles/facet_probe.jsonl]

10M x 128 L2, nlist 4096 (the seeded corpus of scripts/filter_probe.py), 1024 queries, nprobe 8, a radius that keeps about --keep of
the probed rows (the --keep quantile of the distances a sample of the queries sees).  Columns of 16, 10 000 and 1 000 000 distinct
values (value = id % cardinality, times a constant) and a fourth of 100.  Medians over --reps calls after two warm-up calls, the
phases of a call from HIP events (qk_timing) and the whole call on the host clock behind a synchronisation.
  range   qk_range_search with cap = 0 for the same arguments: the same emission scan, and range's own counting as the yardstick for
          the tail (merge_ms)
  facet   qk_facet_search for each column alone and for all four in one call, n_values = 10
  host    the route without facet counts, for the 16-value column: range_search with ids (device tensors), the ids to the host,
          Attr.get and numpy.unique per query -- wall clock only
The two variants of k_facet_count are two libraries: the product build (one atomic per hit and column) and a side build with
-DQK_FACET_WAVE_AGG=1 (equal values of a wave added up in registers first):
    python -c "from quake_amd.build import build_lib; build_lib(variant='facet_agg', extra_flags=['-DQK_FACET_WAVE_AGG=1'])"
    QUAKE_HIP_LIB=quake_amd/lib/libquake_hip_facet_agg.so python scripts/facet_probe.py --tag wave_aggregation --cases facet ...
The probe asserts nothing about time."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="range,facet,host")
    ap.add_argument("--host-queries", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="per_lane_atomics")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from quake_amd import capi
    from scripts.filter_probe import corpus  # (the same seeded corpus)
    cases = args.cases.split(",")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = dict(tag=args.tag, lib=os.path.basename(os.environ.get("QUAKE_HIP_LIB") or "libquake_hip.so"), n=args.n, d=args.d,
                   nlist=args.nlist, q=args.q, nprobe=args.nprobe, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    s, parent, offsets, qall = corpus(ctx, args.n, args.d, args.nlist, "l2", seed=1234)
    q = qall[: args.q].contiguous()
    Q, n, nprobe = args.q, args.n, args.nprobe
    # the radius: the --keep quantile of the distances 16 of the queries see in their probed lists
    lims, _, dist = ctx.range_search(parent, s, q[:16].contiguous(), nprobe, float("inf"), "l2")
    ctx.synchronize()
    radius = float(torch.quantile(dist[: 4_000_000].float(), args.keep).item())
    lims = ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0)[0]
    probed = ctx.range_search(parent, s, q, nprobe, float("inf"), "l2", cap=0)[0]
    ctx.synchronize()
    hits, rows = int(lims[Q].item()), int(probed[Q].item())
    emit(dict(case="setup", radius=radius, hits=hits, probed_rows=rows, kept=hits / max(rows, 1)))
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    cards = [("16", 16), ("10000", 10_000), ("1000000", 1_000_000), ("100", 100)]
    cols = {}
    for name, card in cards:
        cols[name] = capi.Attr(s)
        cols[name].set(ids, (ids % card) * 1000003 - 7)
    ctx.synchronize()
    if "range" in cases:
        rec = timed(ctx, lambda: ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0, timing=True, out=(None, None))[3], args.reps)
        emit(dict(case="range_count_only", **rec))
    if "facet" in cases:
        runs = [([name], name) for name, _ in cards[:3]] + [([name for name, _ in cards], "all four")]
        for names, label in runs:
            C_ = len(names)
            bufs = (torch.empty((C_, Q, 10), dtype=torch.int64, device="cuda"), torch.empty((C_, Q, 10), dtype=torch.int64, device="cuda"),
                    torch.empty((C_, Q), dtype=torch.int64, device="cuda"), torch.empty((C_, Q), dtype=torch.int64, device="cuda"),
                    torch.empty((Q,), dtype=torch.int64, device="cuda"))
            rec = timed(ctx, lambda: ctx.facet_search(parent, s, q, nprobe, radius, "l2", [cols[k] for k in names], n_values=10, timing=True,
                                                      out=bufs)[5], args.reps)
            ctx.synchronize()
            assert int(bufs[4].sum().item()) == hits
            emit(dict(case="facet", columns=label, distinct_mean=float(bufs[2].float().mean().item()), **rec))
    if "host" in cases:
        nq = min(args.host_queries, Q)
        col = cols["16"]
        wall = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            hl, hi, _ = ctx.range_search(parent, s, q[:nq].contiguous(), nprobe, radius, "l2")
            ctx.synchronize()
            hl, hi = hl.cpu().numpy(), hi.cpu().numpy()
            vals, found = col.get(hi)
            for i in range(nq):
                v = vals[hl[i]:hl[i + 1]][found[hl[i]:hl[i + 1]]]
                uv, uc = np.unique(v, return_counts=True)
                order = np.lexsort((uv, -uc))[:10]
            wall.append((time.perf_counter() - t0) * 1e3)
        emit(dict(case="host_route", columns="16", queries=nq, ids_to_host=int(hi.shape[0]), wall_ms=float(np.median(wall)),
                  wall_ms_scaled_to_batch=float(np.median(wall)) / nq * Q))
    for c in cols.values():
        c.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
