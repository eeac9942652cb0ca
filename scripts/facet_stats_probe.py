"""Cost of facet statistics on the bench corpus shape.  One JSON line per measurement to stdout and --out:

    python scripts/facet_stats_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--nprobe 8] [--keep 0.01] [--reps 7]
        [--cases range,facet,stats,host] [--tag TAG] [--out profiles/facet_stats_probe.jsonl]

The workload of scripts/facet_probe.py: 10M x 128 L2, nlist 4096 (the seeded corpus of scripts/filter_probe.py), 1024 queries,
nprobe 8, a radius that keeps about 1.6 % of the probed rows (the --keep quantile of the distances a sample of the queries sees).
The column has 1 000 000 distinct values (value = (id % 1 000 000) * 1000003 - 7): the case facet statistics exist for.  All calls
run on the same index in the same process.  Medians over --reps calls after two warm-up calls, the phases of a call from HIP events
(qk_timing) and the whole call on the host clock behind a synchronisation.
  range   qk_range_search with cap = 0 for the same arguments: the same emission scan, and range's own counting (merge_ms) as the
          yardstick for the tail
  facet   qk_facet_search of the column, n_values = 10
  stats   qk_facet_stats_search of the column with 0, 16 and 255 edges, and of four columns (1 000 000 / 10 000 / 100 / 16 values,
          16 edges each) in one call
  host    the route without facet statistics: range_search with ids (device tensors), the ids to the host, Attr.get, then numpy
          min / max / sum / searchsorted per query with 16 edges -- wall clock only
`tail_ms` of a record is its total_ms minus the total_ms of `range`: what the call adds to the count-only range call.  The two
variants of k_facet_stats are two libraries: the product build (register accumulation, one global atomic per statistic and
workgroup) and a side build with -DQK_FACET_STATS_HIT_ATOMICS=1 (every hit issues its own global atomics):
    python -c "from quake_amd.build import build_lib; build_lib(variant='facet_stats_hit', extra_flags=['-DQK_FACET_STATS_HIT_ATOMICS=1'])"
    QUAKE_HIP_LIB=quake_amd/lib/libquake_hip_facet_stats_hit.so python scripts/facet_stats_probe.py --tag per_hit_atomics --cases range,stats
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
    ap.add_argument("--cases", default="range,facet,stats,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="register_accumulation")
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
    cards = [("1000000", 1_000_000), ("10000", 10_000), ("100", 100), ("16", 16)]
    cols = {}
    for name, card in cards:
        cols[name] = capi.Attr(s)
        cols[name].set(ids, (ids % card) * 1000003 - 7)
    ctx.synchronize()

    def edges_of(card, E):
        """E ascending edges spread over the column's values"""
        top = (card - 1) * 1000003 - 7
        return sorted({int(x) for x in np.linspace(-7, top, E + 2)[1:-1]}) if E else []

    range_total = None
    if "range" in cases:
        rec = timed(ctx, lambda: ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0, timing=True, out=(None, None))[3], args.reps)
        range_total = rec["total_ms"]
        emit(dict(case="range_count_only", **rec))

    def tail(rec):
        return {} if range_total is None else dict(tail_ms=rec["total_ms"] - range_total)

    if "facet" in cases:
        bufs = (torch.empty((1, Q, 10), dtype=torch.int64, device="cuda"), torch.empty((1, Q, 10), dtype=torch.int64, device="cuda"),
                torch.empty((1, Q), dtype=torch.int64, device="cuda"), torch.empty((1, Q), dtype=torch.int64, device="cuda"),
                torch.empty((Q,), dtype=torch.int64, device="cuda"))
        rec = timed(ctx, lambda: ctx.facet_search(parent, s, q, nprobe, radius, "l2", [cols["1000000"]], n_values=10, timing=True,
                                                  out=bufs)[5], args.reps)
        ctx.synchronize()
        assert int(bufs[4].sum().item()) == hits
        emit(dict(case="facet_counts", columns="1000000", **rec, **tail(rec)))
    if "stats" in cases:
        runs = [(["1000000"], E) for E in (0, 16, 255)] + [([name for name, _ in cards], 16)]
        for names, E in runs:
            edges = [edges_of(dict(cards)[k], E) for k in names]
            assert all(len(e) == min(E, len(e)) for e in edges)
            res = {}

            def call():
                o = ctx.facet_stats_search(parent, s, q, nprobe, radius, "l2", [cols[k] for k in names], edges=edges, timing=True)
                res["out"] = o
                return o[8]

            rec = timed(ctx, call, args.reps)
            ctx.synchronize()
            o = res["out"]
            assert int(o[7].sum().item()) == hits and int(o[0][0].sum().item()) == hits and int(o[6][0].sum().item()) == hits
            emit(dict(case="facet_stats", columns="+".join(names), n_edges=[len(e) for e in edges], **rec, **tail(rec)))
    if "host" in cases:
        col = cols["1000000"]
        e16 = np.array(edges_of(1_000_000, 16), np.int64)
        wall = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            hl, hi, _ = ctx.range_search(parent, s, q, nprobe, radius, "l2")
            ctx.synchronize()
            hl, hi = hl.cpu().numpy(), hi.cpu().numpy()
            vals, found = col.get(hi)
            for i in range(Q):
                v = vals[hl[i]:hl[i + 1]][found[hl[i]:hl[i + 1]]]
                if v.shape[0]:
                    lo, up, sm = v.min(), v.max(), int(v.sum())   # (these values cannot leave int64: numpy's sum is exact here)
                hist = np.bincount(np.searchsorted(e16, v, side="right"), minlength=17)
            wall.append((time.perf_counter() - t0) * 1e3)
        emit(dict(case="host_route", columns="1000000", n_edges=[16], queries=Q, ids_to_host=int(hi.shape[0]), wall_ms=float(np.median(wall))))
    for c in cols.values():
        c.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
