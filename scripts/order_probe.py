"""Cost of ordered search on the facet workload.  One JSON line per measurement to stdout and --out:

    python scripts/order_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--nprobe 8] [--radius 14.708] [--reps 7]
        [--cases range,stats,order,host] [--tag TAG] [--out profiles/order_probe.jsonl]

The workload of scripts/facet_stats_probe.py: 10M x 128 L2, nlist 4096 (the seeded corpus of
scripts/filter_probe.py), 1024 queries, nprobe 8, the radius that keeps about 1.6 % of the probed rows.  Two columns: 1 000 000
distinct values (value = (id % 1 000 000) * 1000003 - 7) and 16 values (the tie-heavy case: (key, id) decides almost every
comparison).  All calls run on the same index in the same process.  Medians over --reps calls after two warm-up calls, the phases
of a call from HIP events (qk_timing) and the whole call on the host clock behind a synchronisation.
  range   qk_range_search with cap = 0: the same emission scan; range's own counting (merge_ms) is the yardstick for the tail
  stats   qk_facet_stats_search of the large column without edges: the other single gathering sweep
  order   qk_order_search at k = 10 / 100 / 1024, ascending and descending, on both columns
  host    the route without ordered search: range_search with ids and distances (device tensors), both to the host, Attr.get,
          numpy.lexsort by (value, distance, id) per query, the first 10 -- wall clock only
`tail_ms` of a record is its total_ms minus the total_ms of `range`: what the call adds to the count-only range call.
The probe asserts nothing about time; it checks the values and distances of the first query of every ordered call against
the host route's order."""
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


def host_order(hl, hi, hd, vals, found, qi, k, desc):
    """(values, distances) of the first k hits of query qi by (value in the direction asked, distance, id) among those that have a
    value -- not the ids: two rows whose squared distances differ may report one float32 distance"""
    a, b = int(hl[qi]), int(hl[qi + 1])
    f = found[a:b]
    v, d, i = vals[a:b][f], hd[a:b][f], hi[a:b][f]
    vkey = -(v.astype(object)) if desc else v.astype(object)     # (Python ints: the negation of INT64_MIN must not wrap)
    o = sorted(range(v.shape[0]), key=lambda j: (vkey[j], d[j], i[j]))[:k]
    return v[o], d[o]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--radius", type=float, default=14.708)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="range,stats,order,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="lds_buffer")
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
    Q, n, nprobe, radius = args.q, args.n, args.nprobe, args.radius
    lims = ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0)[0]
    probed = ctx.range_search(parent, s, q, nprobe, float("inf"), "l2", cap=0)[0]
    ctx.synchronize()
    hits, rows = int(lims[Q].item()), int(probed[Q].item())
    emit(dict(case="setup", radius=radius, hits=hits, probed_rows=rows, kept=hits / max(rows, 1)))
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    cols = {}
    for name, card in (("1000000", 1_000_000), ("16", 16)):
        cols[name] = capi.Attr(s)
        cols[name].set(ids, (ids % card) * 1000003 - 7)
    ctx.synchronize()

    range_total = None
    if "range" in cases:
        rec = timed(ctx, lambda: ctx.range_search(parent, s, q, nprobe, radius, "l2", cap=0, timing=True, out=(None, None))[3], args.reps)
        range_total = rec["total_ms"]
        emit(dict(case="range_count_only", **rec))

    def tail(rec):
        return {} if range_total is None else dict(tail_ms=rec["total_ms"] - range_total)

    if "stats" in cases:
        rec = timed(ctx, lambda: ctx.facet_stats_search(parent, s, q, nprobe, radius, "l2", [cols["1000000"]], timing=True)[8], args.reps)
        emit(dict(case="facet_stats", columns="1000000", n_edges=[0], **rec, **tail(rec)))
    # the host route, also the check of the ordered calls' first query
    hl, hi, hd = ctx.range_search(parent, s, q, nprobe, radius, "l2")
    ctx.synchronize()
    hl, hi, hd = hl.cpu().numpy(), hi.cpu().numpy(), hd.cpu().numpy()
    if "order" in cases:
        for name in ("1000000", "16"):
            vals, found = cols[name].get(hi)
            for k in (10, 100, 1024):
                for desc in (False, True):
                    res = {}

                    def call():
                        o = ctx.order_search(parent, s, q, nprobe, radius, "l2", cols[name], k, descending=desc, timing=True)
                        res["out"] = o
                        return o[6]

                    rec = timed(ctx, call, args.reps)
                    ctx.synchronize()
                    o = res["out"]
                    assert int(o[5].sum().item()) == hits
                    wv, wd = host_order(hl, hi, hd, vals, found, 0, k, desc)
                    m = wv.shape[0]
                    assert (o[2][0].cpu().numpy()[:m] == wv).all() and (o[1][0].cpu().numpy()[:m] == wd).all()
                    assert (o[0][0].cpu().numpy()[m:] == -1).all()
                    emit(dict(case="order_search", columns=name, k=k, descending=desc, **rec, **tail(rec)))
    if "host" in cases:
        col = cols["1000000"]
        wall = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            rl, ri, rd = ctx.range_search(parent, s, q, nprobe, radius, "l2")
            ctx.synchronize()
            rl, ri, rd = rl.cpu().numpy(), ri.cpu().numpy(), rd.cpu().numpy()
            vals, found = col.get(ri)
            for i in range(Q):
                a, b = rl[i], rl[i + 1]
                f = found[a:b]
                o = np.lexsort((ri[a:b][f], rd[a:b][f], vals[a:b][f]))[:10]
                first = ri[a:b][f][o]
            wall.append((time.perf_counter() - t0) * 1e3)
        emit(dict(case="host_route", columns="1000000", k=10, queries=Q, ids_to_host=int(ri.shape[0]), wall_ms=float(np.median(wall))))
    for c in cols.values():
        c.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
