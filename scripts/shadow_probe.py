"""The fp16 shadow form on bench.py's own indexes (the headline mixture and the low-intrinsic-dimension `hard` corpus), nprobe 1:
what the feedback chooses, the per-form phase times, the finish's counters, the shadow's build time and size.

    python scripts/shadow_probe.py [--corpus mixture|hard|both] [--quick] > profiles/shadow_probe.jsonl

One JSON line per corpus.  --quick: only the forced-mode step time (A/B of library variants through QUAKE_HIP_LIB)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402

SHADOW = "k_scan (fp16 shadow)"


def step_ms(ctx, parent, store, batches, k, metric, out, steps=100):
    for i in range(20):
        ctx.search(parent, store, batches[i % len(batches)], 1, k, metric, out=out)
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ctx.search(parent, store, batches[i % len(batches)], 1, k, metric, out=out)
    ctx.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def phases(ctx, parent, store, batches, k, metric):
    ctx.set_timing(1)
    acc = {}
    for b in batches * 3:
        t = ctx.search(parent, store, b, 1, k, metric, timing=True)[2]
        for key in ("coarse_ms", "group_ms", "scan_ms", "merge_ms", "total_ms", "scan_bytes"):
            acc[key] = acc.get(key, 0.0) + float(t[key]) / (3 * len(batches))
    ctx.set_timing(0)
    return {key: round(v, 5) for key, v in acc.items()}


def run(name, args, dev):
    from quake_amd.capi import Context
    n, d, nlist, k, Q, metric = args.nvec, 128, args.nlist, 10, 1024, "l2"
    ctx = Context(dev.index)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if name == "hard":
        x, basis = B.gen_manifold(n, d, seed=1, device=dev, latent=10)
    else:
        x, cent = B.gen_mixture(n, d, nlist, seed=1, device=dev, sigma=0.3)
    idx = B.build_single(ctx, dev, x, nlist, metric, 5, keep_host=False)
    parent, store = idx["parent"], idx["store"]
    if name == "hard":
        batches = [B.gen_manifold(Q, d, seed=2 + b, device=dev, latent=10, basis=basis)[0] for b in range(B.N_BATCHES)]
    else:
        batches = [B.gen_queries(Q, cent, seed=2 + b, device=dev, sigma=0.3) for b in range(B.N_BATCHES)]
    del x
    out = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
    res = {"corpus": name, "nvec": n, "nlist": nlist, "library": os.environ.get("QUAKE_HIP_LIB", "product")}
    # mode 0: the reference answers and the tile form's figures
    ctx.set_shadow(0)
    ref = []
    for b in batches:
        i, dd = ctx.search(parent, store, b, 1, k, metric)
        ref.append((i.clone(), dd.clone()))
    if not args.quick:
        res["tile_form"] = {"label": ctx.last_scan_kernel(), "step_ms": round(step_ms(ctx, parent, store, batches, k, metric, out), 5),
                            "phases": phases(ctx, parent, store, batches, k, metric)}
    # forced: the first call builds the shadow
    ctx.set_shadow(2)
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.search(parent, store, batches[0], 1, k, metric, out=out)
    ctx.synchronize()
    torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.search(parent, store, batches[0], 1, k, metric, out=out)
    ctx.synchronize()
    torch.cuda.synchronize()
    t_second = time.perf_counter() - t0
    res["shadow"] = dict(store.shadow_info(), build_ms=round(1e3 * (t_first - t_second), 3), arena_bytes=store.device_bytes())
    before = ctx.shadow_stats()
    equal = True
    for b, (ri, rd) in zip(batches, ref):
        i, dd = ctx.search(parent, store, b, 1, k, metric)
        equal = equal and bool((i == ri).all()) and bool((dd.view(torch.int32) == rd.view(torch.int32)).all())
    after = ctx.shadow_stats()
    nq = Q * len(batches)
    res["forced"] = {"label": ctx.last_scan_kernel(), "answers_equal_mode0": equal,
                     "queries": nq, "verified": after["verified"] - before["verified"], "fallback": after["fallback"] - before["fallback"],
                     "fallback_share": round((after["fallback"] - before["fallback"]) / nq, 6),
                     "candidates_per_query": round((after["candidates"] - before["candidates"]) / nq, 3),
                     "step_ms": round(step_ms(ctx, parent, store, batches, k, metric, out), 5)}
    if not args.quick:
        res["forced"]["phases"] = phases(ctx, parent, store, batches, k, metric)
        # automatic: what the feedback settles on (fresh context: its own figures)
        c2 = Context(dev.index)
        c2.set_stream(torch.cuda.current_stream().cuda_stream)
        labels = []
        for i in range(24):
            c2.search(parent, store, batches[i % len(batches)], 1, k, metric, out=out)
            c2.synchronize()
            labels.append(c2.last_scan_kernel())
        res["automatic"] = {"labels_of_the_first_24_calls": labels, "settled_on": labels[-1],
                            "step_ms": round(step_ms(c2, parent, store, batches, k, metric, out), 5)}
        c2.close()
    store.close()
    parent.close()
    ctx.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="both")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nvec", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    for name in (("mixture", "hard") if args.corpus == "both" else (args.corpus,)):
        run(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
