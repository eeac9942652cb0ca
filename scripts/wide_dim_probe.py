"""Wide-row probe: how the wide-row kernels (qk_scan_wide.hip) use the MI355X at d = 3072 / 4096, with today's k_scan at d = 2048
as the calibration point.  One JSON line per (corpus, k, nprobe) to stdout and to --out:

    python scripts/wide_dim_probe.py [--n 1000000] [--nlist 1024] [--q 1024] [--reps 5] [--out profiles/wide_dim_probe.jsonl]

Corpora (seeded, generated on the device): n x 4096 L2, n x 3072 IP, n x 2048 L2 (calibration).  Lists come from one nearest-
centroid assign of every row against nlist sampled rows (that assign is the k-means assign figure: 2 n nlist d flops).  Figures:
  scan_frac_hbm    unique probed bytes (qk_timing.scan_bytes) / scan kernel time / 8 TB/s
  coarse_frac_mfma 2 Q nlist d / coarse time / 157.3 TFLOP/s (fp32 MFMA peak)
  assign_frac_mfma 2 n nlist d / assign time / 157.3 TFLOP/s
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/wide_dim_probe.py ...` for the per-kernel summary.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
MFMA_F32_PEAK = 157.3e12


def corpus(ctx, n, d, nlist, metric, seed):
    from quake_amd.capi import Store
    g = torch.Generator(device="cuda").manual_seed(seed)
    nc = 4 * nlist
    cent = torch.randn(nc, d, device="cuda", generator=g)
    x = cent[torch.randint(0, nc, (n,), device="cuda", generator=g)]
    x.add_(0.5 * torch.randn(n, d, device="cuda", generator=g))
    if metric == "ip":
        x /= x.norm(dim=1, keepdim=True)
    lists = x[torch.randperm(n, device="cuda", generator=g)[:nlist]].contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ctx.kmeans_assign_only(x[:1024], lists, metric)  # (first call: function attributes, code load)
    torch.cuda.synchronize()
    ev[0].record()
    a = ctx.kmeans_assign_only(x, lists, metric)
    ev[1].record()
    torch.cuda.synchronize()
    assign_ms = ev[0].elapsed_time(ev[1])
    order = torch.argsort(a, stable=True)
    offsets = torch.zeros(nlist + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(a, minlength=nlist).cpu(), 0)
    ids = torch.arange(n, device="cuda", dtype=torch.int64)[order].contiguous()
    vecs = x[order].contiguous()
    del x
    s = Store(ctx, d)
    s.build_csr(offsets.numpy(), ids, vecs)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), lists.cpu())
    torch.cuda.synchronize()
    del vecs, ids
    return s, parent, lists, assign_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from quake_amd.capi import Context
    ctx = Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None
    for d, metric in ((4096, "l2"), (3072, "ip"), (2048, "l2")):
        s, parent, lists, assign_ms = corpus(ctx, args.n, d, args.nlist, metric, seed=d)
        g = torch.Generator(device="cuda").manual_seed(d + 1)
        rows = torch.randint(0, args.nlist, (args.q,), device="cuda", generator=g)
        q = (lists[rows] + 0.3 * torch.randn(args.q, d, device="cuda", generator=g)).contiguous()
        if metric == "ip":
            q /= q.norm(dim=1, keepdim=True)
        for k in (10, 100):
            for nprobe in (1, 8):
                ctx.search(parent, s, q, nprobe, k, metric)  # warm-up
                ts = [ctx.search(parent, s, q, nprobe, k, metric, timing=True)[2] for _ in range(args.reps)]
                med = {key: float(np.median([t[key] for t in ts])) for key in ("coarse_ms", "scan_ms", "total_ms")}
                scan_bytes = int(ts[-1]["scan_bytes"])
                rec = dict(n=args.n, d=d, metric=metric, nlist=args.nlist, Q=args.q, k=k, nprobe=nprobe,
                           scan_kernel=ctx.last_scan_kernel(), **{kk: round(v, 4) for kk, v in med.items()}, scan_bytes=scan_bytes,
                           scan_frac_hbm=round(scan_bytes / (med["scan_ms"] * 1e-3) / HBM_PEAK, 3) if med["scan_ms"] > 0 else None,
                           coarse_frac_mfma=round(2.0 * args.q * args.nlist * d / (med["coarse_ms"] * 1e-3) / MFMA_F32_PEAK, 3)
                           if med["coarse_ms"] > 0 else None,
                           assign_ms=round(assign_ms, 3),
                           assign_frac_mfma=round(2.0 * args.n * args.nlist * d / (assign_ms * 1e-3) / MFMA_F32_PEAK, 3))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
        s.close()
        parent.close()
        del lists, q
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
