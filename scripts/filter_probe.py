"""Filtered-search probe: what a filter costs and what it saves on the bench corpora.  One JSON line per measurement to stdout and
to --out:

    python scripts/filter_probe.py [--config bench128|ip768|all] [--n 10000000] [--nlist 4096] [--q 1024] [--reps 7]
                                   [--out profiles/filter_probe.jsonl] [--unfiltered-only]

Configs: bench128 = n x 128 L2, k 10, nprobe 1 and 8 (the bench.py corpus shape); ip768 = n x 768 IP, k 100, nprobe 1.  For every
selectivity in 1, 0.5, 0.1, 0.01, 0.001 the allowed ids are drawn (a) "uniform": uniformly over all ids, (b) "ranges": as whole
contiguous id ranges of the build order -- ids are handed out list by list, so a range is a run of rows of a few lists (the tenant
case: most tiles of a probed list empty out).  Per case: the scan kernel's device time (qk_timing.scan_ms: HIP events around the
kernel) and the whole call's, medians over --reps calls after two warm-up calls; the unfiltered search of the same call on the
same tree (--unfiltered-only prints only those lines and uses nothing a tree without filters lacks: run it on the parent commit
for the yardstick); the algorithmic bytes of the probed lists (scan_bytes) and the share of their 16-row tiles that holds a
candidate; filter creation (host wall clock: sort + upload + first mask build) and the device time of a search that has to
rebuild the mask first (after a table change) next to a steady one (total_ms of the call: HIP events).
Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/filter_probe.py ...` for the per-kernel summary."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SELECTIVITIES = [1.0, 0.5, 0.1, 0.01, 0.001]


def corpus(ctx, n, d, nlist, metric, seed):
    """seeded clustered rows generated on the device, lists from one nearest-centroid assign against nlist sampled rows; ids
    0..n-1 in build order (list by list)"""
    from quake_amd.capi import Store
    g = torch.Generator(device="cuda").manual_seed(seed)
    nc = 4 * nlist
    cent = torch.randn(nc, d, device="cuda", generator=g)
    x = cent[torch.randint(0, nc, (n,), device="cuda", generator=g)]
    x.add_(0.5 * torch.randn(n, d, device="cuda", generator=g))
    if metric == "ip":
        x /= x.norm(dim=1, keepdim=True)
    lists = x[torch.randperm(n, device="cuda", generator=g)[:nlist]].contiguous()
    # the context runs on its own stream: everything torch has enqueued so far -- the rows it is about to read, and the randperm
    # whose freed block `a` may be given -- must be done before the library call (it returns synchronised)
    torch.cuda.synchronize()
    a = ctx.kmeans_assign_only(x, lists, metric)
    order = torch.argsort(a, stable=True)
    sizes = torch.bincount(a, minlength=nlist).cpu().numpy().astype(np.int64)
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    q = (x[torch.randint(0, n, (4096,), device="cuda", generator=g)] + 0.05 * torch.randn(4096, d, device="cuda", generator=g))
    if metric == "ip":
        q /= q.norm(dim=1, keepdim=True)
    vecs = x[order].contiguous()
    del x
    ids = torch.arange(n, device="cuda", dtype=torch.int64)
    torch.cuda.synchronize()  # (as above: build_csr reads vecs and ids on the context's stream)
    s = Store(ctx, d)
    s.build_csr(offsets, ids, vecs)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), lists.cpu())
    torch.cuda.synchronize()
    del vecs
    return s, parent, offsets, q.contiguous()


def draw(n, sel, how, rng):
    m = n if sel >= 1 else max(1, int(round(sel * n)))
    if how == "uniform" or sel >= 1:
        return np.sort(rng.permutation(n)[:m]).astype(np.int64)
    # whole ranges of the build order: 64 ranges that add up to m ids
    nr = 64
    ln = max(1, m // nr)
    starts = np.sort(rng.choice(max(1, n - ln), size=nr, replace=False))
    return np.unique(np.concatenate([np.arange(s0, min(n, s0 + ln)) for s0 in starts])).astype(np.int64)


def tile_share(offsets, S, n):
    """share of the 16-row tiles of all lists that hold an allowed row"""
    allowed = np.zeros(n, bool)
    allowed[S] = True
    sizes = np.diff(offsets)
    lst = np.repeat(np.arange(sizes.shape[0]), sizes)
    tile = (np.arange(n) - offsets[lst]) // 16
    ntl = (sizes + 15) // 16
    base = np.zeros(sizes.shape[0] + 1, np.int64)
    base[1:] = np.cumsum(ntl)
    hit = np.zeros(int(base[-1]), bool)
    hit[(base[lst] + tile)[allowed]] = True
    return float(hit.mean())


def timed(ctx, fn, reps):
    for _ in range(2):
        fn()
    scan, total = [], []
    for _ in range(reps):
        tm = fn()
        scan.append(tm["scan_ms"])
        total.append(tm["total_ms"])
    return float(np.median(scan)), float(np.median(total)), tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--unfiltered-only", action="store_true")
    args = ap.parse_args()
    from quake_amd import capi
    Filter = getattr(capi, "Filter", None)
    if Filter is None and not args.unfiltered_only:
        sys.exit("this tree has no filtered search: run with --unfiltered-only")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    configs = {"bench128": (128, "l2", 10, [1, 8]), "ip768": (768, "ip", 100, [1])}
    for name, (d, metric, k, nprobes) in configs.items():
        if args.config not in ("all", name):
            continue
        s, parent, offsets, qall = corpus(ctx, args.n, d, args.nlist, metric, seed=1234)
        q = qall[: args.q].contiguous()
        oi = torch.empty((args.q, k), dtype=torch.int64, device="cuda")
        od = torch.empty((args.q, k), dtype=torch.float32, device="cuda")
        rng = np.random.default_rng(99)
        for nprobe in nprobes:
            sc, tot, tm = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=(oi, od))[2], args.reps)
            emit(dict(config=name, n=args.n, d=d, metric=metric, k=k, nprobe=nprobe, q=args.q, case="unfiltered", scan_ms=sc, total_ms=tot,
                      kernel=ctx.last_scan_kernel(), scan_bytes=int(tm["scan_bytes"])))
        if args.unfiltered_only:
            s.close()
            parent.close()
            continue
        for how in ("uniform", "ranges"):
            for sel in SELECTIVITIES:
                if how == "ranges" and sel >= 1:
                    continue
                S = draw(args.n, sel, how, rng)
                t0 = time.perf_counter()
                f = Filter(s, S, "allow")
                ctx.synchronize()
                create_ms = (time.perf_counter() - t0) * 1e3
                info = f.info()
                share = tile_share(offsets, S, args.n)
                for nprobe in nprobes:
                    fn = lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, out=(oi, od), filter=f)[2]
                    sc, tot, tm = timed(ctx, fn, args.reps)
                    emit(dict(config=name, n=args.n, d=d, metric=metric, k=k, nprobe=nprobe, q=args.q, case=how, selectivity=sel,
                              n_ids=info["n_ids"], rows_allowed=info["rows_allowed"], tiles_with_candidate=share, scan_ms=sc, total_ms=tot,
                              kernel=ctx.last_scan_kernel(), scan_bytes=int(tm["scan_bytes"]),
                              padded=float((oi < 0).float().mean().item())))
                # a table change (an empty list comes and goes), then one search: its total_ms (HIP events from the coarse step to the
                # merge) contains the mask rebuild, which is enqueued between the two
                rebuild = []
                for _ in range(3):
                    s.add_list(args.nlist + 7)
                    s.remove_list(args.nlist + 7)
                    s.publish()
                    rebuild.append(ctx.search(parent, s, q, nprobes[0], k, metric, timing=True, out=(oi, od), filter=f)[2]["total_ms"])
                steady = ctx.search(parent, s, q, nprobes[0], k, metric, timing=True, out=(oi, od), filter=f)[2]["total_ms"]
                emit(dict(config=name, n=args.n, case=how, selectivity=sel, n_ids=info["n_ids"], filter_create_ms=create_ms,
                          search_with_rebuild_ms=float(np.median(rebuild)), search_steady_ms=steady, rebuilds=f.info()["rebuilds"],
                          filter_device_bytes=info["device_bytes"]))
                f.close()
        s.close()
        parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
