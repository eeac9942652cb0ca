"""Exact per-query filtered search probe: a batch of 1024 queries that mixes T tenants, answered (a) by the one call over the
candidate pool, (c) by the only exact route a tree without it has -- the batch split on the host and the single-filter exact call
looped over the distinct tenants -- and (d) by the probed per-query call at nprobe 8.  One JSON line per measurement to stdout and
to --out:

    python scripts/exact_filter_batch_probe.py [--tree DIR] [--loop-only] [--process NAME] [--q 1024] [--reps 7]
                                               [--out profiles/exact_filter_batch_probe.jsonl]

Corpus: filter_probe.py's 10M x 128 L2 shape (4096 lists), k = 10.  Tenants are `where` filters tenant == t over a column that
scatters the ids uniformly over n // rows tenants: about 10 000 candidates each with T = 4, 64, 1024 tenants per batch, about
100 000 each with T = 4, 64; queries are assigned to the batch's tenants uniformly.  Per shape: total_ms of qk_timing (HIP events:
mask builds, admission, scan, merge) as the median of --reps calls after two warm-ups, and for the loop the sum of its calls'
total_ms next to the wall time of the whole loop with its split and scatter (the one call's wall time is given too);
(b) the one call right after a store change (every mask rebuilt, every slot gathered again) and with half of the batch's tenants
new to the pool; recall@10 of (d) against (a); the pool's device bytes.  --tree DIR imports quake_amd from another tree (the
parent commit's, with its own library), --loop-only measures (c) alone and uses nothing such a tree lacks.  --process names the
process in every line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(10_000, 4), (10_000, 64), (10_000, 1024), (100_000, 4), (100_000, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--process", default="tree")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "scripts"))
    from quake_amd import capi
    from adaptive_filter_probe import recall_rows
    from filter_probe import corpus
    if not args.loop_only and not hasattr(capi.Context, "search_exact_batch"):
        sys.exit("this tree has no exact per-query filtered search: run with --loop-only")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(process=args.process, pid=os.getpid(), **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n, d, metric, k, Q = args.n, 128, "l2", 10, args.q
    s, parent, offsets, qall = corpus(ctx, n, d, args.nlist, metric, seed=1234)
    q = qall[:Q].contiguous()
    oi = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(77)
    scatter = torch.randperm(n, generator=g, device="cuda")
    all_ids = torch.arange(n, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(99)

    def touch():
        """a table change that moves no row: an empty list comes and goes"""
        s.add_list(args.nlist + 7)
        s.remove_list(args.nlist + 7)
        s.publish()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def med(fn, reps):
        for _ in range(2):
            fn()
        return [float(np.median(v)) for v in zip(*[fn() for _ in range(reps)])]

    columns = {}
    for rows, T in SHAPES:
        ntenants = n // rows
        if T > ntenants:  # (1024 tenants of 10 000 rows need 10.24M rows: the tenants shrink to n // 1024)
            ntenants = T
        if (rows, ntenants) not in columns:
            attr = capi.Attr(s)
            attr.set(all_ids, scatter % ntenants)
            columns[(rows, ntenants)] = attr
        attr = columns[(rows, ntenants)]
        order = rng.permutation(ntenants)
        tenants, spare = order[:T], order[T:]
        make = lambda ts: [capi.Filter.where(s, [(attr, "range", int(t), int(t))]) for t in ts]
        flts = make(tenants)
        qf_host = rng.integers(0, T, size=Q).astype(np.int32)
        qf = torch.from_numpy(qf_host).cuda()
        base = dict(n=n, nlist=args.nlist, d=d, q=Q, k=k, tenants=T, rows_per_tenant=int(flts[0].info()["rows_allowed"]))
        groups = [(int(t), torch.from_numpy(np.nonzero(qf_host == t)[0]).cuda()) for t in np.unique(qf_host)]

        def loop():
            """today's exact route: split, one single-filter call per distinct tenant, scatter"""
            tot = 0.0
            for t, idx in groups:
                gi, gd, tm = ctx.search_exact(s, q[idx], k, metric, flts[t], timing=True)
                oi[idx], od[idx] = gi, gd
                tot += tm["total_ms"]
            return tot

        def loop_timed():
            tot, w = wall(loop)
            return tot, w

        lt, lw = med(loop_timed, args.reps)  # (every tenant's private store is resident behind the warm-ups)
        loop_ids = oi.clone()
        emit(dict(call="(c) loop of search_exact over the distinct tenants, steady", total_ms=lt, wall_ms=lw, calls=len(groups), **base))
        if not args.loop_only:
            one = lambda: wall(lambda: ctx.search_exact_batch(s, q, k, metric, flts, qf, timing=True, out=(oi, od))[2]["total_ms"])
            st, sw = med(one, args.reps)
            ctx.synchronize()
            assert torch.equal(oi, loop_ids), "the one call and the loop differ"
            exact = oi.clone()
            info = s.exact_pool_info()
            emit(dict(call="(a) one call, all slots resident", total_ms=st, wall_ms=sw, kernel=ctx.last_scan_kernel(),
                      pool_device_bytes=info["device_bytes"], pool_rows=info["rows"], **base))
            after = []
            for _ in range(3):
                touch()
                after.append(one())
            emit(dict(call="(b) one call right after a store change", total_ms=float(np.median([a[0] for a in after])),
                      wall_ms=float(np.median([a[1] for a in after])), builds=s.exact_pool_info()["builds"], **base))
            half = []
            for r in range(3):
                fresh = spare[r * (T // 2):(r + 1) * (T // 2)]
                if len(fresh) < T // 2 or T < 2:
                    break
                mixed = flts[:T - T // 2] + make(fresh)
                half.append(wall(lambda: ctx.search_exact_batch(s, q, k, metric, mixed, qf, timing=True, out=(oi, od))[2]["total_ms"]))
                for f in mixed[T - T // 2:]:
                    f.close()
            if half:
                emit(dict(call="(b) one call, half of the tenants new", total_ms=float(np.median([a[0] for a in half])),
                          wall_ms=float(np.median([a[1] for a in half])), reps=len(half), **base))
            pt, pw = med(lambda: wall(lambda: ctx.search(parent, s, q, 8, k, metric, timing=True, out=(oi, od), filters=flts,
                                                          query_filter=qf)[2]["total_ms"]), args.reps)
            ctx.synchronize()
            short, rec = recall_rows(oi, exact)
            emit(dict(call="(d) probed per-query call, nprobe 8", total_ms=pt, wall_ms=pw, recall_at_k=rec, short_rows=short, **base))
        for f in flts:
            f.close()
        if not args.loop_only:
            s.exact_pool_drop()
    if out:
        out.close()


if __name__ == "__main__":
    main()
