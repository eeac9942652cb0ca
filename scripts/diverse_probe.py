"""Cost of diversified search on the facet workload.  One JSON line per measurement to stdout and --out:

    python scripts/diverse_probe.py [--n 10000000] [--d 128] [--nlist 4096] [--q 1024] [--nprobe 8] [--k 10] [--fetch 50,100,256]
        [--lam 0.5] [--reps 7] [--cases search,diverse,host] [--tag TAG] [--out profiles/diverse_probe.jsonl]

The workload of scripts/facet_probe.py: 10M x 128 L2, nlist 4096 (the seeded corpus of scripts/filter_probe.py),
1024 queries, nprobe 8.  All calls run on the same index in the same process.  Medians over --reps calls after two warm-up calls;
the phases of a call from HIP events (qk_timing) and the whole call on the host clock behind a synchronisation.
  search   qk_search with k = fetch_k: the candidate search alone
  diverse  qk_diverse_search at k and fetch_k; `tail_ms` = its total_ms minus the total_ms of `search` at the same fetch_k.  The
           tail is split by a second call with k = 1, whose selection kernel writes the first pick and runs no step:
           `lookup_ms` = total_ms(k = 1) - total_ms(search) -- the table, the sweep over the stored ids and the per-candidate
           lookups -- and `select_ms` = total_ms(k) - total_ms(k = 1) -- staging and the k - 1 selection steps
  host     the route without the call: search(k = fetch_k) with device buffers, ids and distances to the host, Store.get_vectors
           (qk_store_get_vectors: host ids, host buffers), then per query the vectorised numpy form of the definition (one matrix
           product for the pairwise values -- not the canonical arithmetic, so its picks may differ in ties) -- wall clock only
Run once per library for the two forms of k_diverse_select (QUAKE_HIP_LIB: the product library stages a query's rows in LDS once;
the side build with -DQK_DIVERSE_STAGE_ALL=0 re-reads the candidate rows from the arena at every step).
The probe asserts nothing about time; it checks the first query of every diversified call against the yardstick's definition on
the vectors the store returns."""
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
    return rec


def host_mmr(r, V, k, lam):
    """the definition for L2 in vectorised numpy float32 over one query's candidates (distances r [n], vectors V [n, d]) -> ranks"""
    n = r.shape[0]
    sq = (V * V).sum(axis=1)
    P = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (V @ V.T), 0.0)).astype(np.float32)
    lam32, mu32 = np.float32(lam), np.float32(1.0) - np.float32(lam)
    picked = np.zeros(n, bool)
    N = np.full(n, np.inf, np.float32)
    pick, out = 0, []
    for _ in range(min(k, n)):
        out.append(pick)
        picked[pick] = True
        N = np.minimum(N, P[:, pick])
        cost = np.where(picked, np.float32(np.inf), lam32 * r - mu32 * N)
        pick = int(np.argmin(cost))
    return np.array(out, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch", default="50,100,256")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="search,diverse,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="stage_all_rows")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
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
    Q, nprobe, k, lam = args.q, args.nprobe, args.k, args.lam
    for C_ in [int(c) for c in args.fetch.split(",")]:
        srec = None
        if "search" in cases or "diverse" in cases:
            srec = timed(ctx, lambda: ctx.search(parent, s, q, nprobe, C_, "l2", timing=True)[2], args.reps)
            emit(dict(case="search", fetch_k=C_, kernel=ctx.last_scan_kernel(), **srec))
        if "diverse" in cases:
            one = timed(ctx, lambda: ctx.diverse_search(parent, s, q, nprobe, 1, C_, lam, "l2", timing=True)[3], args.reps)
            rec = timed(ctx, lambda: ctx.diverse_search(parent, s, q, nprobe, k, C_, lam, "l2", timing=True)[3], args.reps)
            emit(dict(case="diverse", k=k, fetch_k=C_, lam=lam, kernel=ctx.last_scan_kernel(), **rec, total_ms_k1=one["total_ms"],
                      tail_ms=rec["total_ms"] - srec["total_ms"], lookup_ms=one["total_ms"] - srec["total_ms"],
                      select_ms=rec["total_ms"] - one["total_ms"]))
            # the first query against the definition, on the vectors the store returns
            import diverse_yardstick as DY
            got = ctx.diverse_search(parent, s, q[:1].contiguous(), nprobe, k, C_, lam, "l2")
            cand = ctx.search(parent, s, q[:1].contiguous(), nprobe, C_, "l2")
            ctx.synchronize()   # (the context's stream is its own)
            gi, gd, gr = (t.cpu().numpy() for t in got)
            ci, cd = (t.cpu().numpy() for t in cand)
            V, found = s.get_vectors(ci[0])
            assert found.all()
            wi, wd, wr = DY.expected(ci[0], cd[0], DY.pairwise(V, "l2"), k, lam, "l2")
            assert (gi[0] == wi).all() and (gr[0] == wr).all() and gd[0].tobytes() == wd.tobytes(), (gr[0], wr)
        if "host" in cases:
            def host_route():
                ids, dist = ctx.search(parent, s, q, nprobe, C_, "l2")
                ctx.synchronize()
                hi, hd = ids.cpu().numpy(), dist.cpu().numpy()
                V, _ = s.get_vectors(hi.reshape(-1))
                V = V.reshape(Q, C_, args.d)
                res = np.empty((Q, k), np.int64)
                for qi in range(Q):
                    res[qi] = hi[qi][host_mmr(hd[qi], V[qi], k, lam)]
                return res
            host_route()
            wall = []
            for _ in range(3):
                ctx.synchronize()
                t0 = time.perf_counter()
                host_route()
                wall.append((time.perf_counter() - t0) * 1e3)
            # where the host route's time goes: the search and copies, the get, the loop
            t0 = time.perf_counter()
            ids, dist = ctx.search(parent, s, q, nprobe, C_, "l2")
            ctx.synchronize()
            hi, hd = ids.cpu().numpy(), dist.cpu().numpy()
            t1 = time.perf_counter()
            V, _ = s.get_vectors(hi.reshape(-1))
            t2 = time.perf_counter()
            V = V.reshape(Q, C_, args.d)
            for qi in range(Q):
                host_mmr(hd[qi], V[qi], k, lam)
            t3 = time.perf_counter()
            emit(dict(case="host_route", k=k, fetch_k=C_, lam=lam, wall_ms=float(np.median(wall)), search_and_copy_ms=(t1 - t0) * 1e3,
                      get_vectors_ms=(t2 - t1) * 1e3, numpy_loop_ms=(t3 - t2) * 1e3))
    if out:
        out.close()


if __name__ == "__main__":
    main()
