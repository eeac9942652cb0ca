"""Paged-search probe: what a page behind a cursor costs at depth 0, 100 and 1000, next to the calls a caller has without it.
One JSON line per measurement to stdout and to --out:

    python scripts/paging_probe.py [--n 10000000] [--nlist 4096] [--q 1024] [--reps 7] [--out profiles/paging_probe.jsonl]

The bench shape (n x 128 L2, seeded, one GPU; scripts/filter_probe.py's corpus), k = 10, nprobe 1 and 8.  Per nprobe:
  page       qk_search_after at depth 0 (NULL cursors), 100 and 1000 -- the cursors come from pages of up to 448 chained in front --
             phases from HIP events (qk_timing), medians over --reps calls after two warm-ups, and the kernel's name
  filtered   qk_search_filtered under a filter that allows every id: the same scan form without the cursor
  search     qk_search with k = 10 and with k = 1000 (the key-emission path): what "ask again with a larger k" costs
  chain      100 chained pages of 10 against ONE qk_search with k = 1000: device time of each, summed over the calls
  next_cursor  once, at nprobe 128 / k = 448: the merge phase of a page (merge + k_next_cursor) next to the filtered search's
The `filtered` and `search` sections use nothing a tree without paged search lacks: run the script from the parent commit's tree
for the yardstick (the `page` and `chain` sections are skipped there)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filter_probe import corpus  # noqa: E402

PHASES = ("coarse_ms", "group_ms", "scan_ms", "merge_ms", "total_ms")


def timed(fn, reps):
    """medians of every phase over reps calls after two warm-ups; fn returns a timing dict"""
    for _ in range(2):
        fn()
    tms = [fn() for _ in range(reps)]
    return {p: float(np.median([t[p] for t in tms])) for p in PHASES}


def cursor_at(ctx, parent, s, q, nprobe, metric, depth):
    """the cursors behind the first `depth` results of every query (None at depth 0), from pages of up to 448"""
    after = None
    while depth > 0:
        step = min(depth, 448)
        after = ctx.search_after(parent, s, q, nprobe, step, metric, after=after)[2]
        depth -= step
    return after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from quake_amd import capi
    paged = hasattr(capi.Context, "search_after")
    ctx = capi.Context(0)
    ctx.set_timing(1)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(dict(tree="paged" if paged else "no paged search", n=args.n, nlist=args.nlist, q=args.q, **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    d, metric, k, Q = 128, "l2", 10, args.q
    s, parent, offsets, qall = corpus(ctx, args.n, d, args.nlist, metric, seed=1234)
    q = qall[:Q].contiguous()
    f_all = capi.Filter(s, np.zeros(0, np.int64), "deny")  # allows every id
    torch.cuda.synchronize()  # (the context runs on its own stream: torch's inputs are complete before it reads them)
    for nprobe in (1, 8):
        for kk in (10, 1000):
            tm = timed(lambda: ctx.search(parent, s, q, nprobe, kk, metric, timing=True)[2], args.reps)
            emit(dict(section="search", call="qk_search", nprobe=nprobe, k=kk, kernel=ctx.last_scan_kernel(), **tm))
        tm = timed(lambda: ctx.search(parent, s, q, nprobe, k, metric, timing=True, filter=f_all)[2], args.reps)
        emit(dict(section="filtered", call="qk_search_filtered", selectivity=1.0, nprobe=nprobe, k=k, kernel=ctx.last_scan_kernel(), **tm))
        if not paged:
            continue
        for depth in (0, 100, 1000):
            after = cursor_at(ctx, parent, s, q, nprobe, metric, depth)
            ctx.synchronize()
            tm = timed(lambda: ctx.search_after(parent, s, q, nprobe, k, metric, after=after, timing=True)[3], args.reps)
            full = float((ctx.search_after(parent, s, q, nprobe, k, metric, after=after)[0][:, -1] >= 0).float().mean().item())
            emit(dict(section="page", call="qk_search_after", nprobe=nprobe, k=k, depth=depth, full_rows=full, kernel=ctx.last_scan_kernel(), **tm))
        # 100 pages of 10 against one call with k = 1000: device time summed over the calls
        sums = []
        for _ in range(3):
            after, tot = None, {p: 0.0 for p in PHASES}
            for _page in range(100):
                r = ctx.search_after(parent, s, q, nprobe, k, metric, after=after, timing=True)
                after = r[2]
                for p in PHASES:
                    tot[p] += r[3][p]
            sums.append(tot)
        emit(dict(section="chain", call="100 x qk_search_after k=10", nprobe=nprobe, **{p: float(np.median([t[p] for t in sums])) for p in PHASES}))
        tm = timed(lambda: ctx.search(parent, s, q, nprobe, 1000, metric, timing=True)[2], 3)
        emit(dict(section="chain", call="1 x qk_search k=1000", nprobe=nprobe, **tm))
    # k_next_cursor at the shape where it walks most records (nprobe 128, k = 448): the page's merge phase -- merge + next cursor --
    # next to the filtered search's, which is the same merge alone
    if paged:
        tm = timed(lambda: ctx.search(parent, s, q, 128, 448, metric, timing=True, filter=f_all)[2], 3)
        emit(dict(section="next_cursor", call="qk_search_filtered", nprobe=128, k=448, **tm))
        tm = timed(lambda: ctx.search_after(parent, s, q, 128, 448, metric, timing=True)[3], 3)
        emit(dict(section="next_cursor", call="qk_search_after", nprobe=128, k=448, depth=0, **tm))
    f_all.close()
    s.close()
    parent.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
