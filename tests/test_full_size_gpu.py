"""Size-independent properties at BASELINE.json's full single-GPU sizes (configs[1]: 10M x 128 L2 nlist 4096 batch 1024 k 10;
configs[2]: 10M x 768 IP k 100), where the CPU oracle would take minutes.  Everything goes through the C ABI (qk_search /
qk_coarse); torch is only the independent arithmetic the answers are checked with.

  sortedness        rows ascending in distance (descending inner product), ids ascending inside a tie, no id twice
  consistency       every returned distance is the distance of the returned id (recomputed in float64)
  exactness         nprobe = 1: the answer is the exact top-k of the probed list (float64 brute force over that list)
  idempotence       the same call twice gives the same bits
  monotonicity      nprobe = 4 is rank by rank at least as good as nprobe = 1, and holds every nprobe = 1 entry that beats
                    its k-th (candidate sets are nested)
  completeness      scanning every list = exact flat search (float64 re-rank of a brute-force shortlist, slice of the batch)

Tolerances (float64 is the judge here, not the fp32 oracle the small-size parity tests are bit-exact against): distances
within 1e-4 (L2, the bar BASELINE.json's north_star states) / 1e-5 (inner product of unit vectors); ids exact wherever the
float64 gap to both neighbours exceeds twice that -- below it fp32 cannot separate the candidates and the canonical tie rule
decides.

configs[3] (100M x 128 L2, nlist 65536, batch 4096, k 10, 8 members) runs here whole, on one GPU: the device group
(qk_group_*, QuakeIndex with num_workers = 8) against ONE store of the same 100M rows, bit for bit on every row, at the shapes
where the group's pieces change (coarse split by queries, per-member scan forms, packed 12-byte top-k records with 64-bit ids,
the lead's merge of 8 blocks), then against the oracle and float64 on a sample of the batch, then after a 1M-id removal."""
import numpy as np
import pytest
import torch

import bench as B

pytestmark = pytest.mark.gpu
ID0 = 7  # ids are not row numbers


def _build(ctx, n, d, nlist, metric, niter=2):
    from quake_amd.capi import Store
    dev = torch.device("cuda", 0)
    unit = metric == "ip"
    x, cent_true = B.gen_mixture(n, d, nlist, seed=11, device=dev, unit=unit)
    centroids, assign, _ = ctx.kmeans(x, nlist, metric, niter=niter, seed=1234)
    order = torch.argsort(assign, stable=True)
    counts = torch.bincount(assign, minlength=nlist).cpu().numpy().astype(np.int64)
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(counts)
    ids_sorted = (order + ID0).contiguous()
    x_sorted = x[order].contiguous()
    del x, order, assign
    store = Store(ctx, d)
    store.build_csr(offsets, ids_sorted, x_sorted)
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), torch.arange(nlist, device=dev), centroids.contiguous())
    q = B.gen_queries(1024, cent_true, seed=12, device=dev, unit=unit)
    return parent, store, x_sorted, ids_sorted, offsets, q


def _dist64(q, rows, metric):
    """float64 distance (as reported: L2 distance / inner product) of every query to its own rows: [Q, d], [Q, m, d] -> [Q, m]"""
    if metric == "l2":
        return ((rows.double() - q.double()[:, None, :]) ** 2).sum(2).sqrt()
    return (rows.double() * q.double()[:, None, :]).sum(2)


def _key(dist, metric):
    return dist if metric == "l2" else -dist


def _check_rows_sorted(ids, dist, metric):
    key = _key(dist, metric)
    assert bool((key[:, 1:] >= key[:, :-1]).all())
    tie = key[:, 1:] == key[:, :-1]
    assert bool((ids[:, 1:][tie] > ids[:, :-1][tie]).all())
    srt = torch.sort(ids, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())


def _check_exact(q, gi, gd, cand_rows, cand_ids, valid, k, metric, tol):
    """(gi, gd) [n, k] = the k best of per-query candidate sets (cand_rows [n, m, d], cand_ids [n, m], valid [n, m]; every
    query has more than k valid candidates), judged in float64."""
    d64 = _dist64(q, cand_rows, metric)
    key = torch.where(valid, _key(d64, metric), torch.full_like(d64, float("inf")))
    skey, sidx = torch.sort(key, dim=1)
    ref_ids = torch.gather(cand_ids, 1, sidx)[:, :k]
    ref_key = skey[:, :k]
    assert torch.allclose(_key(gd, metric).double(), ref_key, atol=tol, rtol=0)
    gap_next = skey[:, 1:k + 1] - skey[:, :k]
    gap_prev = torch.cat([torch.full_like(skey[:, :1], 1.0), skey[:, 1:k] - skey[:, :k - 1]], 1)
    clear = (gap_next > 2 * tol) & (gap_prev > 2 * tol)
    assert clear.float().mean().item() > 0.3, clear.float().mean().item()
    assert bool((gi[clear] == ref_ids[clear]).all())


def _run_properties(ctx, n, d, nlist, k, metric, list_queries, flat_queries):
    tol = 1e-4 if metric == "l2" else 1e-5
    parent, store, xs, ids_sorted, offsets, q = _build(ctx, n, d, nlist, metric)
    dev = q.device
    off_t = torch.from_numpy(offsets).to(dev)
    row_of = torch.empty(n, dtype=torch.int64, device=dev)  # id -> row of the (list-sorted) corpus
    row_of[ids_sorted - ID0] = torch.arange(n, device=dev)
    # ---- nprobe = 1 -------------------------------------------------------------------------------------------------
    i1, d1 = ctx.search(parent, store, q, 1, k, metric)
    i1b, d1b = ctx.search(parent, store, q, 1, k, metric)
    assert torch.equal(i1, i1b) and torch.equal(d1.view(torch.int32), d1b.view(torch.int32))  # idempotence
    pids = ctx.coarse(parent, q, 1, metric)[0].reshape(-1)
    sizes_all = off_t[pids + 1] - off_t[pids]
    full = sizes_all > k  # (a probed list with fewer than k rows pads its answer with -1: left to the small-size tests)
    assert full.float().mean().item() > 0.9
    q1, i1f, d1f = q[full], i1[full], d1[full]
    assert bool(((i1f >= ID0) & (i1f < n + ID0)).all())
    _check_rows_sorted(i1f, d1f, metric)
    for s0 in range(0, q1.shape[0], 256):  # consistency: the distance belongs to the id
        sl = slice(s0, s0 + 256)
        got = _dist64(q1[sl], xs[row_of[i1f[sl] - ID0]], metric)
        assert torch.allclose(d1f[sl].double(), got, atol=tol, rtol=0)
    # exactness on the probed list (a slice of the batch: the candidate gather is [slice, longest list, d])
    sl = slice(0, list_queries)
    pf = pids[full][sl]
    lo, hi = off_t[pf], off_t[pf + 1]
    sizes = hi - lo
    ar = torch.arange(int(sizes.max().item()), device=dev)[None, :]
    rows = torch.minimum(lo[:, None] + ar, (hi - 1)[:, None])  # padded with the list's last row
    _check_exact(q1[sl], i1f[sl], d1f[sl], xs[rows], ids_sorted[rows], ar < sizes[:, None], k, metric, tol)
    del rows
    # ---- nprobe = 4: nested candidate sets ------------------------------------------------------------------------------
    i4, d4 = ctx.search(parent, store, q, 4, k, metric)
    _check_rows_sorted(i4[full], d4[full], metric)
    key1, key4 = _key(d1f, metric), _key(d4[full], metric)
    assert bool((key4 <= key1).all())
    better = key1 < key4[:, k - 1:k]
    present = (i1f[:, :, None] == i4[full][:, None, :]).any(2)
    assert bool(present[better].all())
    # ---- every list: exact flat search ----------------------------------------------------------------------------------
    qf = q[:flat_queries].contiguous()
    ia, da = ctx.search(parent, store, qf, nlist, k, metric)
    _check_rows_sorted(ia, da, metric)
    bi, _ = B.brute_force_topk(qf, xs, 2 * k, metric=metric)  # fp32 shortlist (row numbers), re-ranked in float64
    cand = torch.sort(torch.cat([bi, row_of[ia - ID0]], 1), dim=1).values
    dup = torch.cat([torch.zeros_like(cand[:, :1], dtype=torch.bool), cand[:, 1:] == cand[:, :-1]], 1)
    _check_exact(qf, ia, da, xs[cand], ids_sorted[cand], ~dup, k, metric, tol)
    store.close()
    parent.close()


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def test_configs1_10m_x_128_l2_k10(ctx):
    _run_properties(ctx, 10_000_000, 128, 4096, 10, "l2", list_queries=256, flat_queries=64)
    torch.cuda.empty_cache()


def test_configs2_10m_x_768_ip_k100(ctx):
    _run_properties(ctx, 10_000_000, 768, 4096, 100, "ip", list_queries=32, flat_queries=16)
    torch.cuda.empty_cache()


# ---- configs[3] at full size: an 8-member device group against one store ------------------------------------------------------
N3, D3, NLIST3, G3 = 100_000_000, 128, 65536, 8
# ids >= 2^33 (a record field cut to 32 bits changes every one of them), not monotone inside a list, and spread over more than
# 2^30: remove_ids takes its hash set then (its id bitmap covers [smallest id, largest id] when that range is below 2^30)
ID_BASE3, ID_STEP3 = 1 << 33, 16
KILL3 = 1_000_000  # ids removed
NEED_FREE3 = 120e9  # corpus (51 GB) + one index (51 GB) + the sample's rows + the scratch of the searches
CPU_THREADS3 = 16  # oracle threads
CASES3 = [  # (Q, k, nprobe, device buffers)
    (4096, 10, 8, False),  # configs[3] itself
    (4096, 10, 1, False),
    (4096, 10, 32, False),
    (4096, 100, 8, False),  # wider pools and merge
    (4097, 10, 8, False),  # the coarse split by queries is not a multiple of 8 (7 x 513 + 506)
    (512, 10, 8, False),  # the smallest split batch: 64 queries per member
    (511, 10, 8, False),  # one below it: every member ranks the centroids for the whole batch itself
    (1, 10, 8, False),
    (4096, 10, 8, True),  # device-resident queries and answers
]


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    if not bad.size:
        return "equal"
    at = tuple(bad[0])
    return f"{len(bad)} entries differ, first at {at}: {got[at]} vs {want[at]}"


def _member_forms(grp):
    """qk_ctx_last_scan_kernel of every member's context"""
    import ctypes
    from quake_amd._lib import check
    forms = []
    for j in range(grp.size()):
        c, _ = grp.member_handles(j)
        buf = ctypes.create_string_buffer(64)
        check(grp.lib.qk_ctx_last_scan_kernel(c, buf, 64))
        forms.append(buf.value.decode())
    return forms


def _run_index(ix, search, forms, q, request, probe_ids):
    """The same calls on either index; only host copies of the answers are kept.  search(x, nprobe, k) -> (ids, dist, timing)."""
    qh = q.cpu().numpy()
    out = {}
    for case in CASES3:
        Q, k, nprobe, on_device = case
        gi, gd, tm = search(q[:Q] if on_device else qh[:Q], nprobe, k)
        assert hasattr(gi, "is_cuda") == on_device
        out[case] = dict(ids=_host(gi), dist=_host(gd), forms=forms(), pairs=tm["partitions_scanned"], bytes=tm["scan_bytes"])
    out["removed"] = ix.remove_ids(request)
    out["ntotal"] = ix.ntotal()
    gi, gd, _ = search(qh[:4096], 8, 10)
    out["after"] = dict(ids=gi, dist=gd, forms=forms())
    out["get"] = [ix.get_vector(int(v)) for v in probe_ids]
    return out


@pytest.fixture(scope="module")
def configs3():
    """Everything the configs[3] tests assert on, made once.  The corpus (51 GB, generated in list order on the device) is the
    input of (a) one Store of all 100M rows, which runs the script and is closed, then of (b) Group([0] * 8) -- the two indexes
    are never held together."""
    import oracle as O
    from quake_amd.capi import Context, Group, Store
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE3:
        pytest.fail(f"configs[3] at full size needs ~{NEED_FREE3 / 1e9:.0f} GB of free device memory; {free / 1e9:.1f} GB are free")
    dev = torch.device("cuda", 0)
    nthr = min(CPU_THREADS3, O.max_threads())
    g = torch.Generator(device=dev).manual_seed(31)
    cent = torch.randn(NLIST3, D3, generator=g, device=dev)
    # the generating centre of a row is its list (no k-means), drawn uniformly: ~1526 rows per list.  Rows are made list by list,
    # already in CSR order (no second 51 GB tensor for a sorted copy).
    counts = torch.bincount(torch.randint(0, NLIST3, (N3,), generator=g, device=dev), minlength=NLIST3)
    offsets = np.zeros(NLIST3 + 1, np.int64)
    offsets[1:] = np.cumsum(counts.cpu().numpy())
    list_of_row = torch.repeat_interleave(torch.arange(NLIST3, device=dev), counts, output_size=N3)
    x = torch.empty(N3, D3, device=dev)
    for i0 in range(0, N3, 1 << 22):
        m = min(1 << 22, N3 - i0)
        x[i0:i0 + m] = cent[list_of_row[i0:i0 + m]] + 0.3 * torch.randn(m, D3, generator=g, device=dev)
    del list_of_row, counts
    ids = ID_BASE3 + ID_STEP3 * torch.randperm(N3, generator=g, device=dev)
    q = B.gen_queries(4097, cent, seed=32, device=dev)
    qh = q.cpu().numpy()

    # ---- the oracle on a 256-query sample of the 4096 batch: coarse over the 65536 centroids, then the union of the probed lists
    #      (<= 2048 lists, ~1.6 GB) as a small CSR of its own -- the corpus never goes to the host
    rng = np.random.default_rng(33)
    sample = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 4095), 254, replace=False)), [4095]])
    qs = np.ascontiguousarray(qh[sample])
    cent_h = cent.cpu().numpy()
    coarse_o = {p: O.coarse(qs, cent_h, None, p, "l2", num_threads=nthr) for p in (1, 8)}
    u = np.unique(coarse_o[8][0])
    sizes = offsets[u + 1] - offsets[u]
    uoff = np.zeros(len(u) + 1, np.int64)
    uoff[1:] = np.cumsum(sizes)
    rows = (torch.repeat_interleave(torch.from_numpy(offsets[u] - uoff[:-1]).to(dev), torch.from_numpy(sizes).to(dev))
            + torch.arange(int(uoff[-1]), device=dev))
    ux, uid = x[rows], ids[rows]
    del rows
    lists_u = {p: np.searchsorted(u, coarse_o[p][0]) for p in (1, 8)}  # list numbers of the small CSR
    ux_h, uid_h = ux.cpu().numpy(), uid.cpu().numpy()
    oracle_ans = {p: O.batched_serial_scan(qs, ux_h, uid_h, uoff, lists_u[p], 10, "l2", num_threads=nthr) for p in (1, 8)}
    del ux_h, uid_h

    # ---- the mutation: 1M ids spread over every list + 1000 ids the index does not hold + 1000 repeats
    kill_rows = rng.choice(N3, KILL3, replace=False)
    kill = ids[torch.from_numpy(kill_rows).to(dev)].cpu().numpy()
    absent = ID_BASE3 + ID_STEP3 * rng.integers(0, N3, 1000) + rng.integers(1, ID_STEP3, 1000)  # between two ids of the index
    request = rng.permutation(np.concatenate([kill, absent, kill[rng.choice(kill.shape[0], 1000, replace=False)]]))
    alive = np.setdiff1d(rng.choice(N3, 64, replace=False), kill_rows)[:16]
    assert alive.shape[0] == 16
    probe = torch.from_numpy(np.concatenate([alive, kill_rows[:16]])).to(dev)  # 16 survivors, then 16 removed
    probe_ids, probe_vecs = ids[probe].cpu().numpy(), x[probe].cpu().numpy()

    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_form_feedback(False)  # the static rule alone decides which form serves a call
    parent = Store(ctx, D3)
    parent.build_csr(np.array([0, NLIST3], np.int64), torch.arange(NLIST3, device=dev), cent)
    coarse_g = {p: ctx.coarse(parent, qs, p, "l2") for p in (1, 8)}
    torch.cuda.synchronize()
    # ---- (a) one store
    store = Store(ctx, D3)
    store.build_csr(offsets, ids, x)
    assert store.ntotal() == N3 and store.nlist() == NLIST3
    single = _run_index(store, lambda xq, nprobe, k: ctx.search(parent, store, xq, nprobe, k, "l2", timing=True),
                        ctx.last_scan_kernel, q, request, probe_ids)
    store.close()
    torch.cuda.empty_cache()
    # ---- (b) the device group of 8 members on device 0, built from the same device arrays
    grp = Group([0] * G3, D3)
    grp.set_stream(torch.cuda.current_stream().cuda_stream)
    grp.set_form_feedback(False)
    grp.build_csr(offsets, ids, x)
    held = [grp.member_list_ids(j) for j in range(G3)]
    layout = dict(size=grp.size(), ntotal=grp.ntotal(), nlist=grp.nlist(),
                  held=[(len(h), bool((h % G3 == j).all())) for j, h in enumerate(held)])
    group = _run_index(grp, lambda xq, nprobe, k: grp.search(parent, xq, nprobe, k, "l2", timing=True),
                       lambda: _member_forms(grp), q, request, probe_ids)
    grp.close()
    del x, ids
    torch.cuda.empty_cache()
    yield dict(single=single, group=group, layout=layout, sample=sample, qs=qs, coarse_o=coarse_o, coarse_g=coarse_g,
               uoff=uoff, ux=ux, uid=uid, lists_u=lists_u, oracle=oracle_ans, kill=kill, probe_vecs=probe_vecs)
    parent.close()
    ctx.close()
    del ux, uid
    torch.cuda.empty_cache()


def _same_answer(got, want, what):
    assert got["ids"].shape == want["ids"].shape, what
    assert (got["ids"] == want["ids"]).all(), f"{what}: ids {_first_diff(got['ids'], want['ids'])}"
    assert (_bits(got["dist"]) == _bits(want["dist"])).all(), \
        f"{what}: distance bits {_first_diff(_bits(got['dist']), _bits(want['dist']))}"


def test_configs3_group_of_8_equals_one_store_bit_exact(configs3):
    s, g = configs3["single"], configs3["group"]
    assert configs3["layout"] == dict(size=G3, ntotal=N3, nlist=NLIST3, held=[(NLIST3 // G3, True)] * G3)  # list p on member p % 8
    for case in CASES3:
        what = f"(Q, k, nprobe, device buffers) = {case}; store form {s[case]['forms']!r}, member forms {g[case]['forms']}"
        assert s[case]["ids"].shape == case[:2], what
        assert (s[case]["ids"] >= ID_BASE3).all(), what  # every list holds more than k rows: no padding
        _same_answer(g[case], s[case], what)
    # device buffers in and out give what host buffers give
    _same_answer(s[(4096, 10, 8, True)], s[(4096, 10, 8, False)], "store, device vs host buffers")


def test_configs3_every_probed_list_is_read_once_by_its_owner(configs3):
    """the members' summed counters equal the one store's: each probed list was read exactly once, by the member that holds it"""
    s, g = configs3["single"], configs3["group"]
    for case in CASES3:
        Q, _, nprobe, _ = case
        what = (case, s[case]["pairs"], g[case]["pairs"], s[case]["bytes"], g[case]["bytes"])
        assert s[case]["pairs"] == Q * nprobe, what  # (no list is empty)
        assert g[case]["pairs"] == s[case]["pairs"], what
        assert g[case]["bytes"] == s[case]["bytes"] > 0, what


def test_configs3_sample_equals_the_oracle(configs3):
    """256 queries of the 4096 batch (query 0 and 4095 among them): the coarse step against the oracle's over the 65536
    centroids, the rows against the oracle's batched scan of the probed lists -- ids and distance bits"""
    c = configs3
    for p in (1, 8):
        (gp, gd), (op, od) = c["coarse_g"][p], c["coarse_o"][p]
        assert (gp == op).all(), f"coarse nprobe={p}: {_first_diff(gp, op)}"
        assert (_bits(gd) == _bits(od)).all(), f"coarse nprobe={p}: distance bits"
        oi, od = c["oracle"][p]
        assert (oi >= ID_BASE3).all()
        for name in ("group", "single"):
            r = c[name][(4096, 10, p, False)]
            _same_answer(dict(ids=r["ids"][c["sample"]], dist=r["dist"][c["sample"]]), dict(ids=oi, dist=od),
                         f"{name} vs oracle, nprobe={p}, forms {r['forms']}")


def _probed_rows(lists, uoff):
    """rows (of the sample's small CSR) of every query's probed lists, one query per row: lists [n, P] -> rows [n, m], valid [n, m]"""
    lo, hi = uoff[lists], uoff[lists + 1]
    end = (hi - lo).cumsum(1)
    start = end - (hi - lo)
    ar = torch.arange(int(end[:, -1].max()), device=lists.device)[None, :].expand(lists.shape[0], -1).contiguous()
    j = torch.searchsorted(end, ar, right=True).clamp_max(lists.shape[1] - 1)  # which probed list a position falls in
    valid = ar < end[:, -1:]
    rows = torch.where(valid, lo.gather(1, j) + ar - start.gather(1, j), lo[:, :1])  # (padding: a real row, masked out)
    return rows, valid


def test_configs3_sample_float64_judge(configs3):
    """the group's rows on the sample, judged in float64 over the query's probed lists: distances within 1e-4 of the returned
    id's row, (distance, id) order, no id twice, every id from a probed list, the float64 top-k wherever the gap to both
    neighbours exceeds 2e-4"""
    c, tol, k = configs3, 1e-4, 10
    dev = c["ux"].device
    uoff = torch.from_numpy(c["uoff"]).to(dev)
    for p in (1, 8):
        r = c["group"][(4096, k, p, False)]
        gi_all = torch.from_numpy(r["ids"][c["sample"]]).to(dev)
        gd_all = torch.from_numpy(r["dist"][c["sample"]]).to(dev)
        lists = torch.from_numpy(c["lists_u"][p]).to(dev)
        for s0 in range(0, lists.shape[0], 32):
            sl = slice(s0, s0 + 32)
            q, gi, gd = torch.from_numpy(c["qs"][sl]).to(dev), gi_all[sl], gd_all[sl]
            rows, valid = _probed_rows(lists[sl], uoff)
            cand_rows, cand_ids = c["ux"][rows], c["uid"][rows]
            hit = (gi[:, :, None] == cand_ids[:, None, :]) & valid[:, None, :]
            assert bool(hit.any(2).all()), f"nprobe={p}: an id from a list the query did not probe"
            d64 = torch.where(valid, _dist64(q, cand_rows, "l2"), torch.full_like(valid, float("inf"), dtype=torch.float64))
            own = torch.where(hit, d64[:, None, :], torch.full_like(d64[:, None, :], float("inf"))).amin(2)
            assert torch.allclose(gd.double(), own, atol=tol, rtol=0), f"nprobe={p}: a distance is not its id's"
            _check_rows_sorted(gi, gd, "l2")
            _check_exact(q, gi, gd, cand_rows, cand_ids, valid, k, "l2", tol)


def test_configs3_remove_1m_ids_at_size(configs3):
    """remove_ids of 1M ids spread over every list (+ 1000 absent, + 1000 repeats) on both indexes: the counts, the search
    afterwards (bit-equal between them, no removed id, unchanged wherever the earlier answer held no removed id) and get_vector"""
    c = configs3
    s, g = c["single"], c["group"]
    for name in ("single", "group"):
        assert (c[name]["removed"], c[name]["ntotal"]) == (KILL3, N3 - KILL3), name
    a, b = s["after"], g["after"]
    _same_answer(b, a, f"after the removal; store form {a['forms']!r}, member forms {b['forms']}")
    assert (a["ids"] >= ID_BASE3).all()
    assert not np.isin(a["ids"], c["kill"]).any()
    before = s[(4096, 10, 8, False)]
    untouched = ~np.isin(before["ids"], c["kill"]).any(1)
    assert untouched.mean() > 0.5
    _same_answer(dict(ids=a["ids"][untouched], dist=a["dist"][untouched]),
                 dict(ids=before["ids"][untouched], dist=before["dist"][untouched]), "rows without a removed id")
    for name in ("single", "group"):
        for i, (v, want) in enumerate(zip(c[name]["get"], c["probe_vecs"])):
            assert (v is None) == (i >= 16), (name, i)  # 16 survivors, then 16 removed ids
            if v is not None:
                assert (_bits(v) == _bits(want)).all(), (name, i)
