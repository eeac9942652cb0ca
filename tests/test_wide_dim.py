"""Wide rows: d up to QK_MAX_D = 8192, beyond what a 16-query tile in LDS allows (k_scan_wide / k_dense_wide / k_assign_wide,
qk_scan_wide.hip).  Every check is bit for bit against the oracle's canonical arithmetic: qk_search and qk_coarse + qk_scan over
d x metric x k (pools, and key emission beyond QK_MAX_K) x nprobe with empty lists and lists shorter than k; the seam where the
LDS-staged kernels hand over (either kernel, same bits; routing asserted); the index surface in both mirrors at d = 3072 (build =
the oracle's k-means, flat index, add / remove / maintenance, recall-target walk, device group, save -> load); and d above the
envelope is refused with QK_ERR_UNSUPPORTED."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu


def _corpus(d, nlist, n, metric, seed, empty=2):
    """clustered rows in skewed lists: `empty` empty lists, a few lists shorter than any k used below"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 0.05
    w[:empty] = 0.0
    w[empty:empty + 2] = 1e-4  # a handful of rows at most
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) + 7
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return dict(cent=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets, x=x,
                rng=rng)


def _queries(c, Q, d):
    rng = c["rng"]
    return (c["x"][rng.integers(0, c["x"].shape[0], size=Q)] + 0.05 * rng.standard_normal((Q, d))).astype(np.float32)


def _stores(ctx, c, d):
    from quake_amd.capi import Store
    s = Store(ctx, d)
    s.build_csr(c["offsets"], c["ids"], c["vecs"])
    nlist = c["cent"].shape[0]
    parent = Store(ctx, d)
    parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), c["cent"])
    return s, parent


def _eq(gi, gd, oi, od, tag):
    np.testing.assert_array_equal(gi, oi, err_msg=str(tag))
    np.testing.assert_array_equal(np.asarray(gd).view(np.uint32), np.asarray(od).view(np.uint32), err_msg=str(tag))


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


# (k, nprobe, Q): k in the pools (1 ... 448) and beyond them (1000: key emission + bisection select), one and several lists
_CASES = [(1, 1, 33), (10, 8, 1024), (100, 1, 33), (448, 8, 33), (1000, 8, 33), (10, 1, 1), (100, 8, 33), (448, 1, 1),
          (1000, 1, 33), (1, 8, 33)]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [2560, 3072, 4096, 4100, 8192])
def test_search_and_scan_bit_exact(ctx, d, metric):
    n = 2400 if d < 8192 else 1200
    c = _corpus(d, 12, n, metric, seed=d + (metric == "ip"))
    s, parent = _stores(ctx, c, d)
    try:
        for k, nprobe, Q in _CASES:
            if d >= 4100 and Q > 33:
                Q = 33  # (the oracle's time, not the kernel's)
            q = _queries(c, Q, d)
            tag = dict(d=d, metric=metric, k=k, nprobe=nprobe, Q=Q)
            oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, batched_scan=True, num_threads=8)
            gi, gd = ctx.search(parent, s, q, nprobe, k, metric)
            _eq(gi, gd, oi, od, tag)
            pids, _ = ctx.coarse(parent, q, nprobe, metric)
            op, _ = O.coarse(q, c["cent"], None, nprobe, metric)
            np.testing.assert_array_equal(pids[:, :op.shape[1]], op, err_msg=str(tag))
            gi, gd = ctx.scan(s, q, pids, k, metric)
            _eq(gi, gd, oi, od, dict(tag, form=ctx.last_scan_kernel()))
    finally:
        s.close()
        parent.close()


def test_seam_either_kernel_same_bits(ctx):
    """d across the hand-over of the LDS-staged scan (k = 10 / 64 / 100 near d ~ 2300-2500, k = 448 near d ~ 1200): every case
    equals the oracle whichever kernel serves it, and both kernels occur"""
    rng = np.random.default_rng(77)
    forms = set()
    cases = [(d, k) for d in range(2176, 2625, 16) for k in (10, 64, 100)] + [(d, 448) for d in range(1152, 1265, 16)]
    for d, k in cases:
        metric = "l2" if rng.random() < 0.5 else "ip"
        c = _corpus(d, 8, 700, metric, seed=int(rng.integers(1 << 30)), empty=1)
        s, parent = _stores(ctx, c, d)
        try:
            q = _queries(c, 40, d)
            pids, _ = ctx.coarse(parent, q, 3, metric)
            gi, gd = ctx.scan(s, q, pids, k, metric)
            forms.add(ctx.last_scan_kernel())
            oi, od = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 3, k, metric, batched_scan=True, num_threads=8)
            _eq(gi, gd, oi, od, dict(d=d, k=k, metric=metric, form=ctx.last_scan_kernel()))
        finally:
            s.close()
            parent.close()
    assert "k_scan_wide" in forms and any(f.startswith("k_scan") and f != "k_scan_wide" for f in forms), forms


@pytest.mark.parametrize("d, wide", [(2048, False), (3072, True)])
def test_routing(ctx, d, wide):
    c = _corpus(d, 8, 1500, "l2", seed=5)
    s, parent = _stores(ctx, c, d)
    try:
        q = _queries(c, 64, d)
        pids, _ = ctx.coarse(parent, q, 2, "l2")
        ctx.scan(s, q, pids, 10, "l2")
        kern = ctx.last_scan_kernel()
        if wide:
            assert kern == "k_scan_wide", kern
        else:
            assert kern.startswith("k_scan") and kern != "k_scan_wide", kern
    finally:
        s.close()
        parent.close()


def test_kmeans_assign_bit_exact(ctx):
    rng = np.random.default_rng(3)
    for d, m, metric in ((3072, 40, "l2"), (4100, 17, "ip"), (8192, 5, "l2")):
        x = rng.standard_normal((500, d)).astype(np.float32)
        cent = rng.standard_normal((m, d)).astype(np.float32)
        a, v = ctx.kmeans_assign(x, cent, metric)
        oa, ov = O.kmeans_assign(x, cent, metric)
        np.testing.assert_array_equal(np.asarray(a), oa, err_msg=str((d, m, metric)))
        np.testing.assert_array_equal(np.asarray(v).view(np.uint32), ov.view(np.uint32), err_msg=str((d, m, metric)))


@pytest.fixture(scope="module")
def qb():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    return b


def _index_corpus(n=8000, d=3072, nc=32, seed=21):
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(nc, d, generator=g)
    x = cent[torch.randint(0, nc, (n,), generator=g)] + 0.3 * torch.randn(n, d, generator=g)
    q = cent[torch.randint(0, nc, (40,), generator=g)] + 0.3 * torch.randn(40, d, generator=g)
    return x.contiguous(), torch.arange(n), q.contiguous()


def _build(mod, x, ids, nlist, metric="l2", workers=0):
    bp = mod.IndexBuildParams()
    bp.nlist, bp.metric, bp.num_workers = nlist, metric, workers
    idx = mod.QuakeIndex()
    idx.build(x, ids, bp)
    return idx


def _params(mod, k, nprobe):
    sp = mod.SearchParams()
    sp.k, sp.nprobe = k, nprobe
    return sp


def _same(ra, rb):
    assert torch.equal(ra.ids.cpu(), rb.ids.cpu())
    assert torch.equal(ra.distances.cpu().contiguous().view(torch.int32), rb.distances.cpu().contiguous().view(torch.int32))


def test_build_equals_oracle_kmeans(qb):
    """QuakeIndex.build at d = 3072 in both mirrors: centroids = the oracle's k-means, list p = the rows the oracle assigns to
    centroid p, and the search over the built index = the oracle's"""
    import quake_amd as qa
    x, ids, q = _index_corpus()
    oc, oa, _ = O.kmeans(x.numpy(), 32, "l2", niter=5, seed=1234)
    py, comp = _build(qa, x, ids, 32), _build(qb, x, ids, 32)
    for idx in (py, comp):
        assert idx.ntotal() == 8000 and idx.nlist() == 32
        np.testing.assert_array_equal(idx.parent.get(torch.arange(32)).numpy().view(np.uint32), oc.view(np.uint32))
    for p in range(32):
        _, pid = py._store.get_list(p)
        np.testing.assert_array_equal(np.sort(pid), np.nonzero(oa == p)[0])
    pv, pi = zip(*[py._store.get_list(p) for p in range(32)])
    vecs, aids, offs = O.csr_from_partitions(pv, pi, 3072)
    for k, nprobe in ((10, 4), (100, 1)):
        oi, od = O.search(q.numpy(), oc, vecs, aids, offs, nprobe, k, "l2", batched_scan=True, num_threads=8)
        for idx, mod in ((py, qa), (comp, qb)):
            r = idx.search(q, _params(mod, k, nprobe))
            _eq(r.ids.numpy(), r.distances.numpy(), oi, od, ("built index", k, nprobe))


def test_flat_index_equals_oracle(qb):
    import quake_amd as qa
    x, ids, q = _index_corpus(n=3000, d=4096, seed=4)
    for mod in (qb, qa):
        idx = _build(mod, x, ids, 0)
        for k in (1, 10, 1000):
            r = idx.search(q, _params(mod, k, 1))
            offs = np.array([0, 3000], np.int64)
            oi, od = O.batched_serial_scan(q.numpy(), x.numpy(), ids.numpy(), offs, np.zeros((40, 1), np.int64), k, "l2", num_threads=8)
            _eq(r.ids.numpy(), r.distances.numpy(), oi, od, ("flat", k))


def _oracle_of(idx, d):
    """the python mirror's partitions and centroids as a CSR in ascending list number (the oracle's tie order)"""
    cent, cids = idx.parent._store.get_list(0)
    order = np.argsort(cids)
    pv, pi = zip(*[idx._store.get_list(int(p)) for p in cids[order]])
    vecs, aids, offs = O.csr_from_partitions(pv, pi, d)
    return cent[order], vecs, aids, offs


def test_add_remove_maintenance(tmp_path):
    import quake_amd as qa
    from quake_amd.maintenance import (DEFAULT_LATENCY_ESTIMATOR_RANGE_K, DEFAULT_LATENCY_ESTIMATOR_RANGE_N,
                                       ListScanLatencyEstimator, MaintenanceCostEstimator)
    d = 3072
    x, ids, q = _index_corpus(n=6000, d=d, nc=16, seed=8)
    idx = _build(qa, x, ids, 16)
    lat = ListScanLatencyEstimator(d, DEFAULT_LATENCY_ESTIMATOR_RANGE_N, DEFAULT_LATENCY_ESTIMATOR_RANGE_K, 1,
                                   profile_fn=lambda n, k: 100.0 + 1.0 * n)
    prof = str(tmp_path / "latency.csv")
    assert lat.save_latency_profile(prof)
    mp = qa.MaintenancePolicyParams()
    mp.window_size, mp.refinement_radius, mp.refinement_iterations = 200, 4, 1
    mp.split_threshold_ns, mp.delete_threshold_ns, mp.min_partition_size = 0.1, 0.1, 8
    idx.initialize_maintenance_policy(mp, cost_estimator=MaintenanceCostEstimator(d, mp.alpha, 10, latency_estimator=lat))

    def check(tag):
        ids_now = idx.get_ids()
        assert idx.ntotal() == ids_now.numel() == torch.unique(ids_now).numel()
        cent, vecs, aids, offs = _oracle_of(idx, d)
        assert offs[-1] == idx.ntotal()
        for k, nprobe in ((10, 4), (100, 2)):
            r = idx.search(q, _params(qa, k, nprobe))
            oi, od = O.search(q.numpy(), cent, vecs, aids, offs, nprobe, k, "l2", batched_scan=True, num_threads=8)
            _eq(r.ids.numpy(), r.distances.numpy(), oi, od, (tag, k, nprobe))

    check("built")
    g = torch.Generator().manual_seed(2)
    nx = x[torch.randint(0, 6000, (500,), generator=g)] + 0.05 * torch.randn(500, d, generator=g)
    assert idx.add(nx, torch.arange(50000, 50500)).n_vectors == 500
    check("add")
    idx.remove(torch.arange(0, 6000, 5))
    check("remove")
    idx.track_hits = True  # (only the window below counts: the parity searches above do not)
    idx.search(q[:10].repeat(40, 1), _params(qa, 10, 3))  # a skewed window: a few lists hot, the others cold
    idx.track_hits = False
    idx.maintenance()
    check("maintenance")


def test_recall_target_walk(ctx):
    d = 3072
    for metric in ("l2", "ip"):
        c = _corpus(d, 24, 3000, metric, seed=31, empty=1)
        s, parent = _stores(ctx, c, d)
        try:
            q = _queries(c, 20, d)
            for rt, frac in ((0.9, 0.2), (0.99, 0.5)):
                gi, gd, gn = ctx.search_aps(parent, s, q, 10, metric, rt, initial_search_fraction=frac)
                oi, od, on = O.search_aps(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 10, metric, rt, initial_search_fraction=frac,
                                          expanded=True, num_threads=8)
                np.testing.assert_array_equal(gn, on)
                _eq(gi, gd, oi, od, (metric, rt, frac))
        finally:
            s.close()
            parent.close()


@pytest.mark.parametrize("mirror", ["compiled", "python"])
def test_workers_same_bits(qb, mirror):
    import quake_amd as qa
    mod = qb if mirror == "compiled" else qa
    x, ids, q = _index_corpus(n=5000, d=3072, nc=16, seed=12)
    a = _build(mod, x, ids, 16, workers=0)
    b = _build(mod, x, ids, 16, workers=2)
    for k, nprobe in ((10, 1), (10, 4), (100, 3)):
        _same(a.search(q, _params(mod, k, nprobe)), b.search(q, _params(mod, k, nprobe)))


@pytest.mark.parametrize("mirror", ["compiled", "python"])
def test_save_load_roundtrip(qb, mirror, tmp_path):
    import quake_amd as qa
    mod = qb if mirror == "compiled" else qa
    x, ids, q = _index_corpus(n=3000, d=4096, nc=8, seed=6)
    a = _build(mod, x, ids, 8)
    path = str(tmp_path / "idx")
    a.save(path)
    b = mod.QuakeIndex()
    b.load(path)
    assert b.ntotal() == 3000 and b.nlist() == 8
    _same(a.search(q, _params(mod, 10, 3)), b.search(q, _params(mod, 10, 3)))


def test_above_the_envelope_is_refused(ctx):
    from quake_amd._lib import QuakeHipError
    d = 8208
    c = _corpus(d, 4, 200, "l2", seed=1, empty=0)
    s, parent = _stores(ctx, c, d)
    try:
        q = _queries(c, 40, d)
        with pytest.raises(QuakeHipError) as e:
            pids, _ = ctx.coarse(parent, q, 2, "l2")
            ctx.scan(s, q, pids, 10, "l2")
        assert "QK_ERR_UNSUPPORTED" in str(e.value) and "8192" in str(e.value)
        with pytest.raises(QuakeHipError) as e:
            ctx.kmeans_assign(c["x"], c["cent"], "l2")
        assert "QK_ERR_UNSUPPORTED" in str(e.value)
    finally:
        s.close()
        parent.close()
