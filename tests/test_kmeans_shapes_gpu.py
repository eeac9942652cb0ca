"""The k-means kernels over the shapes of tests/kmeans_cases.py: every assign form (the 24 fp32 MFMA kernels with their tails, the
wide-row kernel on both sides of the LDS seam), both accumulate orders over the float / float4 forms with one and several trips, the
bucketing with doubled wave rows, qk_kmeans_update / qk_normalize_rows / qk_rand_perm, the edges of the Lloyd driver and
qk_store_refine_lists with its refusal.  Every comparison is bit for bit with the oracle: no tolerance anywhere (the float64 bounds
that vouch for the oracle live in tests/test_kmeans_cases_oracle.py, which also pins what the cases reach)."""
import numpy as np
import pytest

import kmeans_cases as K
import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- assign ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric", K.assign_groups())
def test_assign(ctx, d, metric):
    """the six (n, m, data) of one (d, metric), each four ways: host arrays with values, values=False, device tensors, device tensors
    again on the same context"""
    for n, m, kind in K.assign_group(d, metric):
        tag = "assign d=%d %s n=%d m=%d %s %s" % (d, metric, n, m, kind, K.assign_form(n, m, d, metric))
        x, c = K.assign_data(n, m, d, metric, kind)
        oa, ov = O.kmeans_assign(x, c, metric)
        ga, gv = ctx.kmeans_assign(x, c, metric)
        np.testing.assert_array_equal(ga, oa, err_msg=tag + " host")
        np.testing.assert_array_equal(_bits(gv), _bits(ov), err_msg=tag + " host values")
        ga, gv = ctx.kmeans_assign(x, c, metric, values=False)
        assert gv is None
        np.testing.assert_array_equal(ga, oa, err_msg=tag + " values=False")
        xd, cd = _dev(x), _dev(c)
        for again in range(2):
            da, dv = ctx.kmeans_assign(xd, cd, metric)
            np.testing.assert_array_equal(_host(da), oa, err_msg=tag + " device #%d" % again)
            np.testing.assert_array_equal(_bits(_host(dv)), _bits(ov), err_msg=tag + " device values #%d" % again)


@pytest.mark.parametrize("metric", K.METRICS)
def test_assign_across_the_lds_seam(ctx, metric):
    """the d = 2544 cases with one more zero column are d = 2545: k_assign<1, 1> on one side, k_assign_wide on the other.  An appended
    zero adds nothing to a dot product or a norm: the assignments are equal, and for L2 the value bits"""
    for n, m, kind in K.assign_group(2544, metric):
        assert K.assign_form(n, m, 2544, metric) == ("mfma", 1, 1) and K.assign_form(n, m, 2545, metric) == "wide"
        tag = "seam %s n=%d m=%d %s" % (metric, n, m, kind)
        x, c = K.assign_data(n, m, 2544, metric, kind)
        a0, v0 = ctx.kmeans_assign(x, c, metric)
        a1, v1 = ctx.kmeans_assign(K.pad_column(x), K.pad_column(c), metric)
        np.testing.assert_array_equal(a1, a0, err_msg=tag)
        if metric == "l2":
            np.testing.assert_array_equal(_bits(v1), _bits(v0), err_msg=tag + " values")


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", K.ORDERS)
@pytest.mark.parametrize("name,d", K.accumulate_cases())
def test_accumulate(ctx, name, d, order):
    blocked = order == "blocked"
    x, a, m, sizes = K.accumulate_data(name, d)
    n = x.shape[0]
    tag = "accumulate %s d=%d %s n=%d m=%d %s %s" % (name, d, order, n, m, K.blocked_form(n, m, d), K.bucket_plan(n, m))
    os_, oc = O.kmeans_accumulate(x, a, m, blocked=blocked)
    if sizes is not None:
        np.testing.assert_array_equal(oc, sizes)
    gs, gc = ctx.kmeans_accumulate(x, a, m, blocked=blocked)
    np.testing.assert_array_equal(gc, oc, err_msg=tag + " host")
    np.testing.assert_array_equal(_bits(gs), _bits(os_), err_msg=tag + " host")
    assert int(gc.sum()) == int(((a >= 0) & (a < m)).sum())
    if name == "large":
        return   # (host arrays only: the case is about the bucketing plan, and 270 MB go to the device once)
    xd, ad = _dev(x), _dev(a)
    for again in range(2):   # twice on one context: the tickets of the multi-group fold and the scan's totals are back at zero
        ds, dc = ctx.kmeans_accumulate(xd, ad, m, blocked=blocked)
        np.testing.assert_array_equal(_host(dc), oc, err_msg=tag + " device #%d" % again)
        np.testing.assert_array_equal(_bits(_host(ds)), _bits(os_), err_msg=tag + " device #%d" % again)


def test_accumulate_blocked_from_a_misaligned_x(ctx):
    """d % 4 == 0 but x starts 4 bytes into its buffer: k_accumulate_blocked<float> on a float4 shape, the same bits"""
    import torch
    name, d = K.MISALIGNED
    x, a, m, _ = K.accumulate_data(name, d)
    n = x.shape[0]
    os_, oc = O.kmeans_accumulate(x, a, m, blocked=True)
    buf = torch.empty(n * d + 1, dtype=torch.float32, device="cuda")
    xv = buf[1:].view(n, d)
    xv.copy_(torch.from_numpy(x))
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    ad = _dev(a)
    ms, mc = ctx.kmeans_accumulate(xv, ad, m, blocked=True)
    al, _ = ctx.kmeans_accumulate(_dev(x), ad, m, blocked=True)
    np.testing.assert_array_equal(_host(mc), oc)
    np.testing.assert_array_equal(_bits(_host(ms)), _bits(os_))
    np.testing.assert_array_equal(_bits(_host(ms)), _bits(_host(al)))


# ---- update, normalise, permutation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", K.UPDATE_D)
@pytest.mark.parametrize("m", K.UPDATE_M)
def test_kmeans_update(ctx, m, d):
    """qk_kmeans_update through its host path and its device path (finalize, counts read back, split on the host, written back)"""
    for pattern in K.UPDATE_PATTERNS:
        tag = "update m=%d d=%d %s" % (m, d, pattern)
        sums, counts, cent = K.update_case(m, d, pattern)
        oc, ocnt = O.kmeans_update(sums, counts, cent)
        hc, hcnt = ctx.kmeans_update(sums, counts.copy(), cent.copy())
        np.testing.assert_array_equal(hcnt, ocnt, err_msg=tag + " host")
        np.testing.assert_array_equal(_bits(hc), _bits(oc), err_msg=tag + " host")
        dc, dcnt = ctx.kmeans_update(_dev(sums), _dev(counts), _dev(cent))
        np.testing.assert_array_equal(_host(dcnt), ocnt, err_msg=tag + " device")
        np.testing.assert_array_equal(_bits(_host(dc)), _bits(oc), err_msg=tag + " device")


@pytest.mark.parametrize("d", K.NORM_D)
def test_normalize_rows(ctx, d):
    for n in K.NORM_N:
        x = K.normalize_case(n, d)
        want = O.normalize_rows(x)
        np.testing.assert_array_equal(_bits(ctx.normalize_rows(x.copy())), _bits(want), err_msg="normalize n=%d d=%d host" % (n, d))
        np.testing.assert_array_equal(_bits(_host(ctx.normalize_rows(_dev(x)))), _bits(want), err_msg="normalize n=%d d=%d device" % (n, d))


def test_rand_perm(ctx):
    for n, m, seed in K.PERM_CASES:
        got, want = ctx.rand_perm(n, m, seed), O.rand_perm(n, m, seed)
        assert got.shape == (min(n, m),)
        np.testing.assert_array_equal(got, want, err_msg="rand_perm %r" % ((n, m, seed),))
        assert len(set(got.tolist())) == len(got) and ((got >= 0) & (got < max(n, 1))).all()


# ---- the Lloyd driver -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d,metric,niter", K.DRIVER_CASES)
def test_kmeans_driver(ctx, n, m, d, metric, niter):
    """host arrays, then kmeans_inplace on device tensors (IP: x is normalised in place): centroids, assignments and x_used"""
    import torch
    x = K.driver_data(n, m, d, metric, niter)
    oc, oa, ox = O.kmeans(x, m, metric, niter=niter, seed=K.DRIVER_SEED)
    gc, ga, gx = ctx.kmeans(x, m, metric, niter=niter, seed=K.DRIVER_SEED)
    np.testing.assert_array_equal(_bits(gx), _bits(ox))
    np.testing.assert_array_equal(_bits(gc), _bits(oc))
    np.testing.assert_array_equal(ga, oa)
    assert int(np.bincount(ga, minlength=m).sum()) == n and ga.min() >= 0 and ga.max() < m
    xd = _dev(x)
    cd = torch.empty((m, d), dtype=torch.float32, device="cuda")
    ad = torch.empty((n,), dtype=torch.int64, device="cuda")
    ctx.kmeans_inplace(xd, m, metric, cd, ad, niter=niter, seed=K.DRIVER_SEED)
    np.testing.assert_array_equal(_bits(_host(xd)), _bits(ox))
    np.testing.assert_array_equal(_bits(_host(cd)), _bits(oc))
    np.testing.assert_array_equal(_host(ad), oa)


# ---- refine_lists ---------------------------------------------------------------------------------------------------------------
def _store(ctx, ivf):
    from quake_amd.capi import Store
    s = Store(ctx, ivf["d"])
    s.build_csr(ivf["offsets"], ivf["ids"], ivf["vecs"])
    return s


def _lists_equal(s, sel, ov, oi, oo):
    total = 0
    for c, p in enumerate(sel):
        gv, gi = s.get_list(int(p))
        np.testing.assert_array_equal(gi, oi[oo[c]:oo[c + 1]])
        np.testing.assert_array_equal(_bits(gv), _bits(ov[oo[c]:oo[c + 1]]))
        total += len(gi)
    return total


def _untouched(s, ivf, but=()):
    for p in range(K.REFINE_LISTS):
        if p not in but:
            gv, gi = s.get_list(p)
            np.testing.assert_array_equal(gi, ivf["part_ids"][p])
            np.testing.assert_array_equal(_bits(gv), _bits(ivf["part_vecs"][p]))


@pytest.mark.parametrize("iters", K.REFINE_ITERS)
@pytest.mark.parametrize("selection", sorted(K.REFINE_SELECTIONS))
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", K.REFINE_D)
def test_refine_lists(ctx, d, metric, selection, iters):
    ivf, sel, cent = K.refine_case(d, metric, selection)
    vecs, ids, offs = K.refine_csr(ivf, sel)
    oc, ov, oi, oo = O.kmeans_refine_partitions(cent, vecs, ids, offs, metric, iters)
    s = _store(ctx, ivf)
    try:
        gc = s.refine_lists(sel, cent, metric, iters)
        np.testing.assert_array_equal(_bits(gc), _bits(oc))
        total = _lists_equal(s, sel, ov, oi, oo)
        assert total == len(ids) and s.ntotal() == len(ivf["ids"])
        _untouched(s, ivf, but=set(sel.tolist()))
    finally:
        s.close()


def test_refine_lists_refuses_an_emptied_cluster(ctx):
    """the second centroid receives no row at the first assignment; at the second iteration its mean is 0 / 0 and the call fails
    with the library's error, which names the unassigned vectors.  The store is untouched and the context's scratch pool is usable
    again: a following refine_lists on the same context succeeds and equals the oracle.

    (A NaN centroid loses every comparison, so no row is ever dropped: the library counts the clusters that hold no row when their
    centroid is recomputed and refuses after the passes, before the store or the caller's centroids are written.)"""
    from quake_amd._lib import QuakeHipError
    ivf, sel, cent = K.refusal_case()
    metric = K.REFUSAL["metric"]
    s = _store(ctx, ivf)
    try:
        with pytest.raises(QuakeHipError) as err:
            s.refine_lists(sel, cent, metric, K.REFUSAL["iterations"])
        assert "could not be assigned" in str(err.value) and "vectors" in str(err.value), str(err.value)
        _untouched(s, ivf)
        assert s.ntotal() == len(ivf["ids"])
        vecs, ids, offs = K.refine_csr(ivf, sel)
        oc, ov, oi, oo = O.kmeans_refine_partitions(cent, vecs, ids, offs, metric, 0)
        gc = s.refine_lists(sel, cent, metric, 0)
        np.testing.assert_array_equal(_bits(gc), _bits(oc))
        assert _lists_equal(s, sel, ov, oi, oo) == len(ids) and s.ntotal() == len(ivf["ids"])
        _untouched(s, ivf, but=set(sel.tolist()))
    finally:
        s.close()

