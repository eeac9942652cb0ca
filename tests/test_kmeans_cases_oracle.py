"""On the CPU: the cases of the k-means shape sweep (tests/kmeans_cases.py, run on the device by tests/test_kmeans_shapes_gpu.py)
reach what they are for, and the expected values can be trusted: the oracle's answers are checked against float64 with derived
bounds (u = 2^-24), so the device comparison does not rest on the project's own restatement alone.  These are conditions on the
cases: where a draw misses one, the draw changes and the condition stays."""
import zlib

import numpy as np
import pytest

import kmeans_cases as K
import oracle as O

U = K.U
FORMS = [("mfma", DB, NQ) for DB in (8, 4, 2, 1) for NQ in (4, 2, 1)]


# ---- coverage, from the restated rules ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", K.METRICS)
def test_every_assign_form_is_reached_with_its_tails(metric):
    """each of the 12 (DB, NQ) forms of this metric (24 kernels in all): a ragged last row tile, a ragged last centroid tile, fewer
    than 4 centroid tiles, odd and even nsteps, a tie across waves; the n <= 16 override for every DB; both sides of the LDS seam"""
    facts, at_d = set(), {}
    for d in K.ASSIGN_D:
        pairs = K.assign_group(d, metric)
        assert len(pairs) == K.PAIRS and len(set(pairs)) == K.PAIRS
        for n, m, kind in pairs:
            assert n < K.APF_MIN_ROWS and n in K.ASSIGN_N and m in K.ASSIGN_M and kind in K.KINDS
            form = K.assign_form(n, m, d, metric)
            assert form != "pf"
            at_d.setdefault(d, set()).add(form)
            facts |= K.assign_facts(n, m, d, kind)
    for form in FORMS:
        for prop in K.PROPS:
            assert (form, prop) in facts, (form, prop)
    for DB in (8, 4, 2, 1):
        assert (("mfma", DB, 1), "override") in facts
    assert at_d[2544] == {("mfma", 1, 1)} and at_d[2545] == {"wide"} and at_d[2560] == {"wide"}
    assert ("wide", "tie") in facts and ("wide", "mrag") in facts and ("wide", "nrag") in facts


def test_the_restated_seam_and_bands():
    assert K.assign_form(1000, 64, 256) == ("mfma", 8, 4) and K.assign_form(1000, 64, 257) == ("mfma", 1, 2)
    assert K.assign_form(1000, 64, 512) == ("mfma", 8, 2) and K.assign_form(1000, 64, 513) == ("mfma", 1, 1)
    assert K.assign_form(16, 64, 64) == ("mfma", 4, 1) and K.assign_form(17, 64, 64) == ("mfma", 4, 4)
    assert K.assign_form(1000, 64, 2544) == ("mfma", 1, 1) and K.assign_form(1000, 64, 2545) == "wide"
    assert K.assign_form(40960, 64, 128) == "pf" and K.assign_form(40960, 64, 128, aligned=False) == ("mfma", 8, 4)
    assert K.bucket_plan(70001, 255)[:2] == (8, 1) and K.bucket_plan(70001, 4096)[:2] == (12, 1) and K.bucket_plan(70001, 4097)[:2] == (12, 2)


def test_the_draws_of_the_assign_cases_did_not_move():
    """a checksum of the drawn (n, m, kind): a change of the generator, the pools or the redraw rule shows here, not silently"""
    text = repr([(d, metric, K.assign_group(d, metric)) for d, metric in K.assign_groups()])
    assert zlib.crc32(text.encode()) == DRAWS_CRC, zlib.crc32(text.encode())


DRAWS_CRC = 2847238299


# ---- the oracle's assign against float64 ----------------------------------------------------------------------------------------
def _assign_bound_holds(x, c, metric, oa):
    """for each row, D in float64 and a = the oracle's choice: D[a] - min D <= B[a] + B[argmin], with
    L2: B = (d + 4) u (|x|^2 + |c|^2 + 2 |x|.|c|)    IP: B = (d + 4) u |x|.|c|"""
    d = x.shape[1]
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    dot, adot = x64 @ c64.T, np.abs(x64) @ np.abs(c64).T
    if metric == "l2":
        xn, cn = (x64 * x64).sum(1)[:, None], (c64 * c64).sum(1)[None, :]
        D, B = xn + cn - 2.0 * dot, (d + 4) * U * (xn + cn + 2.0 * adot)
    else:
        D, B = -dot, (d + 4) * U * adot
    rows = np.arange(x.shape[0])
    best = D.argmin(1)
    gap = D[rows, oa] - D[rows, best]
    return gap, B[rows, oa] + B[rows, best]


@pytest.mark.parametrize("d,metric", K.assign_groups())
def test_assign_oracle_against_float64(d, metric):
    for n, m, kind in K.assign_group(d, metric):
        x, c = K.assign_data(n, m, d, metric, kind)
        assert x.shape == (n, d) and c.shape == (m, d) and np.isfinite(x).all() and np.isfinite(c).all()
        oa, ov = O.kmeans_assign(x, c, metric)
        assert ((oa >= 0) & (oa < m)).all()
        gap, bound = _assign_bound_holds(x, c, metric, oa)
        assert (gap <= bound).all(), (n, m, kind, float((gap - bound).max()))
        # the lower index wins: no bit-equal copy of the chosen centroid lies below it
        first = {}
        for j in range(m):
            first.setdefault(c[j].tobytes(), j)
        assert all(first[c[a].tobytes()] == a for a in np.unique(oa)), (n, m, kind)
        if kind == "mixture" and metric == "ip" and m <= min(d, 130):
            assert (ov < 0).any(), (n, m)   # a row whose best dot product is negative: a zero centroid would beat it
        if kind == "ties":
            copies = [j for j in range(m) if first[c[j].tobytes()] != j]
            assert copies, (n, m)
            chosen = set(oa.tolist())
            won = [j for j in copies if first[c[j].tobytes()] in chosen]   # a row's best centroid has a copy above it
            assert won, (n, m)
            if m >= 17:   # ... in another wave's tile range
                assert any(K.wave_of_centroid(j, m) != K.wave_of_centroid(first[c[j].tobytes()], m) for j in won), (n, m)


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
def _f64_sums(x, a, m):
    """(S, A, cnt): float64 sums of the rows and of their absolute values per centroid, rows out of range ignored"""
    n, d = x.shape
    ok = (a >= 0) & (a < m)
    cnt = np.bincount(a[ok], minlength=m).astype(np.int64)
    S, A = np.zeros((m, d)), np.zeros((m, d))
    if d <= 8:
        idx = a[ok]
        for k in range(d):
            col = x[ok, k].astype(np.float64)
            S[:, k], A[:, k] = np.bincount(idx, col, m), np.bincount(idx, np.abs(col), m)
    else:
        for c in range(m):
            v = x[a == c].astype(np.float64)
            S[c], A[c] = v.sum(0), np.abs(v).sum(0)
    return S, A, cnt


@pytest.mark.parametrize("name,d", K.accumulate_cases())
def test_accumulate_oracle_against_float64(name, d):
    """sums, either order: |s - S| <= gamma sum|x_i| per component, gamma = (cnt - 1) u / (1 - (cnt - 1) u); the prescribed sizes
    really are the sizes after the out-of-range rows are dropped"""
    x, a, m, sizes = K.accumulate_data(name, d)
    assert np.isfinite(x).all()
    S, A, cnt = _f64_sums(x, a, m)
    if sizes is not None:
        np.testing.assert_array_equal(cnt, sizes)
    if name not in ("n0",):
        assert set(K.out_of_range(m)) <= set(a.tolist())
    k = np.maximum(cnt - 1, 0).astype(np.float64)[:, None]
    gamma = k * U / (1.0 - k * U)
    for blocked in (False, True):
        s, oc = O.kmeans_accumulate(x, a, m, blocked=blocked)
        np.testing.assert_array_equal(oc, cnt)
        assert (np.abs(s.astype(np.float64) - S) <= gamma * A).all(), (name, d, blocked)


def test_accumulate_forms_are_reached():
    seen = set()
    for name, d in K.accumulate_cases():
        if name in ("large", "n0"):
            n, m, sizes = (K.LARGE["n"], K.LARGE["m"], None) if name == "large" else (0, 3, None)
        else:
            x, a, m, sizes = K.accumulate_data(name, d)
            n = x.shape[0]
        V, units, TPC, NCH, trips, lanes = K.blocked_form(n, m, d)
        bits, passes, wave_rows, nchunks = K.bucket_plan(n, m)
        G = max(K.groups_of(int(s)) for s in sizes) if sizes is not None else None
        seen |= {(V, "trips>1" if trips > 1 else "trips1"), ("NCH", "1" if NCH == 1 else "several"), ("bits", bits),
                 ("reference trips", K.reference_order_trips(d))}
        if G is not None and G > lanes:
            seen.add(("lanes", lanes, "G", G))
        if name == "large":
            assert (bits, passes, wave_rows) == (12, 1, 2048) and nchunks > 2048
            assert K.bucket_plan(2 ** 24, m)[2] == 1024   # the branch starts above 4096 chunks
        if name == "m257":
            assert (bits, passes) == (12, 1)
    want = {("float", "trips>1"), ("float4", "trips>1"), ("float", "trips1"), ("float4", "trips1"), ("NCH", "1"), ("NCH", "several"),
            ("bits", 8), ("bits", 12), ("lanes", 2, "G", 4), ("lanes", 8, "G", 10), ("reference trips", 1), ("reference trips", 2)}
    assert want <= seen, want - seen
    assert K.blocked_form(*_shape(K.MISALIGNED), aligned=True)[0] == "float4"      # d % 4 == 0 ...
    assert K.blocked_form(*_shape(K.MISALIGNED), aligned=False)[:2] == ("float", 64)   # ... and the float kernel by misalignment
    assert K.blocked_form(100, 3, 1028)[:5] == ("float4", 257, 256, 1, 2) and K.blocked_form(100, 3, 1101)[:5] == ("float", 1101, 256, 1, 5)
    assert set(K.ACC_SIZES) == set(K.ARRANGEMENTS["lanes8"]) and set(K.ARRANGEMENTS["lanes2"]) <= set(K.ACC_SIZES)


def _shape(case):
    x, a, m, _ = K.accumulate_data(*case)
    return x.shape[0], m, x.shape[1]


# ---- update, normalise, permutation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.UPDATE_M)
def test_update_patterns_are_what_they_say(m):
    for pattern in K.UPDATE_PATTERNS:
        sums, counts, cent = K.update_case(m, 3, pattern)
        oc, ocnt = O.kmeans_update(sums, counts, cent)
        assert ocnt.sum() == counts.sum() and np.isfinite(oc).all()
        if pattern == "full":
            assert (counts > 0).all() and (ocnt == counts).all()
        if pattern == "nosplit":
            assert (counts == 0).any() and counts.max() < 2 and (ocnt == counts).all()
            np.testing.assert_array_equal(oc[counts == 0], cent[counts == 0])      # an empty cluster keeps its centroid
        if pattern == "donor" and m >= 2:
            assert (counts == 0).any() and (ocnt > 0).all()
        if pattern == "tied" and m >= 3:
            top = np.nonzero(counts == counts.max())[0]
            assert len(top) == 2 and ocnt[top[0]] < counts[top[0]]                  # the lower index donates first


def test_normalize_cases_have_no_zero_row():
    for n in K.NORM_N:
        for d in K.NORM_D:
            x = K.normalize_case(n, d)
            y = O.normalize_rows(x)
            assert np.isfinite(y).all()
            np.testing.assert_allclose(np.linalg.norm(y.astype(np.float64), axis=1), 1.0, rtol=1e-5)


# ---- driver and refine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d,metric,niter", K.DRIVER_CASES)
def test_driver_cases_run_through_the_oracle(n, m, d, metric, niter):
    x = K.driver_data(n, m, d, metric, niter)
    c, a, xu = O.kmeans(x, m, metric, niter=niter, seed=K.DRIVER_SEED)
    assert np.isfinite(c).all() and np.isfinite(xu).all()
    assert np.bincount(a, minlength=m).sum() == n and ((a >= 0) & (a < m)).all()
    if d in (2544, 2545):
        assert K.assign_form(n, m, d, metric) == {2544: ("mfma", 1, 1), 2545: "wide"}[d]


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", K.REFINE_D)
def test_refine_cases_empty_no_cluster(d, metric):
    for selection in K.REFINE_SELECTIONS:
        ivf, sel, cent = K.refine_case(d, metric, selection)
        sizes = [len(ivf["part_ids"][p]) for p in sel]
        assert (0 in sizes) == (selection == "with_empty") and len(ivf["part_ids"]) == K.REFINE_LISTS
        vecs, ids, offs = K.refine_csr(ivf, sel)
        moved = False
        for iters in K.REFINE_ITERS:
            oc, ov, oi, oo = O.kmeans_refine_partitions(cent, vecs, ids, offs, metric, iters)
            assert np.isfinite(oc).all() and oo[-1] == len(ids) and (np.diff(oo) > 0).all(), (selection, iters)
            moved = moved or not np.array_equal(oo, offs)
        assert moved or len(sel) == 1


def test_the_refusal_case_empties_the_second_cluster():
    ivf, sel, cent = K.refusal_case()
    vecs, ids, offs = K.refine_csr(ivf, sel)
    a, _ = O.kmeans_assign(vecs, cent, K.REFUSAL["metric"])
    assert len(ids) > 0 and (a == 0).all()                     # the first assignment leaves the second centroid with count 0
    oc, _, _, _ = O.kmeans_refine_partitions(cent, vecs, ids, offs, K.REFUSAL["metric"], K.REFUSAL["iterations"])
    assert np.isnan(oc[1]).all() and np.isfinite(oc[0]).all()  # ... and its mean is 0 / 0 at the second iteration
