"""The oracle's rule for non-finite values (oracle/quake_oracle.c, "Non-finite values"): a (query, row) pair whose
canonical value is NaN is never a candidate -- whatever the NaN's sign, payload or position and whichever scan form --, +-inf are
ordinary floats, -0 and +0 tie and the lower id goes first.  CPU only: this file pins the checker the GPU tests compare with
(tests/test_nonfinite_search.py)."""
import numpy as np
import pytest

import filter_yardstick as FY
import nonfinite_yardstick as NF
import oracle as O
import range_yardstick as RY

NAN_WORDS = {"positive": 0x7FC00000, "negative": 0xFFC00000}


def _flat(seed=1, n=200, d=16, nq=20):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return x, np.arange(n, dtype=np.int64), np.array([0, n], np.int64), q


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("sign", ["positive", "negative"])
@pytest.mark.parametrize("row", [3, 150])
def test_a_nan_row_is_dropped_wherever_it_sits(metric, sign, row):
    """200 rows, one NaN coordinate, k = 5: the reference's buffer returned the row first from row 3 and never from row 150 -- here
    both placements, both signs, serial and batched give the answer on the same data with that row deleted"""
    x, ids, offsets, q = _flat()
    x.view(np.uint32)[row, 7] = NAN_WORDS[sign]
    keep = np.ones(200, bool)
    keep[row] = False
    rv, ri, ro = FY.reduced_csr(x, ids, offsets, keep)
    pids = np.zeros(1, np.int64)
    for scan in (O.batched_serial_scan, O.serial_scan):
        gi, gd = scan(q, x, ids, offsets, pids, 5, metric)
        ei, ed = scan(q, rv, ri, ro, pids, 5, metric)
        np.testing.assert_array_equal(gi, ei)
        np.testing.assert_array_equal(gd.view(np.uint32), ed.view(np.uint32))
        assert not (gi == row).any() and not np.isnan(gd).any()
    # fewer than k other rows: the NaN row does not surface behind them either, the padding does
    gi, gd = O.batched_serial_scan(q, x[row - 2:row + 1], ids[row - 2:row + 1], np.array([0, 3], np.int64), pids, 5, metric)
    np.testing.assert_array_equal(gi[:, 2:], -1)
    assert (np.sort(gi[:, :2], axis=1) == np.array([row - 2, row - 1])).all()
    assert (gd[:, 2:] == (-np.inf if metric == "ip" else np.inf)).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", NF.CLASSES)
def test_search_is_the_rule_applied_to_the_pair_values(cls, metric):
    """every input class of the GPU tests, Q <= 64: O.search equals the brute-force reference written from the per-pair values
    (drop NaN, sort by (value, id), take k, sqrt for L2, pad) -- a NaN can depend on the pair (inf * 0, inf - inf, overflowed norms)"""
    c = NF.corpus(cls, metric, 4000, 16, 32, seed=3)
    q, special = NF.queries(c, 48, seed=4)
    for nprobe, k in ((1, 10), (4, 10), (16, 300)):
        oi, od = NF.expected(c, q, nprobe, k)
        bi, bd = NF.brute(q, c["centroids"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric)
        NF.assert_same_answer(oi, od, bi, bd)
        NF.assert_no_nan_pair(c, q, special, oi)
        assert not np.isnan(od).any()
    val = O.pair_values(q, c["vecs"][c["special"]], metric)
    if cls == "underflow":
        assert not np.isnan(val).any()
    elif (cls, metric) == ("overflow", "ip"):
        assert np.isinf(val).any()  # (unit rows: no single product overflows, the sums do -- infinite values of either sign, no NaN)
    else:
        assert np.isnan(val).any(), "the class is meant to produce NaN pairs"


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_infinite_values_are_returned_in_front_of_the_padding(metric):
    """contract 2: a row at +inf (L2) / -inf (IP) comes back with its own id; only then the padding"""
    x, ids, offsets, q = _flat(seed=5, n=6, d=8, nq=4)
    if metric == "l2":
        x[2] *= NF.TWO64       # the norm overflows, the products do not: +inf (an infinite coordinate would give inf - inf = NaN)
    else:
        x[2, 3] = -np.inf
        q[:, 3] = np.abs(q[:, 3]) + 1.0
    x[4, 1] = np.nan
    gi, gd = O.batched_serial_scan(q, x, ids, offsets, np.zeros(1, np.int64), 8, metric)
    np.testing.assert_array_equal(gi[:, 4], 2)
    assert (gd[:, 4] == (np.inf if metric == "l2" else -np.inf)).all()
    np.testing.assert_array_equal(gi[:, 5:], -1)
    assert not (gi == 4).any()


def test_signed_zeros_tie_and_the_lower_id_goes_first():
    d = 16
    x = np.stack([np.full(d, -NF.ZP, np.float32), np.full(d, NF.ZP, np.float32)])
    q = np.full((1, d), NF.ZP, np.float32)
    val = O.pair_values(q, x, "ip")[0]
    assert val[0] == 0 and val[1] == 0 and np.signbit(val[0]) and not np.signbit(val[1])  # the chains end in -0.0 and +0.0
    offsets, pids = np.array([0, 2], np.int64), np.zeros(1, np.int64)
    for ids in (np.array([5, 9], np.int64), np.array([9, 5], np.int64)):
        for scan in (O.batched_serial_scan, O.serial_scan):
            gi, gd = scan(q, x, ids, offsets, pids, 2, "ip")
            np.testing.assert_array_equal(gi[0], [5, 9])
            assert (gd == 0).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_coarse_step_never_probes_a_nan_centroid(metric):
    rng = np.random.default_rng(6)
    cent = rng.standard_normal((12, 8)).astype(np.float32)
    q = rng.standard_normal((5, 8)).astype(np.float32)
    cent.view(np.uint32)[0, 2] = 0x7FC00000
    cent.view(np.uint32)[7, 0] = 0xFFC00000
    op, od = O.coarse(q, cent, None, 12, metric)
    np.testing.assert_array_equal(op[:, 10:], -1)                # fewer than kk centroids remain: padded with -1
    assert not np.isin(op, [0, 7]).any() and not np.isnan(od).any()
    assert (np.sort(op[:, :10], axis=1) == np.array([1, 2, 3, 4, 5, 6, 8, 9, 10, 11])).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("cls", ["nan", "inf", "overflow"])
def test_the_range_yardstick_refuses_nan_pairs_and_keeps_infinite_ones(cls, metric):
    """range_yardstick.all_pairs holds every pair, NaN included (it no longer goes through the top-k buffer); passes() refuses the
    NaN ones at every radius, and the widest radius (+inf for L2, -inf for IP) returns every other row, +-inf ones included"""
    c = NF.corpus(cls, metric, 3000, 12, 32, seed=8)
    q, _ = NF.queries(c, 16, seed=9)
    pids = O.coarse(q, c["centroids"], None, 4, metric)[0]
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    lims, rows, dist = pairs
    assert lims[-1] == rows.shape[0] == sum(int(c["offsets"][p + 1] - c["offsets"][p]) for p in pids.reshape(-1) if p >= 0)
    wide = np.inf if metric == "l2" else -np.inf
    wl, wi, wd = RY.select(pairs, c["ids"], wide, metric)
    assert wl[-1] == (~np.isnan(dist)).sum() and not np.isnan(wd).any()
    if cls != "overflow":      # (an overflowed query probes the lists of the lowest numbers: no NaN pair is certain there)
        assert np.isnan(dist).any()
    if cls != "nan":
        assert np.isinf(wd).any()
    fl, fi, fd = RY.select(pairs, c["ids"], 1.0 if metric == "l2" else 0.5, metric)
    assert np.isfinite(fd).all() if metric == "l2" else not np.isnan(fd).any()
