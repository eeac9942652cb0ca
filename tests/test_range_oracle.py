"""Pins tests/range_yardstick.py on the CPU: the rows it returns are the rows a float64 brute force puts inside the radius (rows
within 1e-4 relative of the radius may fall on either side), in scan order, with monotone lims; and the filtered yardstick is the
yardstick over the reduced store."""
import numpy as np
import pytest

import filter_yardstick as FY
import oracle as O
import range_yardstick as RY


def _brute64(q, c, pids, metric):
    """float64 distances of every (query, probed row), as (query, CSR row) -> value in scan order"""
    out = []
    v64 = c["vecs"].astype(np.float64)
    for i in range(q.shape[0]):
        rows = np.concatenate([np.arange(c["offsets"][p], c["offsets"][p + 1]) for p in pids[i] if p >= 0] + [np.zeros(0, np.int64)])
        x = q[i].astype(np.float64)
        dv = np.sqrt(((v64[rows] - x) ** 2).sum(1)) if metric == "l2" else v64[rows] @ x
        out.append((rows.astype(np.int64), dv))
    return out


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_yardstick_against_float64(metric):
    c = RY.corpus(32, 24, 4000, metric, seed=3)
    q = RY.queries(c, 48, seed=4)
    pids = RY.probed(q, c["cent"], c["offsets"], 6, metric)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    b64 = _brute64(q, c, pids, metric)
    # scan order: a query's rows are its lists in rank order, each in stored order
    for i in range(q.shape[0]):
        np.testing.assert_array_equal(pairs[1][pairs[0][i]:pairs[0][i + 1]], b64[i][0])
        np.testing.assert_allclose(pairs[2][pairs[0][i]:pairs[0][i + 1]], b64[i][1], rtol=7e-5, atol=7e-5)
    alld = np.sort(pairs[2])
    radii = [alld[alld.shape[0] // 1000], alld[alld.shape[0] // 20], alld[alld.shape[0] // 2]]
    if metric == "ip":
        radii = [alld[-1 - alld.shape[0] // 1000], alld[-1 - alld.shape[0] // 20], alld[alld.shape[0] // 2]]
    for r in radii + [np.inf if metric == "l2" else -np.inf]:
        lims, gi, gd = RY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 6, r, metric)
        assert lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == gi.shape[0] == gd.shape[0]
        for i in range(q.shape[0]):
            rows, dv = b64[i]
            r64 = float(np.float32(r))
            inside = dv <= r64 if metric == "l2" else dv >= r64
            near = np.abs(dv - r64) <= 1e-4 * max(abs(r64), 1e-30) if np.isfinite(r64) else np.zeros_like(inside)
            got = gi[lims[i]:lims[i + 1]]
            must, may = c["ids"][rows[inside & ~near]], c["ids"][rows[inside | near]]
            assert np.isin(must, got).all() and np.isin(got, may).all(), (metric, r, i)
            # scan order: the positions of the returned ids in the query's row sequence increase
            where = {int(v): j for j, v in enumerate(c["ids"][rows])}
            seq = [where[int(v)] for v in got]
            assert seq == sorted(seq)
        if not np.isfinite(r):
            assert gi.shape[0] == pairs[1].shape[0]


def test_filtered_yardstick_is_the_yardstick_over_the_reduced_store():
    c = RY.corpus(32, 24, 4000, "l2", seed=5)
    q = RY.queries(c, 31, seed=6)
    rng = np.random.default_rng(7)
    pairs = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], RY.probed(q, c["cent"], c["offsets"], 5, "l2"), "l2")
    r = np.sort(pairs[2])[pairs[2].shape[0] // 10]
    for sel, mode in [(0.5, "allow"), (0.01, "deny"), (0, "allow")]:
        S = FY.draw_set(c["ids"], sel, rng)
        lims, gi, gd = RY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 5, r, "l2", S, mode)
        fv, fi, fo = FY.reduced_csr(c["vecs"], c["ids"], c["offsets"], FY.allowed_rows(c["ids"], S, mode))
        l2, i2, d2 = RY.search(q, c["cent"], fv, fi, fo, 5, r, "l2")
        np.testing.assert_array_equal(lims, l2)
        np.testing.assert_array_equal(gi, i2)
        np.testing.assert_array_equal(gd.view(np.uint32), d2.view(np.uint32))
        # ... and it is the unfiltered answer with the other rows taken out, order kept
        ul, ui, ud = RY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 5, r, "l2")
        keep = np.isin(ui, S) if mode == "allow" else ~np.isin(ui, S)
        np.testing.assert_array_equal(gi, ui[keep])
        np.testing.assert_array_equal(gd.view(np.uint32), ud[keep].view(np.uint32))


def test_edge_lists():
    c = RY.corpus(16, 12, 600, "l2", seed=8)
    q = RY.queries(c, 3, seed=9)
    pids = np.array([[-1, 5, 0], [-1, -1, -1], [99, 4, 2]], np.int64)  # -1, an empty list (0), a list number out of range
    lims, gi, gd = RY.scan(q, c["vecs"], c["ids"], c["offsets"], pids, np.inf, "l2")
    sizes = np.diff(c["offsets"])
    assert sizes[0] == 0
    np.testing.assert_array_equal(np.diff(lims), [sizes[5], 0, sizes[4] + sizes[2]])
    np.testing.assert_array_equal(gi[lims[2]:], np.concatenate([c["ids"][c["offsets"][4]:c["offsets"][5]], c["ids"][c["offsets"][2]:c["offsets"][3]]]))
