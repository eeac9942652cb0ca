"""The yardstick of grouped search (tests/grouped_yardstick.py) pinned on the CPU: with every id in a group of its own it is the
oracle's search bit for bit, and a case small enough to work out by hand comes out as worked out."""
import numpy as np
import pytest

import filter_yardstick as FY
import grouped_yardstick as GY
import oracle as O
import range_yardstick as RY


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("k", [1, 10, 70])
def test_unique_values_equal_search(metric, k):
    c = RY.corpus(32, 24, 5000, metric, seed=5 + (1 if metric == "ip" else 0))
    q = RY.queries(c, 21, seed=6)
    q[0] = c["cent"][2]                                               # its nearest list holds 5 rows: a padded answer
    vals = c["ids"] * 3 - 1000                                        # every id its own value
    for nprobe in (1, 5):
        want = O.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, batched_scan=True, num_threads=8)
        gi, gd, gg = GY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, metric, c["ids"], vals)
        np.testing.assert_array_equal(gi, want[0])
        np.testing.assert_array_equal(gd.view(np.uint32), want[1].view(np.uint32))
        np.testing.assert_array_equal(gg, np.where(gi >= 0, gi * 3 - 1000, 0))
        if nprobe == 1 and k > 5:
            assert (gi[0, 5:] == -1).all() and (gi[0, :5] >= 0).all()
    # a filter: the same over the reduced CSR
    S = FY.draw_set(c["ids"], 0.3, np.random.default_rng(7))
    want = FY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 5, k, metric, S, "deny")
    gi, gd, gg = GY.search(q, c["cent"], c["vecs"], c["ids"], c["offsets"], 5, k, metric, c["ids"], vals, S, "deny")
    np.testing.assert_array_equal(gi, want[0])
    np.testing.assert_array_equal(gd.view(np.uint32), want[1].view(np.uint32))


def test_hand_worked_case():
    """12 rows in two lists, the query at the origin, L2.  By hand: group 5 is represented by id 10 (ids 10 and 11 tie at 1, the
    NaN row 18 does not count), groups 8 and 7 tie at 4 and come in id order (3 before 12), group 9 has a NaN row only and is
    absent, id 15 -- the nearest row of all -- has no value and never appears."""
    nan = np.float32(np.nan)
    imin = np.iinfo(np.int64).min
    table = [  # id, vector, group (None: no value)
        (10, (1, 0), 5), (12, (2, 0), 7), (13, (3, 0), 7), (14, (nan, 0), 9), (15, (0.5, 0), None), (16, (0, 3), -1),
        (11, (0, 1), 5), (3, (0, 2), 8), (17, (4, 0), imin), (18, (nan, 1), 5), (19, (0, 5), 0), (20, (6, 0), 8)]
    ids = np.array([t[0] for t in table], np.int64)
    vecs = np.array([t[1] for t in table], np.float32)
    offsets = np.array([0, 6, 12], np.int64)
    attr_ids = np.array([t[0] for t in table if t[2] is not None], np.int64)
    attr_vals = np.array([t[2] for t in table if t[2] is not None], np.int64)
    q = np.zeros((1, 2), np.float32)
    gi, gd, gg = GY.scan(q, vecs, ids, offsets, np.array([[0, 1]], np.int64), 8, "l2", attr_ids, attr_vals)
    np.testing.assert_array_equal(gi[0], [10, 3, 12, 16, 17, 19, -1, -1])
    np.testing.assert_array_equal(gd[0], np.array([1, 2, 2, 3, 4, 5, np.inf, np.inf], np.float32))
    np.testing.assert_array_equal(gg[0], [5, 8, 7, -1, imin, 0, 0, 0])
    # k smaller than the number of groups cuts the same order; one list only sees its own rows
    gi, gd, gg = GY.scan(q, vecs, ids, offsets, np.array([[0, 1]], np.int64), 2, "l2", attr_ids, attr_vals)
    np.testing.assert_array_equal(gi[0], [10, 3])
    gi, gd, gg = GY.scan(q, vecs, ids, offsets, np.array([[1, -1]], np.int64), 3, "l2", attr_ids, attr_vals)
    np.testing.assert_array_equal(gi[0], [11, 3, 17])
    np.testing.assert_array_equal(gg[0], [5, 8, imin])
    # a filter that takes the best row of group 5 away: the next one represents it
    gi, gd, gg = GY.scan(q, vecs, ids, offsets, np.array([[0, 1]], np.int64), 2, "l2", attr_ids, attr_vals, S=[10], mode="deny")
    np.testing.assert_array_equal(gi[0], [11, 3])
    # IP: descending; every product with the zero query is 0, so the ids decide among the representatives
    gi, gd, gg = GY.scan(q, vecs, ids, offsets, np.array([[0, 1]], np.int64), 8, "ip", attr_ids, attr_vals)
    np.testing.assert_array_equal(gi[0], [3, 10, 12, 16, 17, 19, -1, -1])
