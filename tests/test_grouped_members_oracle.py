"""The yardstick of grouped search with members (tests/grouped_members_yardstick.py) pinned on the CPU: at m = 1, and in member 0
at any m, it is the one-row yardstick; with one group and k = 1 it is the oracle's scan with k = m; with every id its own group it
is the oracle's search with padding behind it; and cases small enough to work out by hand come out as worked out.  The header and
the ctypes table carry the new entry points."""
import os
import re

import numpy as np
import pytest

import grouped_members_yardstick as GMY
import grouped_yardstick as GY
import oracle as O
import range_yardstick as RY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32))
    if len(a) > 2 and len(b) > 2:
        np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_member_zero_is_the_one_row_yardstick(metric):
    c = RY.corpus(32, 24, 5000, metric, seed=15 + (1 if metric == "ip" else 0))
    q = RY.queries(c, 21, seed=16)
    ids = c["ids"]
    for vals in (ids % 60 - 30, np.full(ids.shape[0], 9, np.int64)):
        pids = GY.probed(q, c["cent"], c["offsets"], 5, metric)
        for k in (1, 10, 70):
            one = GY.scan(q, c["vecs"], ids, c["offsets"], pids, k, metric, ids, vals)
            _same(GMY.scan(q, c["vecs"], ids, c["offsets"], pids, k, 1, metric, ids, vals), (one[0][:, :, None], one[1][:, :, None], one[2]))
            for m in (2, 16):
                wi, wd, wg = GMY.scan(q, c["vecs"], ids, c["offsets"], pids, k, m, metric, ids, vals)
                _same((wi[:, :, 0], wd[:, :, 0], wg), one)
                # members ascend under (distance, id), padding only behind live members, every member of its group
                live = wi >= 0
                assert (live[:, :, :-1] >= live[:, :, 1:]).all()
                col = dict(zip(ids.tolist(), vals.tolist()))
                for i, j, r in zip(*np.nonzero(live)):
                    assert col[int(wi[i, j, r])] == wg[i, j]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_one_group_is_the_scan(metric):
    c = RY.corpus(32, 24, 5000, metric, seed=25)
    q = RY.queries(c, 21, seed=26)
    q[0] = c["cent"][2]
    ids = c["ids"]
    vals = np.full(ids.shape[0], -5, np.int64)
    for nprobe in (1, 5):
        pids = GY.probed(q, c["cent"], c["offsets"], nprobe, metric)
        for m in (1, 3, 16):
            want = O.batched_serial_scan(q, c["vecs"], ids, c["offsets"], pids, m, metric)
            wi, wd, wg = GMY.scan(q, c["vecs"], ids, c["offsets"], pids, 1, m, metric, ids, vals)
            _same((wi[:, 0, :], wd[:, 0, :]), want)
            assert (wg[wi[:, 0, 0] >= 0] == -5).all()
            if nprobe == 1 and m == 16:   # the nearest list of query 0 holds 5 rows: padding inside the one live group
                assert (wi[0, 0, 5:] == -1).all() and (wi[0, 0, :5] >= 0).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_own_groups_are_the_search(metric):
    c = RY.corpus(32, 24, 5000, metric, seed=35)
    q = RY.queries(c, 21, seed=36)
    ids = c["ids"]
    vals = ids * 3 - 1000
    for k in (1, 10, 70):
        want = O.search(q, c["cent"], c["vecs"], ids, c["offsets"], 5, k, metric, batched_scan=True, num_threads=8)
        wi, wd, wg = GMY.search(q, c["cent"], c["vecs"], ids, c["offsets"], 5, k, 3, metric, ids, vals)
        _same((wi[:, :, 0], wd[:, :, 0]), want)
        assert (wi[:, :, 1:] == -1).all() and np.isinf(wd[:, :, 1:]).all()


def _hand():
    """3 groups of 1, 2 and 5 rows in two lists, the query at the origin, L2 (distances are the first coordinate).  Group 7: ids 40
    and 41 tie at distance 2, then 42 (3), 43 (4), 44 (5).  Group 8: id 30 at 1.5 and the NaN row 31.  Group 9: id 20 at 1.  Id 50,
    the nearest row of all, has no value; group 6 has a NaN row only."""
    nan = np.float32(np.nan)
    table = [  # id, vector, group
        (41, (2, 0), 7), (20, (1, 0), 9), (44, (5, 0), 7), (31, (nan, 0), 8), (50, (0.5, 0), None), (60, (nan, 1), 6),
        (40, (0, 2), 7), (30, (1.5, 0), 8), (43, (4, 0), 7), (42, (0, 3), 7), (32, (2.5, 0), 8)]
    ids = np.array([t[0] for t in table], np.int64)
    vecs = np.array([t[1] for t in table], np.float32)
    offsets = np.array([0, 6, 11], np.int64)
    attr_ids = np.array([t[0] for t in table if t[2] is not None], np.int64)
    attr_vals = np.array([t[2] for t in table if t[2] is not None], np.int64)
    return ids, vecs, offsets, attr_ids, attr_vals


def test_hand_worked_case():
    ids, vecs, offsets, ai, av = _hand()
    q = np.zeros((1, 2), np.float32)
    both = np.array([[0, 1]], np.int64)
    inf = np.inf
    # group sizes 1 (9), 2 (8: 30 and 32; the NaN row 31 is no member) and 5 (7), at m = 3; the tie of 40 and 41 in id order
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 4, 3, "l2", ai, av)
    np.testing.assert_array_equal(wi[0], [[20, -1, -1], [30, 32, -1], [40, 41, 42], [-1, -1, -1]])
    np.testing.assert_array_equal(wd[0], np.array([[1, inf, inf], [1.5, 2.5, inf], [2, 2, 3], [inf, inf, inf]], np.float32))
    np.testing.assert_array_equal(wg[0], [9, 8, 7, 0])
    # the tie straddles the cut at m = 1; k cuts groups, not rows
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 3, 1, "l2", ai, av)
    np.testing.assert_array_equal(wi[0, :, 0], [20, 30, 40])
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 2, 16, "l2", ai, av)
    np.testing.assert_array_equal(wg[0], [9, 8])
    assert (wi[0, 1, :2] == [30, 32]).all() and (wi[0, :, 2:] == -1).all()
    # one list sees its own rows only
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, np.array([[1, -1]], np.int64), 3, 3, "l2", ai, av)
    np.testing.assert_array_equal(wi[0], [[30, 32, -1], [40, 42, 43], [-1, -1, -1]])
    # NaN rows are never members, a group of NaN rows only is absent, a row without a value never appears
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 8, 16, "l2", ai, av)
    assert not np.isin([31, 60, 50], wi).any() and 6 not in wg[0]
    assert sorted(wi[wi >= 0].tolist()) == [20, 30, 32, 40, 41, 42, 43, 44]


def test_filter_moves_members_up():
    ids, vecs, offsets, ai, av = _hand()
    q = np.zeros((1, 2), np.float32)
    both = np.array([[0, 1]], np.int64)
    # group 7 loses its best row (40) and its third (42): the allowed rows move up, the group stays where its best allowed row puts it
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 3, 3, "l2", ai, av, S=[40, 42], mode="deny")
    np.testing.assert_array_equal(wi[0], [[20, -1, -1], [30, 32, -1], [41, 43, 44]])
    np.testing.assert_array_equal(wd[0, 2], np.array([2, 4, 5], np.float32))
    # ... and behind group 8 once both rows at distance 2 are gone
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 3, 3, "l2", ai, av, S=[40, 41, 30], mode="deny")
    np.testing.assert_array_equal(wg[0], [9, 8, 7])
    np.testing.assert_array_equal(wi[0], [[20, -1, -1], [32, -1, -1], [42, 43, 44]])
    # a group all of whose rows are disallowed is absent
    wi, wd, wg = GMY.scan(q, vecs, ids, offsets, both, 3, 3, "l2", ai, av, S=[20], mode="deny")
    np.testing.assert_array_equal(wg[0], [8, 7, 0])


def test_abi_declares_the_member_entry_points():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    syms = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", txt))
    assert {"qk_search_grouped_n", "qk_scan_grouped_n", "qk_search_grouped", "qk_scan_grouped"} <= syms
    assert re.search(r"^#define\s+QK_MAX_GROUP_SIZE\s+16\b", txt, re.M)
    for name in ("qk_search_grouped", "qk_scan_grouped"):
        old = re.search(r"QK_API int %s\((.*?)\);" % name, txt, re.S).group(1)
        new = re.search(r"QK_API int %s_n\((.*?)\);" % name, txt, re.S).group(1)
        norm = lambda s: [a.strip() for a in " ".join(s.split()).split(",")]   # noqa: E731
        o, n = norm(old), norm(new)
        at = o.index("int k")
        assert n == o[:at + 1] + ["int group_size"] + o[at + 1:], name          # the old list with group_size behind k
    from quake_amd import _lib
    for name in ("qk_search_grouped", "qk_scan_grouped"):
        assert name + "_n" in _lib.SIGNATURES
        r0, a0 = _lib.SIGNATURES[name]
        r1, a1 = _lib.SIGNATURES[name + "_n"]
        assert r0 is r1 and len(a1) == len(a0) + 1
