"""The numpy model of the shadow form's exact finish (tests/shadow_finish_yardstick.py) pinned on the host: for CONSISTENT records
-- approximate keys within E of the exact ones, dropped rows at or above a full record's last key -- the rule's answer is the
oracle's single-probe search, whether a query verifies or falls back.  tests/test_shadow_finish.py then holds the kernel to the
model."""
import numpy as np
import pytest

import oracle as O
import shadow_finish_yardstick as Y
from helpers import make_ivf, make_queries


def test_key_maps_round_trip_and_order():
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, 7.25, np.inf], np.float32)
    for metric in ("l2", "ip"):
        vv = v[4:] if metric == "l2" else v
        k = Y.key_of(vv, metric)
        back = Y.value_of(k, metric)
        assert (back[vv != 0] == vv[vv != 0]).all() and (back[vv == 0] == 0).all()
        order = np.argsort(k, kind="stable")
        assert (np.diff(vv[order]) >= 0).all() if metric == "l2" else (np.diff(vv[order]) <= 0).all()
    assert Y.key_of(np.float32(np.nan), "l2") == Y.NONE and Y.key_of(np.float32(np.nan), "ip") == Y.NONE
    assert Y.key_of(np.float32(-0.0), "ip") == Y.key_of(np.float32(0.0), "ip")


def test_widen_moves_outwards():
    for metric in ("l2", "ip"):
        for val, E in ((1.0, 0.25), (3.0, 0.0), (100.0, 1e-3), (0.0, 0.5)):
            k0 = Y.key_of(np.float32(val if metric == "l2" else -val), metric)[()]
            k1 = Y.widen(k0, E, metric)
            assert k1 > k0  # (even E = 0 moves one step: the rounding is outwards)
            moved = float(Y.value_of(k1, metric)) - float(Y.value_of(k0, metric))
            assert (moved if metric == "l2" else -moved) >= E
    assert Y.widen(Y.NONE, 1.0, "l2") == Y.NONE and Y.widen(Y.NONE, 1.0, "ip") == Y.NONE


@pytest.mark.parametrize("d,metric,k,scale", [(20, "l2", 10, 0.02), (128, "l2", 16, 0.05), (48, "ip", 1, 0.02), (8, "ip", 10, 0.3), (136, "l2", 10, 1.0)])
def test_consistent_records_give_the_oracles_search(d, metric, k, scale):
    ivf = make_ivf(3000, d, 12, seed=5 + d, metric=metric, empty=(3,))
    q = make_queries(48, d, seed=6 + d, like=ivf["x"], metric=metric)
    pid, _ = O.coarse(q, ivf["centroids"], None, 1, metric)
    lists = pid[:, 0].copy()
    # E in proportion to the spread of a query's exact values: small ones verify, large ones cannot and fall back
    spread = np.array([np.ptp(O.pair_values(q[i:i + 1], ivf["vecs"][ivf["offsets"][p]:ivf["offsets"][p + 1]], metric)[0]) if p != 3 else 1.0
                       for i, p in enumerate(lists)])  # (a query next to the empty list's centroid has nothing to score)
    E = (scale * spread * np.linspace(0.05, 1.0, q.shape[0])).astype(np.float32)
    recs = Y.consistent_records(q, E, lists, ivf["offsets"], ivf["vecs"], metric, seed=d)
    m = Y.model(q, E, lists, recs, ivf["offsets"], ivf["vecs"], ivf["ids"], k, metric)
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, k, metric, batched_scan=True)
    np.testing.assert_array_equal(m["ids"], oi)
    np.testing.assert_array_equal(m["dist"].view(np.uint32), od.view(np.uint32))
    nothing = np.array([ivf["offsets"][p + 1] == ivf["offsets"][p] for p in lists])  # (next to the empty list's centroid)
    assert ((m["verified"] ^ m["fallback"]) | nothing).all()
    if scale <= 0.05:
        assert m["verified"].sum() >= q.shape[0] // 2, "the small bounds must verify: the rule itself is what is compared"
        assert (m["candidates"][m["verified"]] >= k).all()
    if scale >= 0.3:
        assert m["fallback"].any(), "a bound as wide as the spread cannot verify"


def test_queries_without_records_or_bound_fall_back():
    d, k, metric = 20, 10, "l2"
    ivf = make_ivf(1500, d, 6, seed=3, empty=(2,))
    q = np.stack([ivf["part_vecs"][p][0] for p in (0, 1, 3, 4, 5, 0)]) + np.float32(0.01)
    pid, _ = O.coarse(q, ivf["centroids"], None, 1, metric)
    lists = pid[:, 0].copy()
    assert (lists != 2).all()
    E = np.array([0.01, -1.0, np.nan, 0.01, 0.01, 0.01], np.float32)
    recs = Y.consistent_records(q, np.abs(np.nan_to_num(E)), lists, ivf["offsets"], ivf["vecs"], metric, seed=1)
    recs.pair_slots[3, 0] = 0  # no record at all
    lists[4] = 2               # an empty list is probed: nothing to fall back to
    recs.pair_slots[4, 0] = 0
    m = Y.model(q, E, lists, recs, ivf["offsets"], ivf["vecs"], ivf["ids"], k, metric)
    assert list(m["fallback"]) == [False, True, True, True, False, False] and list(m["verified"]) == [True, False, False, False, False, True]
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, k, metric, batched_scan=True)
    keep = [0, 1, 2, 3, 5]
    np.testing.assert_array_equal(m["ids"][keep], oi[keep])
    np.testing.assert_array_equal(m["dist"][keep].view(np.uint32), od[keep].view(np.uint32))
    assert (m["ids"][4] == -1).all() and np.isinf(m["dist"][4]).all()
    assert m["candidates"][1] == 0 and m["candidates"][2] == 0  # (a query without a bound never looks at its records)
