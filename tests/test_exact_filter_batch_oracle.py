"""Pins the yardstick of exact filtered search with one filter per query on the CPU (tests/exact_filter_batch_yardstick.py):
answering query i with the single-filter yardstick under filter qfilter[i] equals the oracle's batched scan over a CSR of F lists
-- list j = the kept rows of filter j in stored order -- with pids[i] = [qfilter[i]], ids and distance bits.  That is the
formulation the device route relies on: a pool store with one list per filter and the ordinary partition scan with P = 1.
Integer-valued rows give many equal keys, so the id order is exercised; one filter has no candidates and one query has pid -1."""
import numpy as np
import pytest

import exact_filter_batch_yardstick as B
import filter_yardstick as Y
from test_exact_filter_oracle import _corpus


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [8, 20])
def test_per_query_equals_one_list_per_filter(d, metric):
    vecs, ids, offsets, q, _ = _corpus(d, metric, seed=900 + d)
    rng = np.random.default_rng(d)
    specs = [(Y.draw_set(ids, 0.3, rng), "allow"), (Y.draw_set(ids, 0.01, rng), "allow"), (Y.draw_set(ids, 0.3, rng), "deny"),
             (np.zeros(0, np.int64), "allow"), (np.zeros(0, np.int64), "deny")]
    counts = B.candidates(ids, specs)
    assert counts[3] == 0 and counts[4] == ids.shape[0]
    qfilter = np.array([0, 1, 2, 3, 4, -1, 2, 1, 0], np.int32)  # every filter named, one query without a list
    assert qfilter.shape[0] == q.shape[0]
    ties = 0
    for k in (1, 10, 1000):
        ai, ad = B.search(q, vecs, ids, offsets, k, metric, specs, qfilter)
        oi, od = B.pool_scan(q, vecs, ids, k, metric, specs, qfilter)
        np.testing.assert_array_equal(ai, oi, err_msg=str(k))
        np.testing.assert_array_equal(ad.view(np.uint32), od.view(np.uint32), err_msg=str(k))
        for i, f in enumerate(qfilter):
            assert (ai[i] >= 0).sum() == (min(k, counts[f]) if f >= 0 else 0)
        assert (ai[5] == -1).all() and (np.isposinf(ad[5]) if metric == "l2" else np.isneginf(ad[5])).all()
        if k == 1000:
            ties += int((ad[:, 1:] == ad[:, :-1])[ai[:, 1:] >= 0].sum())
    assert ties > 0  # equal keys occurred: the id order was needed
