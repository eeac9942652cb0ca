"""Pins the yardstick of exact filtered search on the CPU (tests/exact_filter_yardstick.py): the filter yardstick with every list
probed equals the oracle's scan over the kept rows as ONE list -- ids and distance bits -- because a row's key is one k-ordered
fmaf chain that does not depend on its neighbours and results are ordered by (key, id).  Integer-valued rows give many equal
keys, so the id order is exercised.  It also pins that the exact answer contains whatever a fixed-nprobe filtered search finds:
against the fixed-nprobe yardstick its recall is 1 and no distance of it is worse."""
import numpy as np
import pytest

import exact_filter_yardstick as E
import filter_yardstick as Y

SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 1203]


def _corpus(d, metric, seed):
    rng = np.random.default_rng(seed)
    sizes = np.array(SIZES, np.int64)
    offsets = np.zeros(sizes.shape[0] + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    n = int(offsets[-1])
    vecs = rng.integers(-2, 3, size=(n, d)).astype(np.float32)  # few distinct values: many ties
    ids = rng.permutation(n).astype(np.int64) * 5 + 3
    q = rng.integers(-2, 3, size=(9, d)).astype(np.float32)
    cent = np.stack([vecs[offsets[i]:offsets[i + 1]].mean(0) if sizes[i] else np.full(d, 9.0, np.float32) for i in range(sizes.shape[0])])
    return vecs, ids, offsets, q, cent.astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [8, 20, 128])
def test_all_lists_equals_one_list(d, metric):
    vecs, ids, offsets, q, _ = _corpus(d, metric, seed=400 + d)
    rng = np.random.default_rng(d)
    ties = 0
    for sel in (0, 0.01, 0.3, 1):
        S = Y.draw_set(ids, sel, rng)
        for mode in ("allow", "deny"):
            for k in (1, 10, 100):
                ai, ad = E.search(q, vecs, ids, offsets, k, metric, S, mode)
                oi, od = E.one_list(q, vecs, ids, k, metric, S, mode)
                np.testing.assert_array_equal(ai, oi, err_msg=str((sel, mode, k)))
                np.testing.assert_array_equal(ad.view(np.uint32), od.view(np.uint32), err_msg=str((sel, mode, k)))
                n = E.candidates(ids, S, mode)
                assert ((ai >= 0).sum(axis=1) == min(k, n)).all()
                if k == 100 and n >= 100:
                    ties += int((ad[:, 1:] == ad[:, :-1]).sum())
    assert ties > 0  # equal keys occurred: the id order was needed


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_exact_contains_the_probed_answer(metric):
    vecs, ids, offsets, q, cent = _corpus(20, metric, seed=77)
    rng = np.random.default_rng(5)
    for sel in (0.01, 0.3):
        S = Y.draw_set(ids, sel, rng)
        ei, ed = E.search(q, vecs, ids, offsets, 10, metric, S, "allow")
        for nprobe in (1, 3, len(SIZES)):
            pi, pd = Y.search(q, cent, vecs, ids, offsets, nprobe, 10, metric, S, "allow")
            # position by position the exact answer is at least as good, and with every list probed the two are the same
            live = pi >= 0
            assert (ei >= 0)[live].all()
            assert (ed[live] <= pd[live]).all() if metric == "l2" else (ed[live] >= pd[live]).all()
            for a in range(q.shape[0]):
                # a row both answers hold has the same distance bits in both; a probed row that the exact answer leaves out is
                # no better than the last row of the exact answer, which is then full
                at = {int(i): j for j, i in enumerate(ei[a]) if i >= 0}
                both = live[a] & np.isin(pi[a], ei[a][ei[a] >= 0])
                np.testing.assert_array_equal(pd[a][both].view(np.uint32), ed[a][[at[int(i)] for i in pi[a][both]]].view(np.uint32))
                out = live[a] & ~both
                if out.any():
                    assert ei[a, -1] >= 0
                    assert (pd[a][out] >= ed[a, -1]).all() if metric == "l2" else (pd[a][out] <= ed[a, -1]).all()
            if nprobe == len(SIZES):
                assert E.recall(pi, ei) == 1.0
                np.testing.assert_array_equal(pi, ei)
                np.testing.assert_array_equal(pd.view(np.uint32), ed.view(np.uint32))
