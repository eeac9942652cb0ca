"""Pins the yardstick of filtered search on the CPU (tests/filter_yardstick.py): the oracle's search over the CSR with the
disallowed rows deleted equals "scan the probed lists with k larger than their total rows, drop the disallowed ids, cut at k" --
ids and distance bits, both metrics, selectivity from 1 down to 0 -- so the expected values of the GPU test are not an invention.
Each row's distance is one k-ordered fmaf chain that does not depend on its neighbours, which is why deleting rows changes no bit."""
import numpy as np
import pytest

import oracle as O
from filter_yardstick import allowed_rows, draw_set, search as filtered_search
from helpers import make_ivf, make_queries

N, D, NLIST, K, NPROBE, NQ = 20000, 64, 32, 10, 1, 64
SELECTIVITIES = [1, 0.5, 0.1, 0.01, 0.0005, 0]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_reduced_csr_equals_overfetch_then_drop(metric):
    ivf = make_ivf(N, D, NLIST, seed=21, metric=metric, empty=(3, 17))
    q = make_queries(NQ, D, seed=22, like=ivf["x"], metric=metric)
    sizes = np.diff(ivf["offsets"])
    assert sizes[3] == 0 and sizes[17] == 0
    # every row of the probed list(s), in order: k' beyond the largest total a query can see
    kbig = int(np.sort(sizes)[::-1][:NPROBE].sum()) + 1
    ai, ad = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], NPROBE, kbig, metric, batched_scan=True)
    pad = np.float32(np.inf) if metric == "l2" else np.float32(-np.inf)
    rng = np.random.default_rng(23)
    padded = []
    for sel in SELECTIVITIES:
        S = draw_set(ivf["ids"], sel, rng)
        fi, fd = filtered_search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], NPROBE, K, metric, S, "allow")
        ei = np.full((NQ, K), -1, np.int64)
        ed = np.full((NQ, K), pad, np.float32)
        for r in range(NQ):
            keep = (ai[r] >= 0) & np.isin(ai[r], S)
            m = min(K, int(keep.sum()))
            ei[r, :m] = ai[r][keep][:m]
            ed[r, :m] = ad[r][keep][:m]
        np.testing.assert_array_equal(fi, ei, err_msg=f"{metric} selectivity {sel}")
        np.testing.assert_array_equal(fd.view(np.uint32), ed.view(np.uint32), err_msg=f"{metric} selectivity {sel}")
        assert np.isin(fi[fi >= 0], S).all()
        padded.append(float((fi < 0).mean()))
        # the complement as a deny-set is the same filter
        deny = np.setdiff1d(ivf["ids"], S)
        di, dd = filtered_search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], NPROBE, K, metric, deny, "deny")
        np.testing.assert_array_equal(di, fi)
        np.testing.assert_array_equal(dd.view(np.uint32), fd.view(np.uint32))
    assert padded[-1] == 1.0 and padded == sorted(padded)  # nothing allowed: padding only; less allowed: no less padding
    assert allowed_rows(ivf["ids"], ivf["ids"][:5], "allow").sum() == 5
