"""Quantized search without a device: the yardstick (tests/sq8_yardstick.py) against the oracle's search where fetch_k covers the probed
rows, the number formats it relies on, and lower_sq8's checks in both mirrors (quake_amd/where.py; quake_amd/cpp, by the bindings)."""
import numpy as np
import pytest

import oracle as O
import sq8_yardstick as SY


def test_numpy_reproduces_the_code_rule():
    F = np.float32
    assert (np.rint(np.array([0.5, 1.5, 2.5, -0.5, -2.5, 3.5], F)) == np.array([0, 2, 2, -0, -2, 4], F)).all()   # half to even
    assert (F(1) / F(3)).dtype == F and F(1) / F(3) == F(np.float64(1) / 3)                                        # IEEE float32 division
    m, s = SY.params(np.array([[-3.96875, 0.0], [3.96875, 1.0]], F), "l2")
    assert s == F(0.03125) and (m == np.array([0, 0.5], F)).all()
    x = np.array([[2.5 / 32, 0.5], [3.5 / 32, 9.0], [np.nan, -np.inf]], F)
    assert (SY.codes(x, m, s) == [[2, 0], [4, 127], [0, -127]]).all()
    assert (SY.query_codes(np.array([[np.inf, 2.0, np.nan, -0.5]], F), None, None, "ip") == [[127, 127, 0, -32]]).all()   # its own scale: 2 / 127
    assert SY.params(np.zeros((3, 2), F), "ip")[1] == 1 and SY.params(np.zeros((0, 2), F), "l2")[1] == 1


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_covering_fetch_k_is_the_oracles_search(metric):
    rng = np.random.default_rng(3)
    sizes, d, nprobe, k = [0, 1, 15, 16, 17, 33, 120, 57], 40, 3, 10
    cent = rng.standard_normal((len(sizes), d)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    vecs = (cent[np.repeat(np.arange(len(sizes)), sizes)] + 0.3 * rng.standard_normal((offsets[-1], d))).astype(np.float32)
    ids = rng.permutation(offsets[-1]).astype(np.int64) + 7
    q = (cent[rng.integers(0, len(sizes), 9)] + 0.3 * rng.standard_normal((9, d))).astype(np.float32)
    pids = O.coarse(q, cent, None, nprobe, metric)[0]
    gi, gd = SY.case(q, vecs, ids, offsets, pids, k, int(offsets[-1]), metric)
    oi, od = O.search(q, cent, vecs, ids, offsets, nprobe, k, metric, batched_scan=True)
    assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()


CASES = [((40, 0, 64), "k=0 must be at least 1"), ((40, 10, 9), "fetch_k=9 must be at least k=10"),
         ((128, 10, 449), "fetch_k=449 must not exceed 448"), ((2112, 10, 64), "d=2112 must not exceed 2048"),
         # several faults: k first, then fetch_k, and the limits last
         ((4096, 0, 500), "k=0 must be"), ((4096, 5, 4), "fetch_k=4 must be at least k=5"), ((4096, 5, 449), "fetch_k=449 must not exceed")]


def test_lower_sq8_and_the_mirrors():
    import torch

    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd as quake
    import quake_amd.bindings as qb
    from quake_amd.where import lower_sq8
    lowers = (lower_sq8, qb.lower_sq8)
    for lower in lowers:
        assert tuple(lower(2048, 448, 448)) == (448, 448) and tuple(lower(d=40, k=1, fetch_k=1)) == (1, 1)
    for args, text in CASES:
        msgs = []
        for lower in lowers:
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] and text in msgs[0] and msgs[0].startswith("[QuakeIndex::quantized_search()]"), msgs
    with pytest.raises(RuntimeError, match="integers"):
        lower_sq8(48, 2.5, 64)
    for mod in (quake, qb):
        idx, sp = mod.QuakeIndex(), mod.SearchParams()
        sp.k = 5
        with pytest.raises(RuntimeError, match=r"\[QuakeIndex::quantized_search\(\)\] No query coordinator. Did you build the index\?"):
            idx.quantized_search(torch.zeros(2, 32), sp, fetch_k=20)
    from quake_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::quantized_search\(\)\] quantized_search is not supported by sharded.py"):
        ShardedIndex(None).quantized_search(torch.zeros(2, 32), 4, 5, 20)
