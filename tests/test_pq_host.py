"""Product-quantized search without a device: lower_pq and lower_pq_codebooks in both mirrors (quake_amd/where.py; quake_amd/cpp,
by the bindings), the sharded refusal, and the yardstick's own invariants."""
import numpy as np
import pytest

import pq_yardstick as PY

BAD = [((40, 0, 64), "k=0 must be at least 1"), ((40, 10, 9), "fetch_k=9 must be at least k=10"), ((128, 449, 4096), "k=449 must not exceed 448"),
       ((128, 10, 4097), "fetch_k=4097 must not exceed 4096"), ((8193, 10, 4096), "d=8193 must not exceed 8192"),
       # several faults: k's limit before fetch_k's, d last
       ((9000, 449, 5000), "k=449 must not exceed 448"), ((9000, 5, 4097), "fetch_k=4097 must not exceed 4096")]
BAD_M = [((128, 0), "num_codebooks=0 must be at least 1"), ((1290, 129), "num_codebooks=129 must not exceed 128"),
         ((130, 4), "num_codebooks=4 must divide d=130"), ((130, 2), "d / num_codebooks = 65 must not exceed 64"),
         # several faults: the limit of M before divisibility, divisibility before dsub
         ((1000, 129), "num_codebooks=129 must not exceed 128"), ((8191, 2), "num_codebooks=2 must divide d=8191")]


def _mirrors(name):
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as qb
    import quake_amd.where as W
    return getattr(W, name), getattr(qb, name)


@pytest.mark.parametrize("name,good,bad,who", [("lower_pq", [((8192, 448, 4096), (448, 4096)), ((1, 1, 1), (1, 1))], BAD, "pq_search"),
                                               ("lower_pq_codebooks", [((8192, 128), 128), ((1, 1), 1), ((130, 65), 65)], BAD_M, "train_pq")])
def test_lowering_and_the_mirrors(name, good, bad, who):
    for lower in _mirrors(name):
        for args, out in good:
            got = lower(*args)
            assert (tuple(got) if isinstance(out, tuple) else got) == out
    for args, text in bad:
        msgs = []
        for lower in _mirrors(name):
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] == "[QuakeIndex::%s()] %s" % (who, text), msgs


def test_sharded_refuses_by_name():
    import torch

    from quake_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::pq_search\(\)\] pq_search is not supported by sharded.py"):
        ShardedIndex(None).pq_search(torch.zeros(2, 32), 4, 5, 2000)


@pytest.mark.parametrize("d,M,metric", [(128, 128, "l2"), (256, 128, "ip")])
def test_yardstick_invariants(d, M, metric):
    """the sum of the rows' largest entries stays under 8192 at M = 128 (table() asserts it), and the key is an exact integer: the same
    in every order of summation"""
    rng = np.random.default_rng(d)
    x = rng.standard_normal((300, d)).astype(np.float32)
    cb = np.ascontiguousarray(x[:256].reshape(256, M, d // M).transpose(1, 0, 2))
    u = PY.table(x[256:264] * np.float32(3), cb, metric)
    assert u.dtype == np.uint16 and (u.max(2).astype(np.int64).sum(1) < PY.BINS).all() and (u.min(2) == 0).all()
    cx = PY.codes(x, cb)
    h = PY.keys(u[0], cx)
    perm = rng.permutation(M)
    assert (h == PY.keys(u[0][perm], cx[:, perm])).all() and (h == sum(u[0][m][cx[:, m]].astype(np.int64) for m in reversed(range(M)))).all()
