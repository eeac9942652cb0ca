"""The cross-rank merge (qk_merge_topk / qk_merge_topk_packed: k_merge_ranks<2|4|8|16> up to k = 960, k_merge_ranks_large beyond)
against the yardstick (tests/merge_yardstick.py: the union of the ranks' candidates sorted under (key, id), its first k) -- not
against each other.  Runs arrive as qk_search returns them: sorted under (key, id), the -1 padding a suffix.  Which kernel a k
launches follows from the pool of k + 64 entries rounded up to 64: <= 128 -> <2> (k <= 64), <= 256 -> <4> (k <= 192), <= 512 -> <8>
(k <= 448), <= 1024 -> <16> (k <= 960), beyond -> the sorted-run form."""
import numpy as np
import pytest

import merge_yardstick as Y

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# (k, [(G, Q)]): every k of the issue's list, every G of (1, 2, 3, 8, 16, 64), every Q of (1, 5, 67); G * Q * k stays under a million
GRID = ((1, [(1, 1), (64, 67), (3, 5)]), (63, [(2, 5), (16, 67)]), (64, [(3, 67), (8, 1)]), (65, [(8, 5), (64, 1)]),
        (192, [(16, 1), (2, 67)]), (193, [(64, 5), (3, 1)]), (448, [(1, 67), (8, 5)]), (449, [(2, 1), (16, 5)]),
        (960, [(3, 5), (16, 5), (1, 1)]), (961, [(8, 67), (64, 1), (2, 5)]), (2000, [(16, 5), (64, 5), (1, 1), (3, 67)]))
MODES = ("distinct", "ties", "equal", "special", "short")


def test_grid_is_covered():
    assert [k for k, _ in GRID] == [1, 63, 64, 65, 192, 193, 448, 449, 960, 961, 2000]
    assert {g for _, c in GRID for g, _ in c} == {1, 2, 3, 8, 16, 64} and {q for _, c in GRID for _, q in c} == {1, 5, 67}
    assert any((q * k) % 2 == 1 for k, c in GRID for _, q in c)          # an odd per * k: packed blocks are padded


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def make_runs(G, Q, k, metric, first_mode, rng):
    """[G, Q, k] ids / keys as the ranks send them; query q is of mode MODES[(q + first_mode) % 5]:
    distinct / ties (seven values across all ranks) / equal / special (infinities, signed zeros) with 0 .. k entries per rank;
    short: so few that the row stays short in total.  Where two ranks have entries, rank 1 also holds rank 0's first (key, id)."""
    ids = (rng.permutation(G * Q * k).astype(np.int64).reshape(G, Q, k) + 1) + np.where(rng.random((G, Q, k)) < 0.3, np.int64(1) << 34, 0)
    keys = np.empty((G, Q, k), np.float32)
    count = np.empty((G, Q), np.int64)
    for q in range(Q):
        mode = MODES[(q + first_mode) % len(MODES)]
        if mode == "ties":
            seven = np.float32([0.0, 0.125, 0.5, 0.75, 2.0, 2.5, 9.0]) * np.float32(-1 if metric == "ip" and q % 2 else 1)
            keys[:, q, :] = seven[rng.integers(0, 7, size=(G, k))]
        else:
            keys[:, q, :] = Y.draw_values(G * k, "distinct" if mode == "short" else mode, metric, rng).reshape(G, k)
        if mode == "short":
            count[:, q] = rng.integers(0, (k - 1) // G + 1, size=G)
        else:
            count[:, q] = np.where(rng.random(G) < 0.3, k, rng.integers(0, k + 1, size=G))
            count[rng.integers(0, G), q] = (0, k, k // 2)[q % 3]
        if G >= 2 and count[0, q] > 0 and count[1, q] > 0:
            ids[1, q, 0], keys[1, q, 0] = ids[0, q, 0], keys[0, q, 0]
    gone = np.arange(k)[None, None, :] >= count[:, :, None]
    ids[gone] = -1
    keys[gone] = Y.pad_dist(metric)
    return Y.sorted_runs(ids, keys, metric)


def merged_both_ways(ctx, ids, keys, metric):
    """(ids, distance bits) of qk_merge_topk on [G][Q][k] and of qk_merge_topk_packed on the G packed blocks"""
    from quake_amd.sharded import pack_topk_host, topk_block_bytes
    G, Q, k = ids.shape
    mi, md = ctx.merge_topk(torch.from_numpy(ids).cuda(), torch.from_numpy(keys).cuda(), metric)
    recv = torch.empty((G, topk_block_bytes(Q, k)), dtype=torch.uint8)
    for g in range(G):
        recv[g] = pack_topk_host(torch.from_numpy(ids[g]), torch.from_numpy(keys[g]), 1)[0]
    pi, pd = ctx.merge_topk_packed(recv.cuda(), Q, k, metric)
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), b.cpu().numpy().view(np.uint32)) for a, b in ((mi, md), (pi, pd))]


def assert_equals_yardstick(ctx, ids, keys, metric, tag):
    ri, rd = Y.merge_ranks_reference(ids, keys, metric, sqrt_l2=True)
    for which, (gi, gd) in zip(("qk_merge_topk", "qk_merge_topk_packed"), merged_both_ways(ctx, ids, keys, metric)):
        np.testing.assert_array_equal(gi, ri, err_msg="ids, %s, %s" % (which, tag))
        np.testing.assert_array_equal(gd, rd.view(np.uint32), err_msg="distance bits, %s, %s" % (which, tag))
    return ri


@pytest.mark.parametrize("k,shapes", GRID, ids=[str(k) for k, _ in GRID])
def test_merged_runs_equal_the_yardstick(ctx, k, shapes):
    for G, Q in shapes:
        rng = np.random.default_rng(k * 1000 + G * 10 + Q)
        for b in range(5 if G * Q * k <= 300000 else 2):      # every mode meets query 0; the large shapes take two rotations
            metric = ("l2", "ip")[b % 2]
            ids, keys = make_runs(G, Q, k, metric, b, rng)
            assert_equals_yardstick(ctx, ids, keys, metric, "k=%d G=%d Q=%d %s rotation %d" % (k, G, Q, metric, b))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("k", [64, 960, 961, 2000])
def test_nan_key_with_a_valid_id_is_no_candidate(ctx, k, metric):
    """A NaN key behind a run's candidates, with a valid id -- in a run that has padding behind it and in a run it makes full -- is
    returned by neither form (a NaN key is no candidate).  Before the sorted-run form counted a rank's candidates up
    to the first id < 0 OR NaN key, k = 961 and k = 2000 returned the entry with a NaN distance while k <= 960 dropped it."""
    G, Q = 3, 5
    rng = np.random.default_rng(k + 17)
    ids = rng.permutation(G * Q * k).astype(np.int64).reshape(G, Q, k) + 1
    keys = Y.draw_values(G * Q * k, "distinct", metric, rng).reshape(G, Q, k)
    count = rng.integers(0, k, size=(G, Q))
    count[0, 0], count[1, 1], count[2, 2], count[0, 3] = k - 1, k - 1, 0, k // 3       # (the NaN makes ranks (0, 0) and (1, 1) full)
    count[:, 4] = k // 8                                     # a row short in total: nothing else keeps a NaN entry out of the first k
    gone = np.arange(k)[None, None, :] >= count[:, :, None]
    ids[gone], keys[gone] = -1, Y.pad_dist(metric)
    nan_ids = []
    for g in range(G):
        for q in range(Q):
            if (g + q) % 2 == 0:                             # in about half of the runs: a NaN of either sign behind the candidates
                ids[g, q, count[g, q]] = 10 ** 12 + g * Q + q
                keys.view(np.uint32)[g, q, count[g, q]] = (0x7FC00000, 0xFFC00001)[(g + q) % 4 == 0]
                nan_ids.append(10 ** 12 + g * Q + q)
    ids, keys = Y.sorted_runs(ids, keys, metric)
    for g in range(G):                                       # (the precondition: candidates, then the NaN, then the padding)
        for q in range(Q):
            c = count[g, q]
            assert (ids[g, q, :c] > 0).all() and not np.isnan(keys[g, q, :c]).any() and (ids[g, q, c + ((g + q) % 2 == 0):] == -1).all()
    got = merged_both_ways(ctx, ids, keys, metric)
    for gi, gd in got:
        print("k=%d %s: %d of %d NaN-keyed ids returned, %d NaN distances" % (k, metric, int(np.isin(gi, nan_ids).sum()), len(nan_ids),
                                                                                int(np.isnan(gd.view(np.float32)).sum())))
    for gi, gd in got:
        assert not np.isin(gi, nan_ids).any() and not np.isnan(gd.view(np.float32)).any()
    assert_equals_yardstick(ctx, ids, keys, metric, "NaN keys, k=%d %s" % (k, metric))
