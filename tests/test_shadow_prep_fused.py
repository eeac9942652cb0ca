"""The fp16 query copy and the error bound E of the shadow form come from the seed waves of k_group_seed where the
grouping runs as that kernel (at most 4096 pairs, k <= 64), and from the k_shadow_prep launch on every other grouping path: one
device function, the same bits.  A wrong copy or bound shows as different answers, as queries that fall back although the rule's host
model passes for them, or as out-of-range queries that are not flagged.

Forced shadow search against mode 0 and the oracle: d = 16, 48, 128 and 256 (the largest the form accepts), Q = 1, 15, 17 and 1100
(a seed workgroup carries 16 waves), L2 and IP; a batch of 4100 queries (more pairs than the small grouping takes: the separate
launch); k = 65 (k_group_seed is not taken, and the form does not accept the call: the tile form answers)."""
import functools

import numpy as np
import pytest

import oracle as O
from test_shadow_scan import SHADOW, TILE, check, corpus, model_passes, queries, same_bits, stores

pytestmark = pytest.mark.gpu

K = 10
SMALL_PAIRS = 4096  # QK_GROUP_SMALL (qk_scan.hip)


def batch(ivf, Q, seed):
    if Q > 1100:  # (copies of one batch of 1100: the host model is asked about 1100 queries, not Q)
        return np.ascontiguousarray(np.concatenate([batch(ivf, 1100, seed)] * ((Q + 1099) // 1100), 0)[:Q])
    if Q < 12:
        per = [0] * 10 + [Q, 0]
    else:
        per = [Q // 16] * 10 + [Q // 8, 0]
        per[11] = Q - sum(per)
    q = queries(ivf, per, seed=seed)
    assert q.shape[0] == Q
    return q


@functools.lru_cache(maxsize=None)
def inputs(d):
    return corpus(d, seed=200 + d)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [16, 48, 128, 256])
def test_fused_prep_answers_with_the_bits_of_mode_0_and_the_oracle(d, metric):
    from quake_amd.capi import Context
    ivf = inputs(d)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    for Q in (1, 15, 17, 1100):
        q = batch(ivf, Q, seed=11 * d + Q)
        if metric == "l2":
            assert model_passes(ivf, q, K, metric).all(), "the fixed inputs must pass the rule's model on the host"
        st = check(ctx, parent, s, ivf, q, K, metric)
        if metric == "l2":  # a bound that is too large or negative would show here: the exact scan answers, with the same bits
            assert st["fallback"] == 0 and st["verified"] == Q, (Q, st)
        else:
            assert st["verified"] + st["fallback"] == Q, (Q, st)
    s.close(); parent.close(); ctx.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_a_batch_beyond_the_small_grouping_keeps_the_separate_launch(metric):
    from quake_amd.capi import Context
    ivf = inputs(48)
    Q = SMALL_PAIRS + 4
    q = batch(ivf, Q, seed=77)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    small = check(ctx, parent, s, ivf, q[:1100], K, metric)       # through k_group_seed
    large = check(ctx, parent, s, ivf, q, K, metric)              # through the three-kernel grouping
    again = check(ctx, parent, s, ivf, q[:1100], K, metric, oracle=False)
    assert large["verified"] + large["fallback"] == Q and small["verified"] + small["fallback"] == 1100
    assert (again["verified"], again["fallback"]) == (small["verified"], small["fallback"])
    s.close(); parent.close(); ctx.close()


def test_k_65_is_not_a_shadow_call():
    from quake_amd.capi import Context
    ivf = inputs(48)
    q = batch(ivf, 40, seed=78)
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    ctx.set_shadow(2)
    before = ctx.shadow_stats()
    got = ctx.search(parent, s, q, 1, 65, "l2")
    assert ctx.last_scan_kernel() in TILE and ctx.shadow_stats() == before
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, 65, "l2", batched_scan=True)
    same_bits(got, (oi, od), "k = 65")
    got = ctx.search(parent, s, q, 1, K, "l2")  # the same context and store, a shadow call again
    assert ctx.last_scan_kernel() == SHADOW
    oi, od = O.search(q, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, K, "l2", batched_scan=True)
    same_bits(got, (oi, od), "k = 10 behind k = 65")
    s.close(); parent.close(); ctx.close()


@pytest.mark.parametrize("Q", [40, SMALL_PAIRS + 4])
def test_queries_outside_the_fp16_range_are_flagged_on_both_paths(Q):
    """+-Inf, a finite value beyond 65504 and a huge one: E < 0, the exact scan of the list answers -- fallback == their number,
    whichever kernel wrote E (Q = 40: the seed waves; Q = 4100: the separate launch)"""
    from quake_amd.capi import Context
    ivf = inputs(48)
    q = batch(ivf, Q, seed=79 + Q)
    assert model_passes(ivf, q[:1100], K, "l2").all(), "the fixed inputs must pass the rule's model on the host"
    bad = np.array([3, 11, 19, Q - 1])
    q[3, 0] = np.inf
    q[11, 40] = -np.inf
    q[19, 1] = 7.0e4
    q[Q - 1, 47] = -1.0e30
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    st = check(ctx, parent, s, ivf, q, K, "l2", oracle=False)
    assert st["fallback"] == len(bad) and st["verified"] == Q - len(bad), st
    s.close(); parent.close(); ctx.close()
