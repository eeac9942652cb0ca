"""The finish counters of the fp16 shadow form (qk_ctx_shadow_stats; quake_amd/csrc/qk_shadow.hip) are striped: 64
lines of four counters, the finish wave of query q adds to line q % 64, the host sums the lines.  The totals stay exact.

Q = 1, 63, 64, 65 and 1100 leave stripes unused, use each once, and share them.  Through qk_debug_shadow_finish the records are laid
out here (as tests/test_shadow_finish.py does): queries that verify, queries without a bound or without a record (the fallback) and
queries whose records are chained, so that all four totals move, and every total equals the numpy model's
(tests/shadow_finish_yardstick.py) exactly.  Through a forced search the records are the scan's own: verified and fallback are
known exactly (the inputs pass the rule's host model; queries beyond the fp16 range cannot have a bound), every verified query
re-scores at least k candidates."""
import functools

import numpy as np
import pytest

import oracle as O
import shadow_finish_yardstick as Y
from test_shadow_finish import E0, add_records, corpus, near_queries
from test_shadow_scan import SHADOW, check, model_passes, queries, stores
from test_shadow_scan import corpus as scan_corpus

pytestmark = pytest.mark.gpu

STRIPES = 64
QS = [1, STRIPES - 1, STRIPES, STRIPES + 1, 1100]
D, K, METRIC = 20, 10, "l2"
KEYS = ("verified", "fallback", "candidates", "chained")


@functools.lru_cache(maxsize=None)
def case(Q):
    """inputs of one hook call and the model's totals.  Query q follows pattern (q + 2) % 5: two records that verify; no bound
    (E < 0); 33 records, two of them chained; no record at all; one short record"""
    ivf = corpus(D)
    rng = np.random.default_rng(500 + Q)
    x = near_queries(ivf, Q, rng)
    E = np.full(Q, E0)
    layouts = []
    for q in range(Q):
        pat = (q + 2) % 5
        if pat == 1:
            E[q] = -1.0
        layouts.append({0: [(32, 3), (20, 2)], 1: [(32, 3)], 2: [(3, 1)] * 33, 3: [], 4: [(5, 5)]}[pat])
    recs = Y.Records(Q, max(1, sum(len(lay) for lay in layouts)))
    for q, lay in enumerate(layouts):
        add_records(recs, q, rng, lay, METRIC)
    lists = np.zeros(Q, np.int64)
    m = Y.model(x, E, lists, recs, ivf["offsets"], ivf["vecs"], ivf["ids"], K, METRIC)
    want = {key: int(m[key].sum()) for key in KEYS}
    return x, E, lists, recs, want


def env():
    from quake_amd.capi import Context, Store
    ivf = corpus(D)
    ctx = Context(0)
    s = Store(ctx, D)
    s.build_csr(ivf["offsets"], ivf["ids"], ivf["vecs"])
    return ctx, s


def finish(ctx, s, Q):
    """one hook call: (what the call reports it added, the change of the context's totals, the model's totals)"""
    x, E, lists, recs, want = case(Q)
    before = ctx.shadow_stats()
    got = ctx.shadow_finish(s, x, E, lists, k=K, metric=METRIC, **recs.arrays())
    after = ctx.shadow_stats()
    return {key: got[key] for key in KEYS}, {key: after[key] - before[key] for key in KEYS}, want


@pytest.mark.parametrize("Q", QS)
def test_hook_totals_equal_the_model(Q):
    ctx, s = env()
    assert ctx.shadow_stats() == dict.fromkeys(KEYS, 0)
    reported, delta, want = finish(ctx, s, Q)
    if Q >= 5:  # (every pattern occurs: every total moves)
        assert want["verified"] > 0 and want["fallback"] >= 2 * (Q // 5) and want["chained"] >= Q // 5 and want["candidates"] > want["verified"]
    else:
        assert want["chained"] == 1 and want["verified"] == 1
    assert reported == want
    assert delta == want
    s.close(); ctx.close()


def test_totals_accumulate_over_calls_and_a_refused_call_changes_nothing():
    from quake_amd._lib import QuakeHipError
    ctx, s = env()
    total = dict.fromkeys(KEYS, 0)
    for Q in (STRIPES + 1, STRIPES + 1, STRIPES + 1, 1, 1100):
        reported, delta, want = finish(ctx, s, Q)
        assert reported == want and delta == want
        total = {key: total[key] + want[key] for key in KEYS}
        assert ctx.shadow_stats() == total
    x, E, lists, recs, _ = case(STRIPES)
    with pytest.raises(QuakeHipError):
        ctx.shadow_finish(s, x, E, lists, k=17, metric=METRIC, **recs.arrays())
    bad = Y.Records(STRIPES, 4)
    bad.pair_slots[3, 0], bad.pair_slots[3, 1] = 1, 9  # a record number outside [-1, max_recs)
    with pytest.raises(QuakeHipError):
        ctx.shadow_finish(s, x, E, lists, k=K, metric=METRIC, **bad.arrays())
    assert ctx.shadow_stats() == total
    s.close(); ctx.close()


def test_two_contexts_on_one_store_keep_separate_totals():
    from quake_amd.capi import Context
    a, s = env()
    b = Context(0)
    _, da, wa = finish(a, s, STRIPES + 1)
    assert b.shadow_stats() == dict.fromkeys(KEYS, 0)
    _, db, wb = finish(b, s, 1100)
    assert da == wa and db == wb and wa != wb
    assert a.shadow_stats() == wa and b.shadow_stats() == wb
    _, da2, _ = finish(a, s, STRIPES - 1)
    assert a.shadow_stats() == {key: wa[key] + da2[key] for key in KEYS} and b.shadow_stats() == wb
    b.close()
    s.close(); a.close()


@functools.lru_cache(maxsize=None)
def search_inputs():
    return scan_corpus(48, seed=148)


@pytest.mark.parametrize("Q", QS)
def test_forced_search_totals(Q):
    """the scan's own records: every query within the fp16 range verifies (the host model passes), every 7th query of a batch has a
    component beyond the range -- no bound, answered by the exact scan of its list; totals accumulate over three calls"""
    from quake_amd.capi import Context
    ivf = search_inputs()
    if Q == 1:
        per = [0] * 10 + [1, 0]
    else:
        per = [Q // 16] * 10 + [Q // 8, 0]
        per[11] = Q - sum(per)
    q = queries(ivf, per, seed=300 + Q)
    assert q.shape[0] == Q
    assert model_passes(ivf, q, K, "l2").all(), "the fixed inputs must pass the rule's model on the host"
    bad = np.arange(3, Q, 7)
    q[bad, 5] = 7.0e4  # finite, beyond the fp16 range (whichever list such a query probes: every list has rows)
    good = np.setdiff1d(np.arange(Q), bad)
    pid, _ = O.coarse(q[good], ivf["centroids"], None, 1, "l2")
    sizes = np.diff(ivf["offsets"])[pid[:, 0]]
    ctx = Context(0)
    parent, s = stores(ctx, ivf)
    total = dict.fromkeys(KEYS, 0)
    for call in range(3):
        # (the oracle on the first call of a batch within the range; mode 0 is the reference for the others)
        st = check(ctx, parent, s, ivf, q, K, "l2", label=SHADOW, oracle=call == 0 and len(bad) == 0)
        assert st["verified"] == Q - len(bad) and st["fallback"] == len(bad), st
        # a verified query re-scores at least the k best entries (all of a list shorter than k), at most the rows of its list
        assert int(np.minimum(sizes, K).sum()) <= st["candidates"] <= int(sizes.sum()), st
        total = {key: total[key] + st[key] for key in KEYS}
        assert ctx.shadow_stats() == total
    s.close(); parent.close(); ctx.close()
