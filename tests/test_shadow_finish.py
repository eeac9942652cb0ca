"""k_shadow_finish, the exact finish of the fp16 shadow form (quake_amd/csrc/qk_shadow.hip), on records a test lays
out, through qk_debug_shadow_finish: ids, distance bits and the four counters must equal the numpy model of the rule
(tests/shadow_finish_yardstick.py, pinned against the oracle in tests/test_shadow_finish_oracle.py) bit for bit.

Behind a scan the finish meets two or three records per query; here a test decides: 0 to 70 records (the slot line holds 31, more
are chained; eight are read per round), 0 to 32 entries per record, fewer than k to 300 candidates (64 are re-scored per round, the
k survivors carried), ties on the exact key across records and rounds, queries that cannot verify.  The approximate keys are
invented: candidates are arbitrary rows of the list, not its nearest ones, so the answer follows the rule and not the truth -- a
kernel that answered from the list itself would not match.  Every case has Q <= 64 over a store of about 3000 rows."""
import functools

import numpy as np
import pytest

import shadow_finish_yardstick as Y

pytestmark = pytest.mark.gpu

ID_BASE = 1 << 41
SIZES = [2600, 300, 0, 40]  # list 2 is empty
NDUP = 24                   # the first rows of list 0 are copies of one vector: ties on the exact key, decided by ids above 2^40
E0 = np.float32(0.25)
NEAR, FAR = (1.0, 1.4), (1.0e6, 2.0e6)  # "badness" of invented keys: candidates lie within 2 E0 of each other, the rest far behind


@functools.lru_cache(maxsize=None)
def corpus(d):
    rng = np.random.default_rng(1000 + d)
    cent = rng.standard_normal((len(SIZES), d)).astype(np.float32)
    parts = [(cent[p] + 0.3 * rng.standard_normal((n, d))).astype(np.float32) for p, n in enumerate(SIZES)]
    parts[0][:NDUP] = 1.5 * parts[0][0]  # (longer than its neighbours: the nearest of a query next to it under IP too)
    ids = rng.permutation(sum(SIZES)).astype(np.int64) + ID_BASE
    offsets = np.zeros(len(SIZES) + 1, np.int64)
    offsets[1:] = np.cumsum(SIZES)
    return dict(vecs=np.ascontiguousarray(np.concatenate(parts, 0)), ids=ids, offsets=offsets, centroids=cent, d=d)


_ENV = {}


def env(d):
    """one context, and one store per dimension, for the module"""
    from quake_amd.capi import Context, Store
    if "ctx" not in _ENV:
        _ENV["ctx"] = Context(0)
    if d not in _ENV:
        ivf = corpus(d)
        s = Store(_ENV["ctx"], d)
        s.build_csr(ivf["offsets"], ivf["ids"], ivf["vecs"])
        _ENV[d] = s
    return _ENV["ctx"], _ENV[d], corpus(d)


def keys_of_badness(b, metric):
    b = np.asarray(b, np.float32)
    return Y.key_of(b if metric == "l2" else -b, metric)


def add_records(recs, q, rng, layout, metric, p=0, size=SIZES[0], positions=None, near=NEAR):
    """layout: (entries, candidates) per record.  A record's candidates get near keys, its other entries far ones; rows are distinct
    positions of list p (positions: the candidates' rows, in order, instead of random ones)"""
    perm = rng.permutation(np.arange(NDUP, size))  # (the copies are placed on purpose only)
    used, cpos = 0, 0
    for n, c in layout:
        b = np.concatenate([np.sort(rng.uniform(*near, c)), np.sort(rng.uniform(*FAR, n - c))])
        pos = perm[used:used + n].copy()
        used += n
        if positions is not None:
            pos[:c] = positions[cpos:cpos + c]
            cpos += c
        recs.add(q, keys_of_badness(b, metric), np.full(n, p), pos)


def run_and_compare(d, metric, k, sqrt_l2, x, E, lists, recs):
    ctx, s, ivf = env(d)
    m = Y.model(x, E, lists, recs, ivf["offsets"], ivf["vecs"], ivf["ids"], k, metric, sqrt_l2=sqrt_l2)
    got = ctx.shadow_finish(s, x, E, lists, k=k, metric=metric, sqrt_l2=sqrt_l2, **recs.arrays())
    bad = [q for q in range(x.shape[0]) if not ((got["ids"][q] == m["ids"][q]).all() and
                                                 (got["dist"][q].view(np.uint32) == m["dist"][q].view(np.uint32)).all())]
    assert not bad, "queries %s differ from the model; first: ids %s / %s, dist %s / %s" % (
        bad, got["ids"][bad[0]], m["ids"][bad[0]], got["dist"][bad[0]], m["dist"][bad[0]])
    assert got["verified"] == int(m["verified"].sum())
    assert got["fallback"] == int(m["fallback"].sum())
    assert got["candidates"] == int(m["candidates"].sum())
    assert got["chained"] == int(m["chained"].sum())
    return m


def near_queries(ivf, Q, rng, p=0):
    return (ivf["centroids"][p] + 0.1 * rng.standard_normal((Q, ivf["d"]))).astype(np.float32)


SHAPES = [(8, "l2", 1, True), (20, "ip", 10, True), (128, "l2", 10, True), (128, "l2", 16, False), (136, "l2", 16, False), (256, "ip", 16, True),
          (256, "l2", 10, True)]


@pytest.mark.parametrize("d,metric,k,sqrt_l2", SHAPES)
def test_records_per_query_and_entries_per_record(d, metric, k, sqrt_l2):
    """0 .. 70 records (one round, several rounds, the full slot line, chained) x 1, k - 1, k, 31, 32 entries per record"""
    rng = np.random.default_rng(d + k)
    nrec = [0, 1, 2, 3, 8, 9, 16, 17, 31, 32, 33, 70]
    nent = [1, k - 1, k, 31, 32]
    Q = len(nrec) * len(nent)
    ivf = corpus(d)
    x = near_queries(ivf, Q, rng)
    recs = Y.Records(Q, sum(nrec) * len(nent))
    for i, R in enumerate(nrec):
        for j, n in enumerate(nent):
            add_records(recs, i * len(nent) + j, rng, [(n, int(rng.integers(0, min(n, 3) + 1))) for _ in range(R)], metric)
    m = run_and_compare(d, metric, k, sqrt_l2, x, np.full(Q, E0), np.zeros(Q, np.int64), recs)
    assert m["verified"].sum() >= Q // 2 and m["fallback"][:len(nent)].all()  # (no record: the list is scanned)
    assert m["chained"].sum() == 3 * len(nent)


@pytest.mark.parametrize("d,metric,k", [(128, "l2", 10), (20, "ip", 16), (256, "l2", 1), (136, "ip", 10)])
def test_candidates_per_query(d, metric, k):
    """fewer than k, k, 63, 64, 65, 129, 300 candidates: one per record, 30 per record, all in one record"""
    rng = np.random.default_rng(7 * d + k)
    cases = []
    for C in (k, 63, 64, 65, 129, 300):
        cases.append((C, [(int(rng.integers(1, 5)), 1) for _ in range(C)]))                      # one per record
        cases.append((C, [(32, 30)] * (C // 30) + ([(32, C % 30)] if C % 30 else [])))           # packed, full records
    cases.append((min(k, 31), [(31, min(k, 31))] + [(5, 0)] * 4))                                # all in one record
    cases.append((31, [(3, 0), (31, 31), (32, 0)]))
    if k > 1:
        cases.append((k - 1, [(k - 1, 0)]))       # fewer than k entries: no a_k, every entry is a candidate
        cases.append((k - 1, [(1, 0)] * (k - 1)))
    Q = len(cases)
    ivf = corpus(d)
    x = near_queries(ivf, Q, rng)
    recs = Y.Records(Q, sum(len(lay) for _, lay in cases))
    for q, (_, lay) in enumerate(cases):
        add_records(recs, q, rng, lay, metric)
    m = run_and_compare(d, metric, k, True, x, np.full(Q, E0), np.zeros(Q, np.int64), recs)
    assert list(m["candidates"]) == [C for C, _ in cases]
    assert m["verified"].all()


@pytest.mark.parametrize("metric,k", [("l2", 10), ("ip", 16), ("l2", 1)])
def test_ties_across_records_and_rounds(metric, k):
    """24 copies of one row, ids above 2^40: one per record over 70 records and three rounds of 64 candidates; all in two records"""
    d = 128
    rng = np.random.default_rng(k)
    ivf = corpus(d)
    x = (ivf["vecs"][0] + 0.01 * rng.standard_normal((2, d))).astype(np.float32)
    recs = Y.Records(2, 72)
    dup = rng.permutation(NDUP)
    pos = np.zeros(140, np.int64)
    others = iter(rng.permutation(np.arange(NDUP, SIZES[0]))[:140])
    for r in range(70):  # two candidates per record: records 0, 3, 6 .. 69 hold a copy
        pos[2 * r] = dup[r // 3] if r % 3 == 0 else next(others)
        pos[2 * r + 1] = next(others)
    add_records(recs, 0, rng, [(4, 2)] * 70, metric, positions=pos)
    add_records(recs, 1, rng, [(20, 12), (12, 12)], metric, positions=dup)
    m = run_and_compare(d, metric, k, True, x, np.full(2, E0), np.zeros(2, np.int64), recs)
    want = np.sort(ivf["ids"][:NDUP])[:k]  # the tie straddles the k-th place: the smallest ids win
    for q in range(2):
        assert (m["ids"][q] == want).all() and len(set(m["dist"][q].view(np.uint32))) == 1
    assert m["verified"].all() and m["chained"][0] and list(m["candidates"]) == [140, 24]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_queries_that_cannot_verify_fall_back(metric):
    """verification failing by one key step, E < 0, NaN, no record, a probed list that is empty, no list"""
    d, k = 128, 10
    near = NEAR if metric == "l2" else (-1000.0, -999.6)  # (invented keys in front of every exact one: the edge key is no candidate)
    rng = np.random.default_rng(3)
    ivf = corpus(d)
    Q = 8
    x = near_queries(ivf, Q, rng)
    E = np.full(Q, E0)
    lists = np.zeros(Q, np.int64)
    recs = Y.Records(Q, 4 * Q)
    seeds = rng.integers(1 << 30)
    for q in range(Q):
        add_records(recs, q, np.random.default_rng(seeds), [(32, 30), (32, 30)], metric, near=near)  # the same records for every query
    x[1] = x[0]
    E[2], E[3] = -1.0, np.nan
    recs.pair_slots[4, 0] = 0
    lists[5], recs.pair_slots[5, 0] = 2, 0   # nothing to fall back to: an empty answer
    lists[6] = 2                             # records of list 0 that verify: the probed list is not looked at
    lists[7], recs.pair_slots[7, 0] = -1, 0
    m = Y.model(x, E, lists, recs, ivf["offsets"], ivf["vecs"], ivf["ids"], k, metric)
    assert m["verified"][0] and m["tau"][0] != Y.NONE
    edge = Y.widen(m["tau"][0], E0, metric)
    r0, r1 = recs.of_query(0)[0], recs.of_query(1)[0]
    recs.rec_ord[r0, 30:] = edge                        # fullmin == widen(tau, E): not greater, not verified
    recs.rec_ord[r1, 30:] = edge, edge + np.uint32(1)   # one key step more: verified
    m = run_and_compare(d, metric, k, True, x, E, lists, recs)
    assert m["fullmin"][0] == edge and m["fullmin"][1] == edge + np.uint32(1) and m["tau"][0] == m["tau"][1]
    assert list(m["verified"]) == [False, True, False, False, False, False, True, False]
    assert list(m["fallback"]) == [True, False, True, True, True, False, False, False]
    assert (m["ids"][5] == -1).all() and (m["ids"][7] == -1).all()


def test_the_answer_follows_the_rule_not_the_truth():
    """approximate keys far from the exact ones: the candidates are the list's farthest rows"""
    d, k, metric = 128, 10, "l2"
    rng = np.random.default_rng(9)
    ivf = corpus(d)
    x = near_queries(ivf, 4, rng)
    recs = Y.Records(4, 8)
    import oracle as O
    for q in range(4):
        ev = O.pair_values(x[q:q + 1], ivf["vecs"][:SIZES[0]], metric)[0]
        far = np.argsort(ev)[-40:]
        add_records(recs, q, rng, [(32, 20), (32, 20)], metric, positions=far)
    m = run_and_compare(d, metric, k, True, x, np.full(4, E0), np.zeros(4, np.int64), recs)
    truth, _ = O.search(x, ivf["centroids"], ivf["vecs"], ivf["ids"], ivf["offsets"], 1, k, metric, batched_scan=True)
    assert m["verified"].all() and not np.isin(m["ids"], truth).any()


def test_the_hook_refuses_malformed_records():
    from quake_amd._lib import QuakeHipError
    d, k, metric = 20, 10, "l2"
    ctx, s, ivf = env(d)
    rng = np.random.default_rng(1)
    x = near_queries(ivf, 2, rng)
    E, lists = np.full(2, E0), np.zeros(2, np.int64)

    def fresh():
        recs = Y.Records(2, 40)
        add_records(recs, 0, np.random.default_rng(2), [(32, 12)] * 33, metric)
        add_records(recs, 1, np.random.default_rng(3), [(5, 5)], metric)
        return recs

    before = ctx.shadow_stats()
    ctx.shadow_finish(s, x, E, lists, k=k, metric=metric, **fresh().arrays())
    after = ctx.shadow_stats()
    assert after["verified"] - before["verified"] == 2 and after["chained"] - before["chained"] == 1

    def refused(change, k=k, lists=lists):
        recs = fresh()
        change(recs)
        with pytest.raises(QuakeHipError):
            ctx.shadow_finish(s, x, E, lists, k=k, metric=metric, **recs.arrays())

    refused(lambda r: r.ent_list.__setitem__((0, 0), len(SIZES)))          # a list out of range
    refused(lambda r: r.ent_list.__setitem__((0, 0), -1))
    refused(lambda r: r.ent_pos.__setitem__((0, 0), SIZES[0]))             # a position out of range
    refused(lambda r: r.ent_list.__setitem__((33, 0), 2))                  # (no row in the empty list)
    refused(lambda r: r.pair_slots.__setitem__((1, 1), 40))                # a record number outside [-1, max_recs)
    refused(lambda r: r.pair_slots.__setitem__((1, 1), -2))
    refused(lambda r: r.pair_head.__setitem__(1, 40))
    refused(lambda r: r.rec_hdr.__setitem__((5, 0), 41))
    refused(lambda r: r.rec_hdr.__setitem__((5, 1), 33))                   # more entries than a record holds
    refused(lambda r: r.rec_hdr.__setitem__((r.pair_head[0], 0), r.pair_head[0]))  # a chain that does not end
    refused(lambda r: None, k=17)
    refused(lambda r: None, lists=np.array([0, len(SIZES)], np.int64))
    from quake_amd.capi import Store
    wide = Store(ctx, 272)
    wide.build_csr(np.array([0, 16], np.int64), np.arange(16, dtype=np.int64), np.zeros((16, 272), np.float32))
    r = Y.Records(1, 1)
    with pytest.raises(QuakeHipError):
        ctx.shadow_finish(wide, np.zeros((1, 272), np.float32), E[:1], lists[:1], k=k, metric=metric, **r.arrays())
    assert ctx.shadow_stats() == after, "a refused call launches nothing"
