"""CPU: the properties that make the cases of tests/aps_yardstick.py reach their branches on the device, computed with the oracle
alone -- a later change to a builder cannot silently turn a case into an easy one.

  * every case: the walk's answer is the fixed-nprobe answer over the lists it visited (tests/test_oracle_aps.py::test_search_aps_walk,
    extended to k up to QK_MAX_K, lists shorter than k, the non-finite corpora, the wide row, a parent with non-identity ids and a
    hole in the list numbers);
  * the walk lengths that the long-round and capped-round cases rest on;
  * the non-finite corpora: the walk returns no NaN pair, and (every class but `underflow`) some query visits a list with planted rows."""
import numpy as np
import pytest

import aps_yardstick as AY
import nonfinite_yardstick as NF
import oracle as O

_UNIQUE = list({AY.case_key(c): c for c in AY.ALL + AY.GROUP}.values())


@pytest.mark.parametrize("c", _UNIQUE, ids=AY.case_id)
def test_walk_is_fixed_nprobe_over_the_visited_prefix(c):
    co = AY.corpus(c)
    oi, od, on = AY.expected(c)
    M = AY.M_of(c)
    assert on.min() >= 2 and on.max() <= M
    if c["target"] > 1.0:   # never reached: every candidate is scanned
        assert (on == M).all()
    wi, wd, _ = AY.fixed_nprobe_answer(c, co, on)
    AY.assert_same(c, (wi, wd, on), (oi, od, on))


def test_case_tables():
    ks = sorted({c["k"] for c in AY.K_BUCKETS})
    assert ks == [33, 64, 65, 128, 129, 256, 257, 448] and AY.QK_MAX_K == 448
    # both sides of every pool size of k_aps_update<MAXCH>: 2k <= 64 / 128 / 256 / 512 / more
    buckets = {k: sum(2 * k > b for b in (64, 128, 256, 512)) for k in ks}
    assert buckets == {33: 1, 64: 1, 65: 2, 128: 2, 129: 3, 256: 3, 257: 4, 448: 4}
    assert len(AY.NONFINITE) == 32 and {c["cls"] for c in AY.NONFINITE} == set(NF.CLASSES)
    for c in AY.K_BUCKETS + AY.LONG_ROUNDS + AY.NONFINITE + AY.WIDE + AY.SQUARED + AY.FIRST_ROUND:
        assert AY.round_cap(c) == AY.M_of(c)   # only the capped cases have a round shorter than the candidate list
    for c in AY.CAPPED:
        assert AY.M_of(c) == 1000 and AY.round_cap(c) == 682


@pytest.mark.parametrize("c", [c for c in AY.K_BUCKETS if c["kind"] == "ivf" and c not in AY.THIN], ids=AY.case_id)
def test_bucket_walks_cross_the_first_round(c):
    on = AY.expected(c)[2]
    assert on.min() >= 2 and on.max() <= 30
    assert (on > AY.APS_FIRST).mean() >= 0.5   # (observed: 82-99 % under L2, 59-76 % under IP)


@pytest.mark.parametrize("c", AY.THIN, ids=AY.case_id)
def test_thin_lists_merge_every_answer_from_several_lists(c):
    """every list is shorter than k: a full answer needs rows of at least ceil(k / longest list) lists, so no merge step of the walk
    is idle (the 500-row lists of the other bucket cases answer most queries from the nearest list alone)"""
    co = AY.corpus(c)
    oi, od, on = AY.expected(c)
    sizes = np.diff(co["offsets"])
    assert sizes.max() < c["k"] / 1.5 and (oi >= 0).all()
    list_of = np.empty(co["ids"].max() + 1, np.int64)
    list_of[co["ids"]] = np.repeat(np.arange(c["nlist"]), sizes)
    used = np.array([np.unique(list_of[row]).shape[0] for row in oi])
    assert used.min() >= max(2, -(-c["k"] // int(sizes.max())))
    assert on.min() > AY.APS_FIRST and on.max() < AY.M_of(c)   # several rounds, and the walk stops on its own


@pytest.mark.parametrize("c", [c for c in AY.K_BUCKETS if c["kind"] == "short"], ids=AY.case_id)
def test_short_lists_keep_the_running_result_below_k(c):
    """the queries placed at the centroids of the lists cut to 0 / 4 / 9 rows: the first list they visit leaves fewer than k results,
    so the walk's first radius is the sentinel"""
    co = AY.corpus(c)
    pids, _ = O.coarse(co["q"][:3], co["centroids"], None, 1, c["metric"])
    assert list(pids[:, 0]) == list(AY.SHORT_LISTS)
    assert list(np.diff(co["offsets"])[list(AY.SHORT_LISTS)]) == list(AY.SHORT_CUTS) and max(AY.SHORT_CUTS) < c["k"]


@pytest.mark.parametrize("c", [c for c in AY.LONG_ROUNDS if c["target"] < 1.0], ids=AY.case_id)
def test_long_walks(c):
    on = AY.expected(c)[2]
    assert AY.M_of(c) == 600
    assert (on > AY.LONG_STEPS).sum() >= 5, np.sort(on)[-12:]   # a round of more than 64 steps: several ballot words
    assert on.max() < AY.M_of(c)                                 # ... and every query stops on its own


@pytest.mark.parametrize("c", [c for c in AY.CAPPED if c["target"] < 1.0], ids=AY.case_id)
def test_capped_walks_need_three_rounds(c):
    on = AY.expected(c)[2]
    assert on.min() > AY.APS_FIRST + AY.round_cap(c), on.min()   # first round + one full later round do not hold the shortest walk
    assert on.max() < AY.M_of(c)                                 # ... and every query stops on its own


@pytest.mark.parametrize("c", AY.NONFINITE, ids=AY.case_id)
def test_nonfinite_walks(c):
    co = AY.corpus(c)
    oi, od, on = AY.expected(c)
    NF.assert_no_nan_pair(co, co["q"], co["special_q"], oi)
    assert np.isfinite(co["centroids"]).all()
    if c["cls"] != "underflow":
        pids, _ = O.coarse(co["q"], co["centroids"], None, AY.M_of(c), c["metric"], num_threads=8)
        planted = list(co["hosts"]) + [co["tiny"]]
        assert any(np.isin(pids[i, :on[i]], planted).any() for i in range(co["q"].shape[0]))
        if c["cls"] in ("nan", "inf"):
            assert not np.isfinite(co["vecs"][co["special"]]).all()


def test_parent_steps():
    """section d: every state's walk is the fixed-nprobe answer over its prefix; the edits change the walk (a stale map or a stale
    centroid row would show), and the deleted list shortens the candidate list by one"""
    c = AY.PARENT_CASE
    steps = AY.parent_steps()
    assert [s["name"] for s in steps] == ["first", "replaced", "second parent", "first parent again", "list deleted"]
    walks = []
    for st in steps:
        oi, od, on = AY.step_walk(st)
        wi, wd, pids = AY.fixed_nprobe_answer(c, st, on, centroid_ids=st["centroid_ids"], nlist_present=st["nlist_present"])
        AY.assert_same(c, (wi, wd, on), (oi, od, on), st["name"])
        assert pids.shape[1] == AY.M_of(c, st["nlist_present"]) and (pids >= 0).all()
        walks.append((oi, on, pids))
    p = steps[1]["replaced"][0]
    assert (walks[0][2][:, 0] == p).sum() >= 3
    for a, b in ((0, 1), (1, 2), (3, 4)):
        assert (walks[a][1] != walks[b][1]).any() or (walks[a][0] != walks[b][0]).any()
        assert (walks[a][2][:, :walks[b][2].shape[1]] != walks[b][2]).any()   # the candidate ranking itself differs
    np.testing.assert_array_equal(walks[1][0], walks[3][0])
    h = steps[4]["removed"]
    assert walks[4][2].shape[1] == 29 and not (walks[4][2] == h).any() and (walks[3][2][:, 0] == h).any()
    # the oracle's new argument changes M only, and nothing when it names the CSR length
    a = AY.oracle_walk(c, steps[0], centroid_ids=steps[0]["centroid_ids"], nlist_present=c["nlist"])
    b = AY.oracle_walk(c, steps[0], centroid_ids=steps[0]["centroid_ids"])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    short = AY.oracle_walk(c, steps[0], centroid_ids=steps[0]["centroid_ids"], nlist_present=20)
    assert short[2].max() <= 10
