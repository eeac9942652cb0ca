"""On the CPU: the seed set of the feature sweep (tests/random_features.py, run on the device by tests/test_random_shapes_gpu.py)
reaches what the sweep exists for.  These are conditions on the cases' own inputs and on the yardsticks' answers, not measurements:
where a draw misses one, the draw changes and the condition stays."""
import numpy as np
import pytest

import grouped_members_yardstick as GMY
import grouped_yardstick as GY
import random_features as RF
import range_yardstick as RY

SEEDS = sorted(set(range(48)) | {107})   # the default set, whatever QK_RANDOM_FEATURES says


def _db(d):
    nblk = (d + 15) // 16
    return 8 if nblk % 8 == 0 else 4 if nblk % 4 == 0 else 2 if nblk % 2 == 0 else 1


def _facts(c):
    """what one case reaches, from its inputs and its expected answers"""
    f, k, Q, m = c["f"], c["k"], c["Q"], c["f"]["m"]
    e = RF.expected(c)
    sizes = np.diff(c["offsets"])
    out = dict(d=c["d"], nlist=c["nlist"], lists_with_rows=int((sizes > 0).sum()), ragged=c["d"] % 16 != 0,
               db=_db(c["d"]), integer=c["integer"], empty=bool((sizes == 0).any()), q33=Q > 32, refused=RF.refused_legs(c))
    fi = e["filtered"][0]
    out["full_first_page"] = bool((fi[:, k - 1] >= 0).all())
    out["padding"] = bool((fi < 0).any())
    pg = e["pages_filtered"]
    out["three_pages"] = bool((pg["ids"][:, RF.PAGES * k - 1] >= 0).any())
    tie = False
    for key, have in ((e[name]["keys"], e[name]["ids"] >= 0) for name in ("pages", "pages_filtered")):
        for p in range(RF.PAGES):
            b = (p + 1) * k
            tie = tie or bool((have[:, b] & (key[:, b - 1] == key[:, b])).any())
    out["boundary_in_a_run"] = tie
    # range: hits, and a query whose hits are fewer than its probed rows
    probed = RY.probed(c["q"], c["cent"], c["offsets"], c["nprobe"], c["metric"])
    rows = np.where(probed >= 0, sizes[np.maximum(probed, 0)], 0).sum(1)
    hits = np.diff(e["range"][0])
    out["range_hits"] = int(hits.sum())
    out["range_selects"] = bool((hits < rows).any())
    # grouped: a selected group with more candidates than m, a live group with fewer (padded members)
    q1 = np.ascontiguousarray(c["q"][:RF.ONE_AT_A_TIME])
    ai, av = f["cols"][f["group_by"]]
    counts = GMY.group_counts(q1, c["vecs"], c["ids"], c["offsets"], GY.probed(q1, c["cent"], c["offsets"], c["nprobe"], c["metric"]),
                              c["metric"], ai, av)
    wi, _, wg = e["grouped"]
    sel = [counts[i].get(int(g), 0) for i in range(wi.shape[0]) for g, h in zip(wg[i], wi[i, :, 0]) if h >= 0]
    out["group_more"] = any(n > m for n in sel)
    out["group_fewer"] = any(n < m for n in sel)
    assert out["group_fewer"] == bool(((wi[:, :, 0] >= 0) & (wi[:, :, m - 1] < 0)).any())   # fewer than m <=> padded members
    # adaptive: a query that goes beyond nprobe, a query that could have and stops there
    M = min(f["max_nprobe"], c["nlist"])
    npb = e["adaptive"][2]
    out["adaptive_beyond"] = bool((npb > c["nprobe"]).any())
    out["adaptive_stops"] = bool(M > c["nprobe"] and (npb == c["nprobe"]).any())
    return out


@pytest.fixture(scope="module")
def facts():
    return {seed: _facts(RF.feature_case(seed)) for seed in SEEDS}


def _count(facts, key, want=True):
    return sum(1 for f in facts.values() if f[key] == want)


def test_the_draws_of_the_plain_sweep_did_not_move():
    from test_random_shapes_gpu import _case
    for seed in (0, 7, 107):
        a, b = _case(np.random.default_rng(1000 + seed)), RF.feature_case(seed)
        for kk, v in a.items():
            assert np.array_equal(v, b[kk]), (seed, kk)


def test_shapes(facts):
    assert _count(facts, "ragged") >= 20
    for db in (1, 2, 4, 8):
        assert _count(facts, "db", db) >= 2, db
    assert _count(facts, "integer") >= 10
    assert _count(facts, "empty") >= 20
    assert _count(facts, "q33") >= 20


def test_filtered(facts):
    n = len(facts)
    assert 3 * _count(facts, "full_first_page") >= n, _count(facts, "full_first_page")
    assert 4 * _count(facts, "padding") >= n, _count(facts, "padding")


def test_paged(facts):
    assert _count(facts, "three_pages") >= 10
    assert sum(1 for f in facts.values() if f["integer"] and f["boundary_in_a_run"]) >= 5


def test_range(facts):
    assert all(f["range_hits"] >= 1 for f in facts.values()), [s for s, f in facts.items() if f["range_hits"] < 1]
    assert 3 * _count(facts, "range_selects") >= 2 * len(facts), _count(facts, "range_selects")


def test_grouped(facts):
    assert _count(facts, "group_more") >= 10
    assert _count(facts, "group_fewer") >= 10


def test_adaptive(facts):
    assert _count(facts, "adaptive_beyond") >= 8
    assert _count(facts, "adaptive_stops") >= 8


def test_no_leg_is_refused_often(facts):
    for leg in RF.LEGS:
        assert 8 * sum(1 for f in facts.values() if leg in f["refused"]) <= len(facts), leg


def test_mutation_seeds(facts):
    assert len(set(RF.MUTATION_SEEDS)) == 16 and set(RF.MUTATION_SEEDS) <= set(SEEDS)
    assert sum(1 for s in RF.MUTATION_SEEDS if facts[s]["ragged"]) >= 8
    # what the mutations need: two lists with rows (a list relocates, a non-empty list is removed), four lists (the refinement)
    assert sum(1 for s in RF.MUTATION_SEEDS if facts[s]["lists_with_rows"] >= 2) >= 8
    assert sum(1 for s in RF.MUTATION_SEEDS if facts[s]["nlist"] >= 4) >= 6


def test_seam_cases():
    want = [(256, 16, False), (260, 17, True), (1000, 63, True), (3000, 188, True)]
    assert {s["metric"] for s in RF.SEAM_CASES} == {"l2", "ip"} and {s["k"] for s in RF.SEAM_CASES} == {10, 100}
    for i, (d, nblk, ragged) in enumerate(want):
        c = RF.seam_case(i)
        sizes = np.diff(c["offsets"])
        assert c["d"] == d and (d + 15) // 16 == nblk and (d % 16 != 0) == ragged
        assert c["nlist"] == 12 and (sizes == 0).sum() == 2 and c["Q"] == 20 and 1400 <= c["n"] <= 1600
        e = RF.expected(c, legs=["range", "filtered"])
        assert np.diff(e["range"][0]).sum() >= 1 and not RF.refused_legs(c)
