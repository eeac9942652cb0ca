"""Multi-vector search on the CPU: tests/maxsim_yardstick.py against a plain Python triple loop on tiny inputs, against grouped
search's yardstick where one sub-query and ids-as-groups make the two the same statement, and against range search's hit counts."""
import math

import numpy as np
import pytest

import grouped_yardstick as GY
import maxsim_yardstick as MY
import oracle as O
import range_yardstick as RY

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def _tiny(metric, seed, n=60, d=8, nlist=4):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    sizes = [n // 2, 0, n // 4, n - n // 2 - n // 4]
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    ids = rng.permutation(n).astype(np.int64) + 3
    return x, ids, offsets


def _triple_loop(q3, vecs, ids, offsets, pids, k, metric, col, radius, n_tokens, missing):
    """the definition, one Python statement after the other: float32 through np.float32 scalars only"""
    L, T, _ = q3.shape
    out = []
    for l in range(L):
        nt = T if n_tokens is None else n_tokens[l]
        best = {}   # value -> {t: best reported distance}
        hits = [0] * T
        for t in range(nt):
            for p in pids[l * T + t]:
                if p < 0 or p >= len(offsets) - 1:
                    continue
                for row in range(offsets[p], offsets[p + 1]):
                    v = O.pair_values(q3[l, t][None, :], vecs[row:row + 1], metric)[0, 0]
                    dist = np.float32(math.sqrt(v)) if metric == "l2" else np.float32(v)
                    if math.isnan(dist) or not (dist <= np.float32(radius) if metric == "l2" else dist >= np.float32(radius)):
                        continue
                    hits[t] += 1
                    if int(ids[row]) not in col:
                        continue
                    b = best.setdefault(col[int(ids[row])], {})
                    if t not in b or (dist < b[t] if metric == "l2" else dist > b[t]):
                        b[t] = dist
        scored = []
        for g, b in best.items():
            s = np.float32(0.0)
            with np.errstate(invalid="ignore"):
                for t in range(nt):
                    s = np.float32(s + (b[t] if t in b else np.float32(missing)))
            scored.append((g, s, len(b)))
        scored.sort(key=lambda e: (math.isnan(e[1]), 0.0 if math.isnan(e[1]) else float(-e[1] if metric == "ip" else e[1]), e[0]))
        out.append((scored[:k], len(scored), hits))
    return out


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("case", range(4))
def test_against_the_triple_loop(metric, case):
    x, ids, offsets = _tiny(metric, 100 + case)
    rng = np.random.default_rng(200 + case)
    L, T, k = 3, (1, 2, 3, 4)[case], (1, 3, 5, 40)[case]
    q3 = rng.standard_normal((L, T, x.shape[1])).astype(np.float32)
    pids = np.stack([rng.permutation(4)[:3] for _ in range(L * T)]).astype(np.int64)
    pids[0, 1] = -1
    with_value = ids[rng.random(ids.shape[0]) < 0.8]
    vals = rng.integers(-3, 4, size=with_value.shape[0]).astype(np.int64)
    vals[:2] = (I64MIN, I64MAX)
    col = dict(zip(with_value.tolist(), vals.tolist()))
    dist = np.sqrt(O.pair_values(q3.reshape(-1, x.shape[1]), x, "l2")) if metric == "l2" else O.pair_values(q3.reshape(-1, x.shape[1]), x, "ip")
    radius = (None, float(np.quantile(dist, 0.5 if metric == "l2" else 0.5)), float(np.quantile(dist, 0.3 if metric == "l2" else 0.7)), None)[case]
    n_tokens = (None, [2, 0, 1], None, [4, 1, 0])[case]
    missing = (0.0, 1.5, -2.0, float("inf"))[case]
    got = MY.scan(q3, x, ids, offsets, pids, k, metric, with_value, vals, radius=radius, n_tokens=n_tokens, missing=missing)
    r = radius if radius is not None else (math.inf if metric == "l2" else -math.inf)
    want = _triple_loop(q3, x, ids, offsets, pids, k, metric, col, r, n_tokens, missing)
    groups, scores, matched, n_groups, hits = got
    pad = np.float32(np.inf if metric == "l2" else -np.inf)
    for l, (top, n, h) in enumerate(want):
        assert n_groups[l] == n and hits[l].tolist() == h
        assert groups[l, :len(top)].tolist() == [g for g, _, _ in top]
        assert scores[l, :len(top)].view(np.uint32).tolist() == [int(np.float32(s).view(np.uint32)) for _, s, _ in top]
        assert matched[l, :len(top)].tolist() == [m for _, _, m in top]
        assert (groups[l, len(top):] == 0).all() and (scores[l, len(top):] == pad).all() and (matched[l, len(top):] == 0).all()
    assert sum(n for _, n, _ in want) > 0


def test_by_hand():
    # one list, four rows on the first axis; two sub-queries; IP, so a term is the largest product
    vecs = np.array([[1, 0], [2, 0], [0, 3], [0, -1]], np.float32)
    ids = np.array([10, 11, 12, 13], np.int64)
    offsets = np.array([0, 4], np.int64)
    q3 = np.array([[[1, 0], [0, 1]]], np.float32)
    col_ids, col_vals = np.array([10, 11, 12, 13]), np.array([5, 5, -1, 7])
    g, s, m, n, h = MY.scan(q3, vecs, ids, offsets, np.array([0]), 4, "ip", col_ids, col_vals)
    # value 5: max(1, 2) + max(0, 0) = 2; value -1: 0 + 3 = 3; value 7: 0 + -1 = -1
    assert g.tolist() == [[-1, 5, 7, 0]] and s[0, :3].tolist() == [3.0, 2.0, -1.0] and np.isneginf(s[0, 3])
    assert m.tolist() == [[2, 2, 2, 0]] and n.tolist() == [3] and h.tolist() == [[4, 4]]
    # a radius of 0.5 drops the zeros and the negative product: a sub-query without a candidate contributes `missing`
    g, s, m, n, h = MY.scan(q3, vecs, ids, offsets, np.array([0]), 4, "ip", col_ids, col_vals, radius=0.5, missing=-10.0)
    assert g.tolist() == [[-1, 5, 0, 0]] and s[0, :2].tolist() == [-7.0, -8.0] and m.tolist() == [[1, 1, 0, 0]]
    assert n.tolist() == [2] and h.tolist() == [[2, 1]]
    # n_tokens = 1 leaves the second sub-query out, n_tokens = 0 everything
    g, s, _, n, h = MY.scan(q3, vecs, ids, offsets, np.array([0]), 2, "ip", np.array([10, 11]), np.array([9, -9]), n_tokens=[1], radius=0.5)
    assert g.tolist() == [[-9, 9]] and s.tolist() == [[2.0, 1.0]] and h.tolist() == [[2, 0]]
    # equal scores: the smaller signed value first
    g, s, _, _, _ = MY.scan(np.array([[[1, 0]]], np.float32), np.array([[1, 0], [1, 0], [1, 0]], np.float32), np.array([1, 2, 3]),
                            np.array([0, 3]), np.array([0]), 3, "ip", np.array([1, 2, 3]), np.array([9, I64MIN, -9]))
    assert g.tolist() == [[I64MIN, -9, 9]] and s.tolist() == [[1.0, 1.0, 1.0]]
    g, s, _, n, _ = MY.scan(q3, vecs, ids, offsets, np.array([0]), 2, "ip", np.array([10, 12]), np.array([4, 3]), missing=1.0, radius=2.5)
    assert g.tolist() == [[3, 0]] and s[0, 0] == 4.0 and n.tolist() == [1]   # 1.0 (missing) + 3.0
    g, _, _, n, h = MY.scan(q3, vecs, ids, offsets, np.array([0]), 2, "ip", col_ids, col_vals, n_tokens=[0])
    assert g.tolist() == [[0, 0]] and n.tolist() == [0] and h.tolist() == [[0, 0]]
    # inf + -inf: the NaN score goes behind every number, NaN among NaN by value
    vecs2 = np.array([[np.inf, 0], [1, 0], [2, 0]], np.float32)
    q2 = np.array([[[-1, 0], [1, 0]]], np.float32)
    g, s, _, _, _ = MY.scan(q2, vecs2, np.array([1, 2, 3]), np.array([0, 3]), np.array([0]), 3, "ip", np.array([1, 2, 3]), np.array([8, 6, 4]))
    assert g.tolist() == [[4, 6, 8]] and s[0, :2].tolist() == [0.0, 0.0] and np.isnan(s[0, 2])
    # the sequential sum: (2^26 + 1) - 2^26 is 0 in float32, (2^26 - 2^26) + 1 is 1: the order of the tokens decides
    big = np.float32(2.0 ** 26)
    vecs3 = np.array([[big, 1, -big]], np.float32)   # one row: the three sub-queries read 2^26, 1, -2^26 off it
    q5 = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    _, s, _, _, _ = MY.scan(q5, vecs3, np.array([1]), np.array([0, 1]), np.array([0]), 1, "ip", np.array([1]), np.array([1]))
    assert s.tolist() == [[0.0]]
    _, s, _, _, _ = MY.scan(q5[:, [0, 2, 1]], vecs3, np.array([1]), np.array([0, 1]), np.array([0]), 1, "ip", np.array([1]), np.array([1]))
    assert s.tolist() == [[1.0]]


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_one_token_is_grouped_search(metric):
    """T = 1, every id its own group, no radius: the k best groups are the k nearest rows, scores their distances"""
    c = RY.corpus(16, 9, 700, metric, seed=5)
    q = RY.queries(c, 6, seed=6)
    pids = np.stack([np.random.default_rng(7 + i).permutation(9)[:4] for i in range(6)]).astype(np.int64)
    k = 20
    gi, gd, gg = GY.scan(q, c["vecs"], c["ids"], c["offsets"], pids, k, metric, c["ids"], c["ids"])
    assert all(np.unique(gd[i][gi[i] >= 0]).shape[0] == (gi[i] >= 0).sum() for i in range(6)), "the data must not hold equal scores"
    groups, scores, matched, n_groups, hits = MY.scan(q[:, None, :], c["vecs"], c["ids"], c["offsets"], pids, k, metric, c["ids"], c["ids"])
    assert np.array_equal(groups, np.where(gi >= 0, gi, 0)) and np.array_equal(groups, gg)
    assert np.array_equal(scores.view(np.uint32), ((gd + np.float32(0.0)).astype(np.float32)).view(np.uint32))
    assert np.array_equal(matched, (gi >= 0).astype(np.int32))
    sizes = np.diff(c["offsets"])
    assert n_groups.tolist() == sizes[pids].sum(axis=1).tolist() == hits[:, 0].tolist()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_hits_are_range_counts(metric):
    c = RY.corpus(16, 9, 700, metric, seed=11)
    L, T = 4, 3
    q = RY.queries(c, L * T, seed=12)
    pids = np.stack([np.random.default_rng(20 + i).permutation(9)[:5] for i in range(L * T)]).astype(np.int64)
    pids[3, 2] = -1
    lims0, _, dist = RY.all_pairs(q, c["vecs"], c["ids"], c["offsets"], pids, metric)
    radius = float(np.quantile(dist, 0.1 if metric == "l2" else 0.9))
    S = c["ids"][::3]
    for kw in (dict(), dict(S=S, mode="deny")):
        lims, _, _ = RY.scan(q, c["vecs"], c["ids"], c["offsets"], pids, radius, metric, **kw)
        n_tokens = [3, 0, 2, 1]
        out = MY.scan(q.reshape(L, T, -1), c["vecs"], c["ids"], c["offsets"], pids, 5, metric, c["ids"], c["ids"] % 7, radius=radius,
                      n_tokens=n_tokens, missing=0.25, **kw)
        want = np.diff(lims).reshape(L, T) * (np.arange(T)[None, :] < np.array(n_tokens)[:, None])
        assert np.array_equal(out[4], want) and want.sum() > 0
        assert (out[3] <= 7).all() and out[3][1] == 0
