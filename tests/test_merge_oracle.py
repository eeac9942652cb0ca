"""The merge yardstick checked on the CPU (tests/merge_yardstick.py; the GPU side is tests/test_merge_records.py and
tests/test_merge_ranks.py): the record builder lays out well-formed structures only, the reference merge is the plain sort it claims
to be, and the special-value rules of DESIGN.md 5.8.1 hold in it."""
import numpy as np
import pytest

import merge_yardstick as Y


# ---- key maps ----------------------------------------------------------------------------------------------------------------------
def _floats(rng, n):
    v = np.concatenate([rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, size=n).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38], np.float32)])
    return np.ascontiguousarray(v, np.float32)


def test_key_maps_order_and_invert():
    rng = np.random.default_rng(1)
    v = _floats(rng, 4000)
    o = Y.ord_from_ip(v)
    a, b = rng.integers(0, v.shape[0], size=20000), rng.integers(0, v.shape[0], size=20000)
    # the larger product has the smaller key; equal products (also -0 and +0) share a key
    np.testing.assert_array_equal(v[a] > v[b], o[a] < o[b])
    np.testing.assert_array_equal(v[a] == v[b], o[a] == o[b])
    back = Y.ip_from_ord(o)
    np.testing.assert_array_equal(back.view(np.uint32), np.where(v == 0, np.float32(0.0), v).view(np.uint32))
    d = np.abs(v)
    d[d == 0] = 0.0
    ol = Y.ord_from_l2(d)
    np.testing.assert_array_equal(d[a] < d[b], ol[a] < ol[b])
    np.testing.assert_array_equal(Y.dist_from_ord(ol, "l2", False).view(np.uint32), d.view(np.uint32))
    np.testing.assert_array_equal(Y.dist_from_ord(ol, "l2", True), np.sqrt(d))
    assert (o != Y.NAN_KEY).all() and (ol != Y.NAN_KEY).all()
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFC12345], np.uint32).view(np.float32)
    assert (Y.ord_from_ip(nans) == Y.NAN_KEY).all() and (Y.ord_from_l2(nans) == Y.NAN_KEY).all()
    assert Y.ord_from_ip(np.float32([-0.0]))[0] == Y.ord_from_ip(np.float32([0.0]))[0]


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,P,metric", [(1, 1, "l2"), (22, 7, "ip"), (33, 9, "l2"), (129, 65, "ip"), (448, 8, "l2")])
def test_builder_lays_out_well_formed_records(k, P, metric):
    names, qs = Y.record_cases(k, P, metric, seed=1000 * k + P)
    assert len(set(names)) == len(names) and {"empty", "equal", "chain", "lost", "tie_records", "tie_pairs"} <= set(names)
    rb = Y.build_records(qs, k, np.random.default_rng(k + P))
    R = rb["max_recs"]
    assert rb["pair_slots"].shape == (len(qs), P, Y.QK_SLOTS) and rb["pair_head"].shape == (len(qs), P)
    assert rb["rec_ord"].shape == (R, k) and rb["rec_id"].shape == (R, k) and rb["rec_hdr"].shape == (R, 2)
    # every number a kernel may follow is -1 or names a record
    assert ((rb["pair_slots"][:, :, 1:] >= -1) & (rb["pair_slots"][:, :, 1:] < R)).all()
    assert ((rb["pair_head"] >= -1) & (rb["pair_head"] < R)).all()
    assert ((rb["rec_hdr"][:, 0] >= -1) & (rb["rec_hdr"][:, 0] < R)).all()
    assert ((rb["rec_hdr"][:, 1] >= 0) & (rb["rec_hdr"][:, 1] <= k)).all()
    seen = []
    saw_chain = saw_lost = False
    for q, qp in enumerate(qs):
        got_k, got_i = [], []
        for p, recs in enumerate(qp):
            count = int(rb["pair_slots"][q, p, 0])
            assert count == len(recs)
            n_lost = sum(1 for r in recs if len(r) > 2 and r[2])
            walked = Y.walk_records(rb, q, p)               # (asserts the chain ends and stays inside the arrays)
            assert len(walked) == count - n_lost
            line = rb["pair_slots"][q, p, 1:1 + min(count, 31)]
            chain = len(walked) - int((line >= 0).sum())
            assert chain == max(0, count - 31) - sum(1 for r in recs[31:] if len(r) > 2 and r[2])
            saw_chain |= chain in (256, 257)
            saw_lost |= bool((line[1:-1] == -1).any()) if line.shape[0] >= 3 else False
            seen += walked
            for r in walked:
                n = int(rb["rec_hdr"][r, 1])
                assert 1 <= n <= k
                ko, io = rb["rec_ord"][r], rb["rec_id"][r]
                o = np.lexsort((io[:n], ko[:n]))
                np.testing.assert_array_equal(o, np.arange(n))                      # sorted under (key, id)
                assert (ko[n:] == Y.POISON_KEY).all() and (io[n:] == Y.POISON_ID).all()
                assert (io[:n] != Y.POISON_ID).all()                                # poison never inside a count
                got_k.append(ko[:n])
                got_i.append(io[:n])
        ek, ei = rb["entries"][q]
        gk = np.concatenate(got_k) if got_k else np.zeros(0, np.uint32)
        gi = np.concatenate(got_i) if got_i else np.zeros(0, np.int64)
        a, b = np.lexsort((gi, gk)), np.lexsort((ei, ek))
        np.testing.assert_array_equal(gk[a], ek[b])         # the layout holds the query's candidates, each once
        np.testing.assert_array_equal(gi[a], ei[b])
        assert np.unique(ei).shape[0] == ei.shape[0]        # unique ids (what the next cursor assumes)
    assert sorted(seen) == sorted(set(seen)) and len(seen) == rb["n_records"]       # every record reachable exactly once
    assert saw_chain and saw_lost
    big = [w for w in (Y.walk_records(rb, names.index("chain"), p) for p in range(P)) if len(w) > 31][0]
    assert (np.diff(np.asarray(big)) != 1).any()            # record numbers are permuted
    # the planted tie: the k-th and (k+1)-th of the union share a key, ids adjacent, in two records
    for nm in ("tie_records", "tie_pairs"):
        ek, ei = rb["entries"][names.index(nm)]
        bk, bi = Y.first_k(ek, ei, k + 1)
        assert bk[k - 1] == bk[k] and bi[k] - bi[k - 1] == 1
        q = names.index(nm)
        where = {}
        for p in range(P):
            for r in Y.walk_records(rb, q, p):
                for want in (bi[k - 1], bi[k]):
                    if want in rb["rec_id"][r, :rb["rec_hdr"][r, 1]]:
                        where[int(want)] = (p, r)
        (p1, r1), (p2, r2) = where[int(bi[k - 1])], where[int(bi[k])]
        assert r1 != r2 and ((p1 != p2) if (nm == "tie_pairs" and P >= 2) else (p1 == p2))


# ---- the reference merge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_reference_is_a_plain_sort_of_the_values(metric):
    rng = np.random.default_rng(5)
    for k, n in ((1, 5), (10, 300), (64, 40), (448, 3000)):
        v = Y.draw_values(n, "distinct", metric, rng)
        ids = Y.draw_ids(n, rng)
        oi, od, nk, ni = Y.merge_reference([(Y.ord_of(v, metric), ids)], k, metric, sqrt_l2=False)
        order = np.lexsort((ids, -v if metric == "ip" else v))[:k]
        m = order.shape[0]
        np.testing.assert_array_equal(oi[0, :m], ids[order])
        np.testing.assert_array_equal(od[0, :m].view(np.uint32), v[order].view(np.uint32))
        assert (oi[0, m:] == -1).all() and (od[0, m:] == Y.pad_dist(metric)).all()
        if m == k:
            assert ni[0] == ids[order[-1]] and nk[0] == Y.ord_of(v[order[-1:]], metric)[0]
        else:
            assert ni[0] == Y.INT64_MAX and nk[0] == Y.NAN_KEY
    # sqrt only under L2, correctly rounded
    v = np.float32([4.0, 2.0, 9.0])
    _, od, _, _ = Y.merge_reference([(Y.ord_of(v, "l2"), np.int64([1, 2, 3]))], 3, "l2", sqrt_l2=True)
    np.testing.assert_array_equal(od[0], np.sqrt(np.float32([2.0, 4.0, 9.0])))


def test_special_values_follow_the_rule():
    nan = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    # L2: NaN is dropped whatever its id, +inf is an ordinary value in front of the padding
    ids = np.int64([[[7, 3, 9, -1]], [[5, 4, 2, -1]]])
    keys = np.float32([[[1.0, np.inf, nan, np.inf]], [[0.5, np.inf, nan, np.inf]]])
    oi, od = Y.merge_ranks_reference(ids, keys, "l2", sqrt_l2=True)
    np.testing.assert_array_equal(oi[0], [5, 7, 3, 4])
    np.testing.assert_array_equal(od[0], np.float32([np.sqrt(np.float32(0.5)), 1.0, np.inf, np.inf]))
    ids = np.int64([[[7, 9, -1, -1, -1, -1]], [[5, 2, -1, -1, -1, -1]]])
    keys = np.float32([[[np.inf, nan, 0, 0, 0, 0]], [[np.inf, nan, 0, 0, 0, 0]]])
    oi, od = Y.merge_ranks_reference(ids, keys, "l2")
    np.testing.assert_array_equal(oi[0], [5, 7, -1, -1, -1, -1])
    np.testing.assert_array_equal(od[0], np.float32([np.inf] * 6))
    # IP: both infinities are ordinary, -0 and +0 tie and the id decides, NaN is dropped
    ids = np.int64([[[10, 8, 6, 1]], [[11, 7, 5, 2]]])
    keys = np.float32([[[np.inf, 0.0, -0.0, -np.inf]], [[np.inf, -0.0, 0.0, nan]]])
    oi, od = Y.merge_ranks_reference(ids, keys, "ip")
    np.testing.assert_array_equal(oi[0], [10, 11, 5, 6])
    assert od[0, 0] == np.inf and od[0, 1] == np.inf and (od[0, 2:] == 0).all()
    oi, od = Y.merge_ranks_reference(ids[:, :, 1:], keys[:, :, 1:], "ip")
    np.testing.assert_array_equal(oi[0], [5, 6, 7])
    # the same (key, id) on two ranks is two entries
    ids = np.int64([[[3, 4]], [[3, 9]]])
    keys = np.float32([[[1.0, 2.0]], [[1.0, 1.5]]])
    oi, _ = Y.merge_ranks_reference(ids, keys, "l2")
    np.testing.assert_array_equal(oi[0], [3, 3])
    # sorted_runs: candidates, then NaN keys, then the -1 padding
    si, sk = Y.sorted_runs(np.int64([[[-1, 4, 2, 9]]]), np.float32([[[np.inf, nan, 3.0, 1.0]]]), "l2")
    np.testing.assert_array_equal(si[0, 0], [9, 2, 4, -1])
    assert np.isnan(sk[0, 0, 2]) and sk[0, 0, 0] == 1.0
