"""Adaptive probing under a filter, the part that needs no GPU: tests/adaptive_yardstick.py is pinned against the yardstick of
filtered search and against its own definition, the entry point is declared, exported and bound, and both mirrors carry the new
SearchParams / SearchResult fields with their defaults outside the summaries.  (The refusals of QuakeIndex.search need a built
index: tests/test_adaptive_search.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_yardstick as A
import filter_yardstick as Y
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corpus(d, nlist, n, metric, seed):
    """clustered rows in skewed lists, two of them empty"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 0.05
    w[:2] = 0.0
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    x = (cent[assign] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64) + 11
    order = np.argsort(assign, kind="stable")
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    q = (x[rng.integers(0, n, size=23)] + 0.05 * rng.standard_normal((23, d))).astype(np.float32)
    if metric == "ip":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(cent=cent, vecs=np.ascontiguousarray(x[order]), ids=np.ascontiguousarray(ids[order]), offsets=offsets,
                q=np.ascontiguousarray(q), metric=metric)


@pytest.fixture(scope="module", params=["l2", "ip"])
def corpus(request):
    return _corpus(16, 40, 3000, request.param, seed=5 + (request.param == "ip"))


def _sets(c):
    rng = np.random.default_rng(77)
    return [(Y.draw_set(c["ids"], 0.1, rng), "allow"), (Y.draw_set(c["ids"], 0.01, rng), "allow"), (Y.draw_set(c["ids"], 0.3, rng), "deny"),
            (np.zeros(0, np.int64), "allow")]


def _run(c, nprobe, max_nprobe, minc, k, flt, qf=None):
    return A.search(c["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, max_nprobe, minc, k, c["metric"], flt, qf)


def test_max_nprobe_equal_to_nprobe_is_the_filtered_search(corpus):
    c = corpus
    for S, mode in _sets(c):
        for nprobe, k in [(1, 1), (4, 10), (9, 100), (64, 10)]:  # (64 > 40 lists)
            for minc in (1, 10 ** 9):
                gi, gd, npd, pr = _run(c, nprobe, nprobe, minc, k, [(S, mode)])
                oi, od = Y.search(c["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], nprobe, k, c["metric"], S, mode)
                np.testing.assert_array_equal(gi, oi)
                np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
                assert (npd == min(nprobe, 40)).all() and (pr >= 0).all()


def test_nprobed_is_monotone_in_min_candidates(corpus):
    c = corpus
    for flt in _sets(c):
        last = None
        for minc in (1, 2, 5, 10, 40, 200, 10 ** 9):
            _, _, npd, _ = _run(c, 2, 33, minc, 10, [flt])
            assert ((npd >= 2) & (npd <= 33)).all()
            if last is not None:
                assert (npd >= last).all(), minc
            last = npd
        assert (last == 33).all()  # nobody has 10^9 candidates


def test_the_prefix_is_the_shortest_that_holds_min_candidates(corpus):
    c = corpus
    sets = _sets(c)
    qf = (np.arange(c["q"].shape[0]) % len(sets)).astype(np.int32)
    n0, M = 3, 37
    seen_inner = False
    for minc in (1, 7, 40, 150):
        gi, _, npd, pr = _run(c, n0, M, minc, 10, sets, qf)
        for i in range(qf.shape[0]):
            cnt = A.list_counts(A.keep_of(sets[qf[i]], c["ids"]), c["offsets"])
            t = int(npd[i])
            assert (pr[i, :t] >= 0).all() and (pr[i, t:] == -1).all()
            have = int(cnt[pr[i, :t]].sum())
            if t < M:
                assert have >= minc, (minc, i)
                if t > n0:
                    seen_inner = True
                    assert int(cnt[pr[i, :t - 1]].sum()) < minc, (minc, i)
            else:
                assert t == M
            # the row holds what the prefix holds, up to k
            assert (gi[i] >= 0).sum() == min(10, have), (minc, i)
    assert seen_inner


def test_out_of_range_filter_number_is_an_empty_row(corpus):
    c = corpus
    sets = _sets(c)[:2]
    qf = np.array([0, 1, 2, -1] + [0] * (c["q"].shape[0] - 4), np.int32)
    gi, gd, npd, pr = _run(c, 2, 9, 5, 3, sets, qf)
    for i in (2, 3):
        assert npd[i] == 0 and (pr[i] == -1).all() and (gi[i] == -1).all() and (gd[i] == A.pad_of(c["metric"])).all()
    assert (npd[[0, 1]] >= 2).all()


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    name = "qk_search_filtered_adaptive"
    header = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    assert name in set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", header))
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    # the batch signature plus max_nprobe, min_candidates, out_nprobed, out_probed
    sig = _lib.SIGNATURES[name][1]
    assert len(sig) == len(_lib.SIGNATURES["qk_search_filtered_batch"][1]) + 4
    args = [1 if t in (C.c_int, C.c_int64) else None for t in sig]
    args[[i for i, t in enumerate(sig) if t == C.POINTER(C.c_void_p)][0]] = (C.c_void_p * 1)(None)
    assert getattr(lib, name)(*args) == 1  # QK_ERR_INVALID: a null context
    assert name.encode() in lib.qk_last_error()


def test_both_mirrors_carry_the_fields_outside_the_summaries():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake._bindings as qb
    import quake_amd as qa
    for mod in (qb, qa):
        sp = mod.SearchParams()
        assert sp.max_nprobe == 0 and sp.filter_min_candidates == 0
        before = repr(sp)
        sp.max_nprobe, sp.filter_min_candidates = 128, 40
        assert (sp.max_nprobe, sp.filter_min_candidates) == (128, 40)
        assert repr(sp) == before and "max_nprobe" not in before and "filter_min_candidates" not in before
        r = mod.SearchResult()
        assert r.nprobed is None
    assert repr(qb.SearchParams()) == repr(qa.SearchParams())
