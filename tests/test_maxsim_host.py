"""Multi-vector search without a device: the argument normalisation of the mirrors (quake_amd/where.py: lower_maxsim; quake_amd/cpp:
lower_maxsim, exposed by the bindings) -- the same results and the same errors in both -- the refusals that need no device, and the
C ABI of qk_maxsim_search / qk_maxsim_scan as far as it can be checked without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = r"\[QuakeIndex::multi_vector_search\(\)\] "


@pytest.fixture(scope="module")
def mirrors():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    from quake_amd.where import lower_maxsim
    return lower_maxsim, b.lower_maxsim


def test_lower_maxsim(mirrors):
    from quake_amd import where
    assert (where.QK_MAXSIM_MAX_TOKENS, where.QK_MAXSIM_MAX_K) == (64, 1024)
    cols = ["doc", "page"]
    for lower in mirrors:
        assert tuple(lower(cols, "doc", 10, 32)) == ("doc", 10, 32, None, 0.0)
        assert tuple(lower(cols, "page", 1, 1, [0, 1], 2.5, "l2")) == ("page", 1, 1, [0, 1], 2.5)
        assert tuple(lower(cols, "page", 1024, 64, [64, 0, 7], -1.0, "ip")) == ("page", 1024, 64, [64, 0, 7], -1.0)
        assert tuple(lower(cols, "doc", 3, 2, None, float("inf"), "l2")) == ("doc", 3, 2, None, float("inf"))
        assert tuple(lower(cols, "doc", 3, 2, missing=float("-inf"), metric="l2"))[4] == float("-inf")
        assert tuple(lower(cols, "doc", 3, 2, n_tokens=[], missing=0, metric="l2")) == ("doc", 3, 2, [], 0.0)
        for args, match in ((("nope", 5, 4), WHO + "unknown attribute column 'nope'"),
                            (("doc", 0, 4), WHO + "k=0 must be between 1 and 1024"),
                            (("doc", 1025, 4), "k=1025 must be between 1 and 1024"),
                            (("doc", 5, 0), WHO + "T=0 vectors per query must be between 1 and 64"),
                            (("doc", 5, 65), "T=65 vectors per query must be between 1 and 64"),
                            (("doc", 5, 4, [4, 5]), WHO + r"n_tokens\[1\]=5 must be between 0 and T=4"),
                            (("doc", 5, 4, [-1]), r"n_tokens\[0\]=-1 must be between 0 and T=4"),
                            (("doc", 5, 4, None, None, "l2"), WHO + "missing must be given for the l2 metric"),
                            (("doc", 5, 4, None, float("nan")), WHO + "missing is NaN"),
                            (("doc", 5, 4, None, float("nan"), "l2"), "missing is NaN"),
                            # several faults: the column first, then k, T, n_tokens, missing
                            (("nope", 0, 0, [9], float("nan")), "unknown attribute column 'nope'"),
                            (("doc", 0, 0, [9], float("nan")), "k=0 must be"),
                            (("doc", 5, 0, [9], float("nan")), "T=0 vectors"),
                            (("doc", 5, 4, [9], float("nan")), r"n_tokens\[0\]=9"),
                            (("doc", 5, 4, [4], None, "l2"), "missing must be given")):
            with pytest.raises(RuntimeError, match=match):
                lower(cols, *args)
        with pytest.raises(RuntimeError, match="unknown attribute column 'doc'"):
            lower([], "doc", 5, 4)
    # the same message, character for character
    for args in (("nope", 5, 4), ("doc", 0, 4), ("doc", 5, 100), ("doc", 5, 4, [1, 2, 7]), ("doc", 5, 4, None, None, "l2"),
                 ("doc", 5, 4, None, float("nan"))):
        msgs = []
        for lower in mirrors:
            with pytest.raises(RuntimeError) as ei:
                lower(cols, *args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1], msgs
    # the Python mirror also says what is wrong with a name, a k, an n_tokens or a missing of another type
    with pytest.raises(RuntimeError, match="group_by must be the name"):
        mirrors[0](cols, ["doc"], 5, 4)
    with pytest.raises(RuntimeError, match="integers"):
        mirrors[0](cols, "doc", 2.5, 4)
    with pytest.raises(RuntimeError, match="n_tokens must be a sequence"):
        mirrors[0](cols, "doc", 5, 4, 3)
    with pytest.raises(RuntimeError, match="missing must be a number"):
        mirrors[0](cols, "doc", 5, 4, None, "zero")


def test_refusals_without_a_device():
    """an index that was never built refuses in both mirrors before anything touches a device"""
    import torch

    import quake_amd as quake
    import quake_amd.bindings as qb
    for mod in (quake, qb):
        idx = mod.QuakeIndex()
        sp = mod.SearchParams()
        sp.k = 5
        with pytest.raises(RuntimeError, match=WHO + r"No query coordinator. Did you build the index\?"):
            idx.multi_vector_search(torch.zeros(2, 3, 8), "doc", sp)
        with pytest.raises(RuntimeError, match="No query coordinator"):
            idx.multi_vector_search(torch.zeros(2, 3, 8), "doc", sp, radius=1.0, n_tokens=[1, 2], missing=0.5)
        r = mod.MultiVectorSearchResult()
        for name in ("groups", "scores", "matched", "n_groups", "hits", "column", "timing_info"):
            assert hasattr(r, name), name


def test_abi():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    assert re.search(r"^#define\s+QK_MAXSIM_MAX_TOKENS\s+64\b", txt, re.M) and re.search(r"^#define\s+QK_MAXSIM_MAX_K\s+1024\b", txt, re.M)
    from quake_amd import _lib, capi
    from quake_amd.build import SOURCES, build_lib
    assert "qk_maxsim.hip" in SOURCES
    build_lib()
    lib = _lib.load()
    for name in ("qk_maxsim_search", "qk_maxsim_scan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"QK_API\s+int\s+%s\s*\(" % name, txt)
    # search has the parent and nprobe where scan has pids and P; the rest is the same list
    a, b = _lib.SIGNATURES["qk_maxsim_search"][1], _lib.SIGNATURES["qk_maxsim_scan"][1]
    assert len(a) == 21 and len(b) == 21 and a[8:] == b[8:] and a[4:7] == b[3:6]
    assert _lib.header_constant("QK_MAXSIM_MAX_K") == capi.QK_MAXSIM_MAX_K == 1024
    assert _lib.header_constant("QK_MAXSIM_MAX_TOKENS") == capi.QK_MAXSIM_MAX_TOKENS == 64
    import quake_amd
    assert hasattr(capi.Context, "maxsim_search") and hasattr(capi.Context, "maxsim_scan")
    assert hasattr(quake_amd.QuakeIndex, "multi_vector_search") and hasattr(quake_amd, "MultiVectorSearchResult")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "qk_maxsim_search" in doc and "qk_maxsim_scan" in doc
