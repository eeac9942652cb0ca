"""Diversified search without a device: the argument normalisation of the mirrors (quake_amd/where.py: lower_diverse;
quake_amd/cpp: lower_diverse, exposed by the bindings) -- the same results and the same errors in both -- the refusals that need
no device, the header's text on the limits, and the C ABI of qk_diverse_search / qk_diverse_scan as far as it can be checked
without a GPU."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirrors():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    from quake_amd.where import lower_diverse
    return lower_diverse, b.lower_diverse


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_lower_diverse(mirrors):
    from quake_amd import where
    assert where.QK_MAX_FETCH_K == 256
    for lower in mirrors:
        assert tuple(lower(10, 50)) == (10, 50, 0.5)
        assert tuple(lower(1, 1, 0.0)) == (1, 1, 0.0)
        assert tuple(lower(256, 256, 1.0)) == (256, 256, 1.0)
        assert tuple(lower(3, 17, 1)) == (3, 17, 1.0)
        # lambda is what the library computes with: the float32 nearest to the argument
        assert tuple(lower(2, 64, 0.3)) == (2, 64, f32(0.3)) and f32(0.3) != 0.3
        assert tuple(lower(k=2, fetch_k=65, lambda_mult=0.7)) == (2, 65, f32(0.7))
        for args, match in (((0, 5), r"\[QuakeIndex::diverse_search\(\)\] k=0 must be at least 1"),
                            ((-3, 5), "k=-3 must be at least 1"),
                            ((6, 5), r"\[QuakeIndex::diverse_search\(\)\] fetch_k=5 must be at least k=6"),
                            ((1, 0), "fetch_k=0 must be at least k=1"),
                            ((10, 257), r"\[QuakeIndex::diverse_search\(\)\] fetch_k=257 must not exceed 256"),
                            ((300, 300), "fetch_k=300 must not exceed 256"),
                            ((2, 5, float("nan")), r"\[QuakeIndex::diverse_search\(\)\] lambda_mult is NaN"),
                            ((2, 5, -0.25), r"\[QuakeIndex::diverse_search\(\)\] lambda_mult=-0.25 must lie in \[0, 1\]"),
                            ((2, 5, 1.5), r"lambda_mult=1.5 must lie in \[0, 1\]"),
                            ((2, 5, float("inf")), r"lambda_mult=inf must lie in \[0, 1\]"),
                            ((2, 5, 1.0000001), r"must lie in \[0, 1\]"),
                            # several faults: k first, then fetch_k, then lambda
                            ((0, 500, 2.0), "k=0 must be at least 1"),
                            ((2, 1, 2.0), "fetch_k=1 must be at least k=2"),
                            ((2, 500, 2.0), "fetch_k=500 must not exceed 256")):
            with pytest.raises(RuntimeError, match=match):
                lower(*args)
    # the same message, character for character
    for args in ((0, 5), (6, 5), (10, 257), (2, 5, float("nan")), (2, 5, -0.25), (2, 5, 1e9), (2, 5, -1e-9), (2, 5, float("-inf"))):
        msgs = []
        for lower in mirrors:
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1], msgs
    # the Python mirror also says what is wrong with an argument of another type
    with pytest.raises(RuntimeError, match="integers"):
        mirrors[0](2.5, 5)
    with pytest.raises(RuntimeError, match="integers"):
        mirrors[0](2, "5")
    with pytest.raises(RuntimeError, match="lambda_mult must be a number"):
        mirrors[0](2, 5, "0.5")
    with pytest.raises(RuntimeError, match="lambda_mult must be a number"):
        mirrors[0](2, 5, None)


def test_refusals_without_a_device():
    """an index that was never built refuses in both mirrors before anything touches a device; sharded.py has no form"""
    import torch

    import quake_amd as quake
    import quake_amd.bindings as qb
    for mod in (quake, qb):
        idx = mod.QuakeIndex()
        sp = mod.SearchParams()
        sp.k = 5
        with pytest.raises(RuntimeError, match=r"\[QuakeIndex::diverse_search\(\)\] No query coordinator. Did you build the index\?"):
            idx.diverse_search(torch.zeros(2, 8), sp, 20)
        with pytest.raises(RuntimeError, match="No query coordinator"):
            idx.diverse_search(torch.zeros(2, 8), sp, fetch_k=20, lambda_mult=0.25)
        r = mod.DiverseSearchResult()
        for name in ("ids", "distances", "ranks", "timing_info"):
            assert hasattr(r, name), name
    from quake_amd.sharded import ShardedIndex
    with pytest.raises(RuntimeError, match=r"\[ShardedIndex::diverse_search\(\)\] diverse_search is not supported by sharded.py"):
        ShardedIndex(None).diverse_search(torch.zeros(2, 8), 4, 5, 20)


def test_abi_and_header_text():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    assert re.search(r"^#define\s+QK_MAX_FETCH_K\s+256\b", txt, re.M)
    from quake_amd import _lib, capi, where
    from quake_amd.build import SOURCES, build_lib
    assert "qk_diverse.hip" in SOURCES
    build_lib()
    lib = _lib.load()
    for name in ("qk_diverse_search", "qk_diverse_scan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"QK_API\s+int\s+%s\s*\(" % name, txt)
    # search has the parent and nprobe where scan has pids and P; the rest is the same list
    a, b = _lib.SIGNATURES["qk_diverse_search"][1], _lib.SIGNATURES["qk_diverse_scan"][1]
    assert len(a) == 16 and len(b) == 16 and a[6:] == b[6:]
    assert _lib.header_constant("QK_MAX_FETCH_K") == capi.QK_MAX_FETCH_K == where.QK_MAX_FETCH_K == 256
    assert _lib.header_constant("QK_MAX_FETCH_K") <= _lib.header_constant("QK_MAX_K")
    # the header states the limits and what answers a call outside them
    sec = txt[txt.index("---- diversified search"):txt.index("#define QK_MAX_FETCH_K")]
    sec = " ".join(sec.replace("*", " ").split())
    for phrase in ("1 <= k <= fetch_k <= QK_MAX_FETCH_K = 256", "k < 1 or fetch_k < k: QK_ERR_INVALID", "fetch_k > 256: QK_ERR_UNSUPPORTED",
                   "a lambda that is NaN or outside [0, 1]: QK_ERR_INVALID", "Q == 0: QK_OK", "d up to QK_MAX_D",
                   "ties, and the all-NaN case, go to the smaller rank", "three separately rounded float32 operations"):
        assert phrase in sec, phrase
    import quake_amd
    assert hasattr(capi.Context, "diverse_search") and hasattr(capi.Context, "diverse_scan")
    assert hasattr(quake_amd.QuakeIndex, "diverse_search") and hasattr(quake_amd, "DiverseSearchResult")
