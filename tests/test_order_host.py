"""Ordered search without a device: the argument normalisation of the mirrors (quake_amd/where.py: lower_order; quake_amd/cpp:
lower_order, exposed by the bindings) -- the same results and the same errors in both -- the refusals that need no device, and the
C ABI of qk_order_search / qk_order_scan as far as it can be checked without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirrors():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    from quake_amd.where import lower_order
    return lower_order, b.lower_order


def test_lower_order(mirrors):
    from quake_amd import where
    assert where.QK_MAX_ORDER_K == 1024 and (where.QK_ORDER_DESC, where.QK_ORDER_MISSING_LAST) == (1, 2)
    cols = ["price", "year"]
    for lower in mirrors:
        assert tuple(lower(cols, "price", 10)) == ("price", 10, 0)
        assert tuple(lower(cols, "year", 1, True)) == ("year", 1, 1)
        assert tuple(lower(cols, "year", 1024, False, "last")) == ("year", 1024, 2)
        assert tuple(lower(cols, "price", 7, True, "last")) == ("price", 7, 3)
        assert tuple(lower(cols, "price", 7, descending=True, missing="exclude")) == ("price", 7, 1)
        for args, match in ((("nope", 5), r"\[QuakeIndex::ordered_search\(\)\] unknown attribute column 'nope'"),
                            (("price", 0), r"\[QuakeIndex::ordered_search\(\)\] k=0 must be between 1 and 1024"),
                            (("price", -1), "k=-1 must be between 1 and 1024"),
                            (("price", 1025), "k=1025 must be between 1 and 1024"),
                            (("price", 5, False, "first"), r"\[QuakeIndex::ordered_search\(\)\] missing must be 'exclude' or 'last', got 'first'"),
                            (("price", 5, True, ""), "missing must be 'exclude' or 'last', got ''"),
                            # several faults: the column first, then k, then missing
                            (("nope", 0, False, "first"), "unknown attribute column 'nope'"),
                            (("price", 0, False, "first"), "k=0 must be"),
                            (("", 5), "unknown attribute column ''")):
            with pytest.raises(RuntimeError, match=match):
                lower(cols, *args)
        with pytest.raises(RuntimeError, match="unknown attribute column 'price'"):
            lower([], "price", 5)
    # the same message, character for character
    for args in (("nope", 5), ("price", 0), ("price", 5000), ("price", 5, False, "First")):
        msgs = []
        for lower in mirrors:
            with pytest.raises(RuntimeError) as ei:
                lower(cols, *args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1], msgs
    # the Python mirror also says what is wrong with a name or a k of another type
    with pytest.raises(RuntimeError, match="order_by must be the name"):
        mirrors[0](cols, ["price"], 5)
    with pytest.raises(RuntimeError, match="integers"):
        mirrors[0](cols, "price", 2.5)


def test_refusals_without_a_device():
    """an index that was never built refuses in both mirrors before anything touches a device"""
    import torch

    import quake_amd as quake
    import quake_amd.bindings as qb
    for mod in (quake, qb):
        idx = mod.QuakeIndex()
        sp = mod.SearchParams()
        sp.k = 5
        with pytest.raises(RuntimeError, match=r"\[QuakeIndex::ordered_search\(\)\] No query coordinator. Did you build the index\?"):
            idx.ordered_search(torch.zeros(2, 8), "price", sp)
        with pytest.raises(RuntimeError, match="No query coordinator"):
            idx.ordered_search(torch.zeros(2, 8), "price", sp, radius=1.0, descending=True, missing="last")
        r = mod.OrderedSearchResult()
        for name in ("ids", "distances", "values", "counts", "missing", "totals", "column", "timing_info"):
            assert hasattr(r, name), name


def test_abi():
    txt = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    assert re.search(r"^#define\s+QK_MAX_ORDER_K\s+1024\b", txt, re.M)
    assert re.search(r"^#define\s+QK_ORDER_DESC\s+1\b", txt, re.M) and re.search(r"^#define\s+QK_ORDER_MISSING_LAST\s+2\b", txt, re.M)
    from quake_amd import _lib, capi
    from quake_amd.build import SOURCES, build_lib
    assert "qk_order.hip" in SOURCES
    build_lib()
    lib = _lib.load()
    for name in ("qk_order_search", "qk_order_scan"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"QK_API\s+int\s+%s\s*\(" % name, txt)
    # search has the parent and nprobe where scan has pids and P; the rest is the same list
    a, b = _lib.SIGNATURES["qk_order_search"][1], _lib.SIGNATURES["qk_order_scan"][1]
    assert len(a) == 20 and len(b) == 20 and a[7:] == b[7:]
    assert _lib.header_constant("QK_MAX_ORDER_K") == capi.QK_MAX_ORDER_K == 1024
    assert (_lib.header_constant("QK_ORDER_DESC"), _lib.header_constant("QK_ORDER_MISSING_LAST")) == (capi.QK_ORDER_DESC, capi.QK_ORDER_MISSING_LAST)
    import quake_amd
    assert hasattr(capi.Context, "order_search") and hasattr(capi.Context, "order_scan")
    assert hasattr(quake_amd.QuakeIndex, "ordered_search") and hasattr(quake_amd, "OrderedSearchResult")
