"""Per-query filters, the part that needs no GPU: the three entry points are declared, exported and bound, refuse a null context
with a message, and the limit of the header is the one the Python wrapper exposes."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("qk_search_filtered_batch", "qk_search_filtered_batch_tracked", "qk_scan_filtered_batch")


def _header():
    return open(os.path.join(ROOT, "include", "quake_hip.h")).read()


def _lib():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    return _lib, _lib.load()


def test_entry_points_are_declared_exported_and_bound():
    declared = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", _header()))
    mod, lib = _lib()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in mod.SIGNATURES, name
    # the single qk_filter * of the single-filter signature is replaced by (filters, F, qfilter): two arguments more
    for one, many in (("qk_search_filtered", "qk_search_filtered_batch"), ("qk_search_filtered_tracked", "qk_search_filtered_batch_tracked"),
                      ("qk_scan_filtered", "qk_scan_filtered_batch")):
        assert len(mod.SIGNATURES[many][1]) == len(mod.SIGNATURES[one][1]) + 2


def test_null_context_is_refused_with_a_message():
    mod, lib = _lib()
    filters = (C.c_void_p * 1)(None)
    nargs = {name: len(mod.SIGNATURES[name][1]) for name in ENTRY_POINTS}
    for name in ENTRY_POINTS:
        args = [None] * nargs[name]
        sig = mod.SIGNATURES[name][1]
        for i, t in enumerate(sig):
            if t in (C.c_int, C.c_int64):
                args[i] = 1
        args[[i for i, t in enumerate(sig) if t == C.POINTER(C.c_void_p)][0]] = filters
        assert getattr(lib, name)(*args) == 1, name  # QK_ERR_INVALID
        assert name.encode() in lib.qk_last_error(), name


def test_the_limit_of_the_header_is_the_wrappers():
    from quake_amd import capi
    m = re.search(r"#define\s+QK_MAX_BATCH_FILTERS\s+(\d+)", _header())
    assert m and int(m.group(1)) == capi.QK_MAX_BATCH_FILTERS == 4096
