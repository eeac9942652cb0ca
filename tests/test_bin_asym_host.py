"""Asymmetric binary search without a device: the entry points declared, exported and bound, and their null-argument refusals by
name."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    declared = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", header))
    integers = (_lib.C.c_int, _lib.C.c_int64)
    # the arguments are the rescored calls': rescore_k behind fetch_k
    for name, same_as in (("qk_bin_search_asym", "qk_bin_search_rescored"), ("qk_bin_scan_asym", "qk_bin_scan_rescored")):
        assert name in declared and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[same_as]
        # every pointer null, every integer 1: refused as invalid (1), and the message names the entry point
        args = [1 if t in integers else None for t in _lib.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == 1
        assert name.encode() in lib.qk_last_error()
    name = "qk_store_bin_asym_info"
    assert name in declared and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == 3
    assert lib.qk_store_bin_asym_info(None, None, None) == 1
    assert name.encode() in lib.qk_last_error()
