"""Deep quantized search without a device: lower_sq8(deep=True) in both mirrors (quake_amd/where.py; quake_amd/cpp, by the bindings),
the default path as it was, the entry points declared, exported and bound, and the sharded refusal."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEEP = [((40, 0, 64), "k=0 must be at least 1"), ((40, 10, 9), "fetch_k=9 must be at least k=10"), ((128, 449, 4096), "k=449 must not exceed 448"),
        ((128, 10, 4097), "fetch_k=4097 must not exceed 4096"), ((2112, 10, 4096), "d=2112 must not exceed 2048"),
        # several faults: k's limit before fetch_k's, d last
        ((4096, 449, 5000), "k=449 must not exceed 448"), ((4096, 5, 4097), "fetch_k=4097 must not exceed 4096")]


def _lowers():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as qb
    from quake_amd.where import lower_sq8
    return lower_sq8, qb.lower_sq8


def test_lower_sq8_deep_and_the_mirrors():
    for lower in _lowers():
        assert tuple(lower(2048, 448, 4096, deep=True)) == (448, 4096) and tuple(lower(d=40, k=1, fetch_k=1, deep=True)) == (1, 1)
        assert tuple(lower(64, 10, 449, deep=True)) == (10, 449)
    for args, text in DEEP:
        msgs = []
        for lower in _lowers():
            with pytest.raises(RuntimeError) as ei:
                lower(*args, deep=True)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] and text in msgs[0] and msgs[0].startswith("[QuakeIndex::quantized_search()]"), msgs


def test_the_default_path_is_unchanged():
    for lower in _lowers():
        assert tuple(lower(2048, 448, 448)) == (448, 448)
        for kw in ({}, {"deep": False}):
            with pytest.raises(RuntimeError) as ei:
                lower(128, 10, 449, **kw)
            assert str(ei.value) == "[QuakeIndex::quantized_search()] fetch_k=449 must not exceed 448"


def test_entry_points_are_declared_exported_and_bound():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    from quake_amd.where import QK_SQ8_MAX_FETCH
    build_lib()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    declared = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", header))
    for deep, shipped in (("qk_sq8_search_deep", "qk_sq8_search"), ("qk_sq8_scan_deep", "qk_sq8_scan")):
        assert deep in declared and hasattr(lib, deep) and _lib.SIGNATURES[deep] == _lib.SIGNATURES[shipped]
        assert getattr(lib, deep)(*([None] * 3 + [None if t is not _lib.C.c_int and t is not _lib.C.c_int64 else 1 for t in _lib.SIGNATURES[deep][1][3:]])) == 1
        assert deep.encode() in lib.qk_last_error()
    assert int(re.search(r"#define QK_SQ8_MAX_FETCH (\d+)", header).group(1)) == QK_SQ8_MAX_FETCH == 4096


def test_sharded_refuses_by_name():
    import torch

    from quake_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::quantized_search\(\)\] quantized_search is not supported by sharded.py"):
        ShardedIndex(None).quantized_search(torch.zeros(2, 32), 4, 5, 2000, deep=True)
