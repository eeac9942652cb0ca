"""Binary search without a device: lower_bin in both mirrors (quake_amd/where.py; quake_amd/cpp, by the bindings), the entry points
declared, exported and bound, and the sharded refusal."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAD = [((40, 0, 64), "k=0 must be at least 1"), ((40, 10, 9), "fetch_k=9 must be at least k=10"), ((128, 449, 4096), "k=449 must not exceed 448"),
       ((128, 10, 4097), "fetch_k=4097 must not exceed 4096"), ((8193, 10, 4096), "d=8193 must not exceed 8192"),
       # several faults: k's limit before fetch_k's, d last
       ((9000, 449, 5000), "k=449 must not exceed 448"), ((9000, 5, 4097), "fetch_k=4097 must not exceed 4096")]


def _lowers():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as qb
    from quake_amd.where import lower_bin
    return lower_bin, qb.lower_bin


def test_lower_bin_and_the_mirrors():
    for lower in _lowers():
        assert tuple(lower(8192, 448, 4096)) == (448, 4096) and tuple(lower(d=1, k=1, fetch_k=1)) == (1, 1)
    for args, text in BAD:
        msgs = []
        for lower in _lowers():
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] == "[QuakeIndex::binary_search()] " + text, msgs


def test_entry_points_are_declared_exported_and_bound():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    from quake_amd.where import QK_BIN_MAX_FETCH
    build_lib()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    declared = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", header))
    for name, shipped in (("qk_bin_search", "qk_sq8_search"), ("qk_bin_scan", "qk_sq8_scan")):
        assert name in declared and hasattr(lib, name) and _lib.SIGNATURES[name] == _lib.SIGNATURES[shipped]
        assert getattr(lib, name)(*([None] * 3 + [None if t is not _lib.C.c_int and t is not _lib.C.c_int64 else 1 for t in _lib.SIGNATURES[name][1][3:]])) == 1
        assert name.encode() in lib.qk_last_error()
    for name in ("qk_store_bin_info", "qk_store_bin_drop"):
        assert name in declared and hasattr(lib, name)
        assert getattr(lib, name)(*([None] * len(_lib.SIGNATURES[name][1]))) == 1 and name.encode() in lib.qk_last_error()
    assert int(re.search(r"#define QK_BIN_MAX_FETCH (\d+)", header).group(1)) == QK_BIN_MAX_FETCH == 4096


def test_sharded_refuses_by_name():
    import torch

    from quake_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::binary_search\(\)\] binary_search is not supported by sharded.py"):
        ShardedIndex(None).binary_search(torch.zeros(2, 32), 4, 5, 2000)
