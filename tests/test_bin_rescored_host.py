"""Rescored binary search without a device: lower_bin_rescored in both mirrors (quake_amd/where.py; quake_amd/cpp, by the bindings),
the entry points declared, exported and bound, and the sharded refusal."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (d, k, fetch_k, rescore_k): one fault each in the order of the checks, then several at once -- the earlier check speaks
BAD = [((40, 0, 64, 10), "k=0 must be at least 1"), ((40, 10, 9, 10), "fetch_k=9 must be at least k=10"),
       ((40, 10, 64, 9), "rescore_k=9 must be at least k=10"), ((40, 10, 64, 65), "rescore_k=65 must be at most fetch_k=64"),
       ((40, 449, 4096, 449), "k=449 must not exceed 448"), ((40, 10, 4096, 449), "rescore_k=449 must not exceed 448"),
       ((40, 10, 4097, 448), "fetch_k=4097 must not exceed 4096"), ((2049, 10, 4096, 448), "d=2049 must not exceed 2048"),
       ((9000, 10, 64, 65), "rescore_k=65 must be at most fetch_k=64"), ((9000, 449, 5000, 449), "k=449 must not exceed 448"),
       ((9000, 10, 5000, 449), "rescore_k=449 must not exceed 448"), ((9000, 10, 5000, 448), "fetch_k=5000 must not exceed 4096")]


def test_lower_bin_rescored_and_the_mirrors():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as qb
    from quake_amd.where import lower_bin_rescored
    lowers = (lower_bin_rescored, qb.lower_bin_rescored)
    for lower in lowers:
        assert tuple(lower(2048, 448, 4096, 448)) == (448, 4096, 448) and tuple(lower(d=1, k=1, fetch_k=1, rescore_k=1)) == (1, 1, 1)
    for args, text in BAD:
        msgs = []
        for lower in lowers:
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] == "[QuakeIndex::binary_search()] " + text, msgs


def test_entry_points_are_declared_exported_and_bound():
    from quake_amd import _lib
    from quake_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quake_hip.h")).read()
    declared = set(re.findall(r"QK_API\s+[\w\s\*]+?\b(qk_\w+)\s*\(", header))
    for name, shipped, at in (("qk_bin_search_rescored", "qk_bin_search", 8), ("qk_bin_scan_rescored", "qk_bin_scan", 8)):
        args = list(_lib.SIGNATURES[shipped][1])
        assert name in declared and hasattr(lib, name) and _lib.SIGNATURES[name] == (_lib.SIGNATURES[shipped][0], args[:at] + [_lib.C.c_int] + args[at:])
        assert getattr(lib, name)(*([None] * 3 + [None if t is not _lib.C.c_int and t is not _lib.C.c_int64 else 1 for t in _lib.SIGNATURES[name][1][3:]])) == 1
        assert name.encode() in lib.qk_last_error()


def test_sharded_refuses_by_name():
    import torch

    from quake_amd.sharded import ShardedIndex
    for kw in ({}, {"rescore_k": 100}):
        with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::binary_search\(\)\] binary_search is not supported by sharded.py"):
            ShardedIndex(None).binary_search(torch.zeros(2, 32), 4, 5, 2000, **kw)
