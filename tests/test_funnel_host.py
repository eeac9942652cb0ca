"""Funnel search without a device: lower_funnel's checks in both mirrors (quake_amd/where.py; quake_amd/cpp, exposed by the
bindings) and both mirrors exposing funnel_search with the same signature."""
import pytest


@pytest.fixture(scope="module")
def mirrors():
    from quake_amd.build_ext import build_bindings
    build_bindings()
    import quake_amd.bindings as b
    from quake_amd.where import lower_funnel
    return lower_funnel, b.lower_funnel


CASES = [((48, 10, 8, 64), "prefix_dim=8 must lie in [16, d=48] and be a multiple of 16 or equal to d"),
         ((48, 10, 24, 64), "prefix_dim=24 must lie"), ((48, 10, 64, 64), "prefix_dim=64 must lie"),
         ((40, 0, 16, 64), "k=0 must be at least 1"), ((40, 10, 16, 9), "fetch_k=9 must be at least k=10"),
         ((4096, 10, 1040, 64), "prefix_dim=1040 must not exceed 1024"), ((128, 10, 32, 449), "fetch_k=449 must not exceed 448"),
         # several faults: prefix_dim first, then k, fetch_k, and the limits last
         ((48, 0, 8, 500), "prefix_dim=8 must lie"), ((4096, 5, 2048, 4), "fetch_k=4 must be at least k=5")]


def test_lower_funnel(mirrors):
    for lower in mirrors:
        assert tuple(lower(48, 10, 16, 64)) == (10, 16, 64)
        assert tuple(lower(40, 1, 40, 1)) == (1, 40, 1)          # d itself, whatever its remainder
        assert tuple(lower(d=4096, k=448, prefix_dim=1024, fetch_k=448)) == (448, 1024, 448)
    for args, text in CASES:
        msgs = []
        for lower in mirrors:
            with pytest.raises(RuntimeError) as ei:
                lower(*args)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1] and text in msgs[0] and msgs[0].startswith("[QuakeIndex::funnel_search()]"), msgs
    with pytest.raises(RuntimeError, match="integers"):
        mirrors[0](48, 2.5, 16, 64)


def test_both_mirrors_expose_funnel_search():
    import torch

    import quake_amd as quake
    import quake_amd.bindings as qb
    for mod in (quake, qb):
        idx, sp = mod.QuakeIndex(), mod.SearchParams()
        sp.k = 5
        with pytest.raises(RuntimeError, match=r"\[QuakeIndex::funnel_search\(\)\] No query coordinator. Did you build the index\?"):
            idx.funnel_search(torch.zeros(2, 32), sp, prefix_dim=16, fetch_k=20)
        with pytest.raises(RuntimeError, match="No query coordinator"):
            idx.funnel_search(torch.zeros(2, 32), sp, 16, 20)
    from quake_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match=r"\[ShardedIndex::funnel_search\(\)\] funnel_search is not supported by sharded.py"):
        ShardedIndex(None).funnel_search(torch.zeros(2, 32), 4, 5, 16, 20)
