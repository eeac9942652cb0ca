"""The recall-target walk (qk_search_aps, quake_amd/csrc/qk_aps.hip) on the device where its first suite never goes, through
capi.Context.search_aps, against the oracle's walk: partitions visited, ids and float32 distance bits all equal.

The cases and the one comparison are tests/aps_yardstick.py's; tests/test_aps_walk_oracle.py pins, on the CPU, that they reach the
branches they are named after: every k_aps_update<MAXCH> (k up to QK_MAX_K, lists shorter than k), rounds of more than 64 steps and
the exit without a stop, a round's row shorter than the walk (CH < M, at least three rounds: asserted from the round count), a parent
with non-identity ids edited under a live context (the cached id -> row map), squared L2 output, the four non-finite classes
(DESIGN.md 5.8.1), a wide row at k > 64, the device group, and another length of the first round (a fresh process each).

(Named like test_range_search.py and test_nonfinite_search.py: a *_gpu.py file needs a stated place in conftest.collection_rank.  No
test here reads a clock: `n_items` of qk_timing is the number of rounds.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the child process of the last test starts without conftest.py)
    sys.path.insert(0, ROOT)

import aps_yardstick as AY  # noqa: E402
import nonfinite_yardstick as NF  # noqa: E402

pytestmark = pytest.mark.gpu


def _stores(ctx, co, centroid_ids=None):
    from quake_amd.capi import Store
    s = Store(ctx, co["d"])
    s.build_csr(co["offsets"], co["ids"], co["vecs"])
    parent = Store(ctx, co["d"])
    n = co["centroids"].shape[0]
    parent.build_csr(np.array([0, n], np.int64), np.arange(n, dtype=np.int64) if centroid_ids is None else centroid_ids, co["centroids"])
    return parent, s


class _Built:
    """the stores of the corpus used last (the cases of one corpus run side by side)"""

    def __init__(self, ctx):
        self.ctx, self.co, self.stores = ctx, None, None

    def get(self, c):
        co = AY.corpus(c)
        if self.co is not co:
            self.drop()
            self.stores, self.co = _stores(self.ctx, co), co
        return self.stores

    def drop(self):
        if self.stores:
            for st in self.stores:
                st.close()
        self.stores = self.co = None


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(ctx):
    b = _Built(ctx)
    yield b
    b.drop()


def _twice(ctx, built, c, **kw):
    """the case against the oracle, called twice (the form feedback takes its second form)"""
    parent, s = built.get(c)
    want = AY.expected(c)
    for call in range(2):
        got = AY.device_walk(ctx, parent, s, c, **kw)
        AY.assert_same(c, got, want, "call %d" % call)
    return got


# ---- a. k buckets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.K_BUCKETS, ids=AY.case_id)
def test_k_buckets(ctx, built, c):
    _twice(ctx, built, c)


def test_k_beyond_the_pools_is_refused(ctx, built):
    from quake_amd._lib import STATUS_NAMES, QuakeHipError
    c = dict(AY.K_BUCKETS[0], k=AY.QK_MAX_K + 1)
    parent, s = built.get(c)
    with pytest.raises(QuakeHipError) as e:
        AY.device_walk(ctx, parent, s, c)
    assert STATUS_NAMES[e.value.status] == "QK_ERR_UNSUPPORTED"
    _twice(ctx, built, dict(c, k=AY.QK_MAX_K))   # (and the context still answers)


# ---- b. rounds of more than 64 steps, the exit without a stop ----------------------------------------------------------------
@pytest.mark.parametrize("c", AY.LONG_ROUNDS, ids=AY.case_id)
def test_long_rounds(ctx, built, c):
    gi, gd, gn = _twice(ctx, built, c)
    if c["target"] > 1.0:
        assert (gn == AY.M_of(c)).all()


# ---- c. a round shorter than the walk -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.CAPPED, ids=AY.case_id)
def test_capped_rounds(ctx, built, c):
    import torch
    parent, s = built.get(c)
    want = AY.expected(c)
    gi, gd, gn, tm = AY.device_walk(ctx, parent, s, c, timing=True)
    AY.assert_same(c, (gi, gd, gn), want, "host arrays")
    assert tm["n_items"] >= 3, tm   # rounds: the first, a full one of CH lists, and what is left
    qd = torch.from_numpy(AY.corpus(c)["q"].copy()).cuda()
    di, dd, dn, tm = AY.device_walk(ctx, parent, s, c, q=qd, timing=True)
    ctx.synchronize()
    AY.assert_same(c, (di, dd, dn), want, "device tensors")
    assert tm["n_items"] >= 3, tm


# ---- d. the parent changes under a live context ---------------------------------------------------------------------------------
def test_parent_changes_under_a_live_context(ctx):
    from quake_amd.capi import Store
    c = AY.PARENT_CASE
    steps = AY.parent_steps()
    first = steps[0]
    parent, s = _stores(ctx, first, first["centroid_ids"])
    parent2 = None
    try:
        for st in steps:
            if "replaced" in st:
                p, vec, ids, rows = st["replaced"]
                assert parent.remove_ids([p]) == 1
                parent.add_entries(0, np.array([p], np.int64), vec[None, :])
                s.remove_list(p)
                s.add_list(p)
                s.add_entries(p, ids, rows)
            if "removed" in st:
                h = st["removed"]
                s.remove_list(h)
                assert parent.remove_ids([h]) == 1
                assert s.nlist() == st["nlist_present"] and parent.ntotal() == st["nlist_present"]
            if st.get("second"):
                parent2 = Store(ctx, c["d"])
                n = st["centroids"].shape[0]
                parent2.build_csr(np.array([0, n], np.int64), st["centroid_ids"], st["centroids"])
            use = parent2 if st.get("second") else parent
            want = AY.step_walk(st)
            for call in range(2):
                got = AY.device_walk(ctx, use, s, c, q=st["q"])
                AY.assert_same(c, got, want, "%s, call %d" % (st["name"], call))
    finally:
        for x in (parent, parent2, s):
            if x is not None:
                x.close()


# ---- e. squared L2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.SQUARED, ids=AY.case_id)
def test_squared_l2(ctx, built, c):
    parent, s = built.get(c)
    oi, od, on = AY.expected(c)
    ctx.set_squared_l2(True)
    try:
        for call in range(2):
            gi, gd, gn = AY.device_walk(ctx, parent, s, c)
            assert gd.dtype == np.float32
            AY.assert_same(c, (gi, np.sqrt(gd), gn), (oi, od, on), "squared, call %d" % call)   # sqrtf is correctly rounded on both sides
    finally:
        ctx.set_squared_l2(False)
    _twice(ctx, built, c)


# ---- f. non-finite values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.NONFINITE, ids=AY.case_id)
def test_nonfinite(ctx, built, c):
    co = AY.corpus(c)
    gi, gd, gn = _twice(ctx, built, c)
    NF.assert_no_nan_pair(co, co["q"], co["special_q"], gi)


# ---- g. one wide row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.WIDE, ids=AY.case_id)
def test_wide_row(ctx, built, c):
    _twice(ctx, built, c)
    built.drop()


# ---- h. the device group --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", AY.GROUP, ids=AY.case_id)
def test_group_equals_single_store(ctx, built, c):
    from quake_amd.capi import Group
    co = AY.corpus(c)
    parent, s = built.get(c)
    single = AY.device_walk(ctx, parent, s, c)
    AY.assert_same(c, single, AY.expected(c), "single store")
    grp = Group([0, 0, 0], c["d"])
    try:
        grp.build_csr(co["offsets"], co["ids"], co["vecs"])
        for call in range(2):
            got = AY.device_walk(grp, parent, None, c)
            AY.assert_same(c, got, single, "group, call %d" % call)
    finally:
        grp.close()


# ---- i. the first round's length ------------------------------------------------------------------------------------------------
def test_first_round_length_changes_no_result():
    """QK_APS_FIRST is read once per process: a fresh child for each length, one after the other, none after a failure"""
    for first in AY.FIRST_ROUND_LENGTHS:
        env = dict(os.environ, QK_APS_FIRST=str(first))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "first-round"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, "QK_APS_FIRST=%d: exit %d\n%s\n%s" % (first, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        assert "APS-FIRST-ROUND-OK %d" % first in r.stdout


def _first_round_child():
    """compares every case of AY.FIRST_ROUND with the oracle under this process's QK_APS_FIRST; any mismatch raises (exit status 1)"""
    from quake_amd.capi import Context
    ctx = Context(0)
    built = _Built(ctx)
    for c in AY.FIRST_ROUND:
        _twice(ctx, built, c)
    built.drop()
    ctx.close()
    print("APS-FIRST-ROUND-OK %d" % int(os.environ["QK_APS_FIRST"]))


if __name__ == "__main__":
    assert sys.argv[1:] == ["first-round"]
    _first_round_child()
