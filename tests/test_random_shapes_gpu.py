"""Seeded sweep over shapes nobody picked by hand: dimension (1 ... 200, multiples of 16 and not), number of lists, skewed list
sizes with empty lists and lists shorter than k, batch sizes on both sides of every dispatch boundary (one-launch search up
to 32 queries; single-workgroup grouping up to 1024 pairs; row-per-lane / 16x16 / query-sharing scan forms), nprobe up to
and beyond the number of lists, k from 1 to 100, both metrics, SIFT-like integer data (dense ties).  Every case: qk_search
ids and float32 distance bits equal the oracle's canonical batched search; the same batch again as qk_coarse + qk_scan.
The same shapes (and four seam shapes, d = 256 ... 3000) through the entry points on the filtered tile form -- filtered, per-query, predicate,
adaptive, range, grouped with members, paged -- interleaved on one context, before and after the store is mutated: the second half
of this file, cases in tests/random_features.py."""
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


def _case(rng):
    d = int(rng.choice([1, 3, 16, 17, 31, 32, 48, 64, 100, 128, 129, 200]))
    nlist = int(rng.choice([1, 2, 5, 17, 64, 150, 300]))
    metric = str(rng.choice(["l2", "ip"]))
    integer = bool(rng.random() < 0.3)
    n = int(rng.choice([nlist, 200, 3000, 20000]))
    # skewed sizes: a few big lists, many small, some empty
    w = rng.random(nlist) ** 3
    w[rng.random(nlist) < 0.15] = 0.0
    if w.sum() == 0:
        w[0] = 1.0
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    if integer:
        cent = rng.integers(0, 30, size=(nlist, d)).astype(np.float32)
        x = cent[assign] + rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    else:
        cent = rng.standard_normal((nlist, d)).astype(np.float32)
        x = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip" and not integer:
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-6)
    ids = rng.permutation(n).astype(np.int64) + int(rng.integers(0, 1000))
    order = np.argsort(assign, kind="stable")
    vecs, aids = np.ascontiguousarray(x[order]), np.ascontiguousarray(ids[order])
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    Q = int(rng.choice([1, 2, 7, 16, 32, 33, 64, 100, 257, 1030]))
    nprobe = int(rng.choice([1, 2, 3, 8, 16, 40, 64, 100]))
    k = int(rng.choice([1, 5, 10, 32, 33, 100]))
    q = (x[rng.integers(0, n, size=Q)] + (0 if integer else 0.05) * rng.standard_normal((Q, d))).astype(np.float32)
    return dict(d=d, nlist=nlist, metric=metric, integer=integer, n=n, cent=cent, vecs=vecs, ids=aids, offsets=offsets, Q=Q,
                nprobe=nprobe, k=k, q=q)


# (a one-off run of 1000 seeds found one failure -- seed 107: d = 128, k = 32, nprobe 100: the row-per-lane form asked for more
#  LDS than a CU has -- and passes since; 107 stays in the default set)
@pytest.mark.parametrize("seed", sorted(set(range(int(os.environ.get("QK_RANDOM_SHAPES", "48")))) | {107}))
def test_random_shape_search_bit_exact(seed):
    from quake_amd.capi import Context, Store
    rng = np.random.default_rng(1000 + seed)
    c = _case(rng)
    ctx = Context(0)
    try:
        s = Store(ctx, c["d"])
        s.build_csr(c["offsets"], c["ids"], c["vecs"])
        parent = Store(ctx, c["d"])
        parent.build_csr(np.array([0, c["nlist"]], np.int64), np.arange(c["nlist"], dtype=np.int64), c["cent"])
        tag = {kk: c[kk] for kk in ("d", "nlist", "metric", "integer", "n", "Q", "nprobe", "k")}
        oi, od = O.search(c["q"], c["cent"], c["vecs"], c["ids"], c["offsets"], c["nprobe"], c["k"], c["metric"], batched_scan=True)
        for rep in range(2):  # twice: per-context state left by the first call (tickets, counters, cleared regions)
            gi, gd = ctx.search(parent, s, c["q"], c["nprobe"], c["k"], c["metric"])
            np.testing.assert_array_equal(gi, oi, err_msg=f"{tag} form={ctx.last_scan_kernel()} rep={rep}")
            np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32), err_msg=str(tag))
        # the two-call form: coarse, then scan of the returned lists
        pids, _ = ctx.coarse(parent, c["q"], c["nprobe"], c["metric"])
        op, _ = O.coarse(c["q"], c["cent"], None, c["nprobe"], c["metric"])
        np.testing.assert_array_equal(pids[:, :op.shape[1]], op, err_msg=str(tag))
        gi, gd = ctx.scan(s, c["q"], pids, c["k"], c["metric"])
        np.testing.assert_array_equal(gi, oi, err_msg=f"{tag} (coarse + scan) form={ctx.last_scan_kernel()}")
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32))
        if seed % 3 == 0:  # the same batch handed over in device memory (no staging, results written in place)
            import torch
            ti, td = ctx.search(parent, s, torch.from_numpy(c["q"]).cuda(), c["nprobe"], c["k"], c["metric"])
            ctx.synchronize()
            np.testing.assert_array_equal(ti.cpu().numpy(), oi, err_msg=f"{tag} (device buffers)")
            np.testing.assert_array_equal(td.cpu().numpy().view(np.uint32), od.view(np.uint32))
        # no parent: every list is scanned (query_coordinator.cpp:624-626)
        if c["Q"] * c["nlist"] <= 40000:
            fi, fd = ctx.search(None, s, c["q"], 1, c["k"], c["metric"])
            allp = np.broadcast_to(np.arange(c["nlist"], dtype=np.int64), (c["Q"], c["nlist"])).copy()
            ei, ed = O.batched_serial_scan(c["q"], c["vecs"], c["ids"], c["offsets"], allp, c["k"], c["metric"])
            np.testing.assert_array_equal(fi, ei, err_msg=f"{tag} (flat) form={ctx.last_scan_kernel()}")
            np.testing.assert_array_equal(fd.view(np.uint32), ed.view(np.uint32))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(10)))
def test_random_shape_wide_k_and_nprobe(seed):
    """the wide ends: k beyond the LDS pools (key emission + bisection select) and nprobe in the hundreds / thousands"""
    from quake_amd.capi import Context, Store
    rng = np.random.default_rng(5000 + seed)
    d = int(rng.choice([8, 24, 40]))
    nlist = int(rng.choice([600, 2500]))
    n = 30000
    metric = str(rng.choice(["l2", "ip"]))
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = rng.integers(0, nlist, size=n)
    x = (cent[assign] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    order = np.argsort(assign, kind="stable")
    vecs, aids = np.ascontiguousarray(x[order]), np.ascontiguousarray(ids[order])
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    Q = int(rng.choice([3, 40]))
    nprobe = int(rng.choice([100, 500, 2000]))
    k = int(rng.choice([100, 449, 1000, 5000]))
    q = (x[rng.integers(0, n, size=Q)] + 0.05 * rng.standard_normal((Q, d))).astype(np.float32)
    ctx = Context(0)
    try:
        s = Store(ctx, d)
        s.build_csr(offsets, aids, vecs)
        parent = Store(ctx, d)
        parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
        oi, od = O.search(q, cent, vecs, aids, offsets, nprobe, k, metric, batched_scan=True)
        gi, gd = ctx.search(parent, s, q, nprobe, k, metric)
        tag = dict(d=d, nlist=nlist, metric=metric, Q=Q, nprobe=nprobe, k=k)
        np.testing.assert_array_equal(gi, oi, err_msg=str(tag))
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32), err_msg=str(tag))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_shape_kmeans_bit_exact(seed):
    """k-means driver (subsample or not, empty-cluster splits when m is close to n) and the refine of a store, random shapes"""
    from quake_amd.capi import Context
    rng = np.random.default_rng(7000 + seed)
    d = int(rng.choice([2, 17, 32, 100, 128, 160]))
    m = int(rng.choice([1, 2, 7, 33, 200]))
    n = int(rng.choice([max(m, 50), 2000, 30000]))
    metric = str(rng.choice(["l2", "ip"]))
    x = (rng.standard_normal((max(m // 4, 1), d)).astype(np.float32)[rng.integers(0, max(m // 4, 1), n)]
         + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    ctx = Context(0)
    try:
        tag = dict(d=d, m=m, n=n, metric=metric)
        gc, ga, gx = ctx.kmeans(x.copy(), m, metric, niter=3, seed=99 + seed)
        oc, oa, ox = O.kmeans(x, m, metric, niter=3, seed=99 + seed)
        np.testing.assert_array_equal(np.asarray(gc).view(np.uint32), oc.view(np.uint32), err_msg=str(tag))
        np.testing.assert_array_equal(np.asarray(ga), oa, err_msg=str(tag))
        np.testing.assert_array_equal(np.asarray(gx).view(np.uint32), ox.view(np.uint32), err_msg=str(tag))
        a, v = ctx.kmeans_assign(x, oc, metric)
        ra, rv = O.kmeans_assign(x, oc, metric)
        np.testing.assert_array_equal(np.asarray(a), ra, err_msg=str(tag))
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("QK_RANDOM_APS", "16")))))
def test_random_shape_aps_bit_exact(seed):
    """recall-target search on random shapes: ids, distance bits AND the number of partitions each query visited equal the
    oracle's walk"""
    from quake_amd.capi import Context, Store
    rng = np.random.default_rng(9000 + seed)
    d = int(rng.choice([8, 33, 64, 128]))
    nlist = int(rng.choice([8, 40, 200]))
    n = int(rng.choice([2000, 30000]))
    metric = str(rng.choice(["l2", "ip"]))
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    w = rng.random(nlist) ** 2 + 1e-3
    assign = rng.choice(nlist, size=n, p=w / w.sum())
    x = (cent[assign] + 0.6 * rng.standard_normal((n, d))).astype(np.float32)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ids = rng.permutation(n).astype(np.int64)
    order = np.argsort(assign, kind="stable")
    vecs, aids = np.ascontiguousarray(x[order]), np.ascontiguousarray(ids[order])
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    Q = int(rng.choice([1, 9, 70, 300]))
    q = (x[rng.integers(0, n, size=Q)] + 0.1 * rng.standard_normal((Q, d))).astype(np.float32)
    k = int(rng.choice([1, 10, 60]))
    rt = float(rng.choice([0.5, 0.8, 0.9, 0.99]))
    frac = float(rng.choice([0.3, 0.6, 1.0]))
    thr = float(rng.choice([0.0, 0.001, 0.05]))
    pre = bool(rng.random() < 0.5)
    if int(nlist * frac) < 2:
        frac = 1.0
    ctx = Context(0)
    try:
        s = Store(ctx, d)
        s.build_csr(offsets, aids, vecs)
        parent = Store(ctx, d)
        parent.build_csr(np.array([0, nlist], np.int64), np.arange(nlist, dtype=np.int64), cent)
        tag = dict(d=d, nlist=nlist, n=n, metric=metric, Q=Q, k=k, rt=rt, frac=frac, thr=thr, pre=pre)
        gi, gd, gn = ctx.search_aps(parent, s, q, k, metric, rt, recompute_threshold=thr, use_precomputed=pre, initial_search_fraction=frac)
        oi, od, on = O.search_aps(q, cent, vecs, aids, offsets, k, metric, rt, recompute_threshold=thr, use_precomputed=pre,
                                  initial_search_fraction=frac, expanded=True, num_threads=8)
        np.testing.assert_array_equal(gn, on, err_msg=str(tag))
        np.testing.assert_array_equal(gi, oi, err_msg=str(tag))
        np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32), err_msg=str(tag))
    finally:
        ctx.close()


# ---- the entry points on the filtered tile form: filtered, per-query, predicate, adaptive, range, grouped with members, paged ----------
# Cases and expected values: tests/random_features.py (the yardsticks of those entry points' own test files, the oracle under them);
# tests/test_random_features_oracle.py pins on the CPU what the seed set reaches.  One context, one store and one parent per test; the
# legs run interleaved on them in an order the seed shuffles, each leg twice in a row; every comparison is exact.
import nonfinite_yardstick as NF
import paging_yardstick as PY
import random_features as RF


def _same_rows(gi, gd, oi, od, msg):
    """ids and the uint32 view of the distances; a non-finite distance of a returned row: NF.assert_same_answer (signed zeros)"""
    gi, gd, od = np.asarray(gi), np.asarray(gd, np.float32), np.asarray(od, np.float32)
    if (~np.isfinite(od) & (np.asarray(oi) >= 0)).any():
        try:
            NF.assert_same_answer(gi, gd, oi, od)
        except AssertionError as ex:
            raise AssertionError(msg) from ex
        return
    np.testing.assert_array_equal(gi, oi, err_msg="ids " + msg)
    np.testing.assert_array_equal(gd.view(np.uint32), od.view(np.uint32), err_msg="dist " + msg)


class _Rig:
    """the context, the store, the parent, the filters and the columns of one case, and the legs over them"""

    def __init__(self, c):
        from quake_amd.capi import Attr, Context, Filter, Store
        self.c, self.f = c, c["f"]
        self.tag = RF.shape_tag(c)
        self.ctx = Context(0)
        self.s = Store(self.ctx, c["d"])
        self.s.build_csr(c["offsets"], c["ids"], c["vecs"])
        self.parent = Store(self.ctx, c["d"])
        self.parent.build_csr(np.array([0, c["nlist"]], np.int64), np.arange(c["nlist"], dtype=np.int64), c["cent"])
        self.filters = [Filter(self.s, S, mode) for S, mode in self.f["sets"]]
        self.attrs = {}
        for name, (ai, av) in self.f["cols"].items():
            self.attrs[name] = Attr(self.s)
            self.attrs[name].set(ai, av)
        name, op, a, b = self.f["where"]
        self.where = Filter.where(self.s, [(self.attrs[name], op, a, b)])
        self.table = self.filters + [self.where]
        self.refused = RF.refused_legs(c)
        self.skipped = {leg: 0 for leg in RF.LEGS}
        self.page0 = {}
        self.absent = set()   # lists remove_list took out of the store
        self.xd = None

    def close(self):
        for h in self.table + list(self.attrs.values()) + [self.s, self.parent]:
            h.close()
        self.ctx.close()

    def host(self, a):
        if type(a).__module__.startswith("torch"):
            self.ctx.synchronize()  # (the context's own stream: torch does not wait for it)
            return a.cpu().numpy()
        return np.asarray(a)

    def absent_mask(self, pids):
        gone = np.isin(self.host(pids), sorted(self.absent))
        if type(pids).__module__.startswith("torch"):
            import torch
            return torch.from_numpy(gone).to(pids.device)
        return gone

    def msg(self, leg, dev, rep, what=""):
        return f"{self.tag} leg={leg} {what} device={dev} rep={rep} form={self.ctx.last_scan_kernel()}"

    def rows(self, got, want, m):
        _same_rows(self.host(got[0]), self.host(got[1]), want[0], want[1], m)

    def run(self, e, device):
        """every leg, in the case's order, each twice in a row; device: the same again with queries and cursors in device memory"""
        for leg in self.f["leg_order"]:
            if leg in self.refused:
                self.skipped[leg] += 1
                continue
            for dev in ((False, True) if device else (False,)):
                if dev and self.xd is None:
                    import torch
                    self.xd = torch.from_numpy(self.c["q"]).cuda()
                for rep in range(2):
                    getattr(self, "leg_" + leg)(e, self.xd if dev else self.c["q"], dev, rep)

    # ---- the legs ----
    def leg_filtered(self, e, x, dev, rep):
        c, ctx = self.c, self.ctx
        got = ctx.search(self.parent, self.s, x, c["nprobe"], c["k"], c["metric"], filter=self.filters[0])
        self.rows(got, e["filtered"], self.msg("filtered", dev, rep, "search"))
        pids, _ = ctx.coarse(self.parent, x, c["nprobe"], c["metric"])
        np.testing.assert_array_equal(self.host(pids)[:, :e["coarse"].shape[1]], e["coarse"], err_msg=self.msg("filtered", dev, rep, "coarse"))
        if self.absent:  # qk_scan refuses a list the store no longer has (QK_ERR_NOT_FOUND, as the reference does); -1 is skipped
            pids[self.absent_mask(pids)] = -1
        got = ctx.scan(self.s, x, pids, c["k"], c["metric"], filter=self.filters[0])
        self.rows(got, e["filtered"], self.msg("filtered", dev, rep, "coarse + scan"))

    def leg_batch(self, e, x, dev, rep):
        c = self.c
        got = self.ctx.search(self.parent, self.s, x, c["nprobe"], c["k"], c["metric"], filters=self.table, query_filter=self.f["query_filter"])
        self.rows(got, e["batch"], self.msg("batch", dev, rep))

    def leg_where(self, e, x, dev, rep):
        c = self.c
        got = self.ctx.search(self.parent, self.s, x, c["nprobe"], c["k"], c["metric"], filter=self.where)
        self.rows(got, e["where"], self.msg("where", dev, rep))

    def leg_adaptive(self, e, x, dev, rep):
        c, f = self.c, self.f
        for name, kw in (("adaptive", dict(filter=self.filters[0])), ("adaptive_table", dict(filters=self.table, query_filter=f["query_filter"]))):
            got = self.ctx.search_adaptive(self.parent, self.s, x, c["nprobe"], f["max_nprobe"], c["k"], c["metric"],
                                           min_candidates=f["min_candidates"], **kw)
            m = self.msg("adaptive", dev, rep, name)
            np.testing.assert_array_equal(self.host(got[2]), e[name][2], err_msg="nprobed " + m)
            np.testing.assert_array_equal(self.host(got[3]), e[name][3], err_msg="probed " + m)
            self.rows(got, e[name], m)

    def leg_range(self, e, x, dev, rep):
        c = self.c
        for name, flt in (("range", None), ("range_filtered", self.filters[0])):
            got = self.ctx.range_search(self.parent, self.s, x, c["nprobe"], self.f["radius"], c["metric"], filter=flt, cap=None)
            m = self.msg("range", dev, rep, name)
            np.testing.assert_array_equal(self.host(got[0]), e[name][0], err_msg="lims " + m)
            _same_rows(self.host(got[1]), self.host(got[2]), e[name][1], e[name][2], m)   # (scan order)

    def leg_grouped(self, e, x, dev, rep):
        c = self.c
        x1 = x[:RF.ONE_AT_A_TIME]
        for name, flt in (("grouped", None), ("grouped_filtered", self.filters[0])):
            got = self.ctx.search_grouped(self.parent, self.s, x1, c["nprobe"], c["k"], c["metric"], self.attrs[self.f["group_by"]], filter=flt,
                                          group_size=self.f["m"])
            m = self.msg("grouped", dev, rep, name)
            self.rows(got, e[name], m)
            np.testing.assert_array_equal(self.host(got[2]), e[name][2], err_msg="groups " + m)

    def leg_pages(self, e, x, dev, rep):
        c, ctx = self.c, self.ctx
        for name, flt in (("pages", None), ("pages_filtered", self.filters[0])):
            want = e[name]
            after = None
            for p in range(RF.PAGES):  # chained from NULL cursors, every page resumed from the cursors the call itself returned
                got = ctx.search_after(self.parent, self.s, x, c["nprobe"], c["k"], c["metric"], after=after, filter=flt)
                m = self.msg("pages", dev, rep, f"{name} page {p}")
                self.rows(got, want["pages"][p], m)
                after = got[2]
                nk, ni = self.host(after[0]), self.host(after[1])
                assert PY.cursor_list(nk, ni) == want["cursors"][p], "cursors " + m
                if p == 0:
                    self.page0[name] = (nk.copy(), ni.copy(), self.host(got[0]).copy())
            # one batch at mixed depths: query i resumes behind page i mod PAGES
            mixed = [want["cursors"][i % RF.PAGES][i] for i in range(c["Q"])]
            got = ctx.search_after(self.parent, self.s, x, c["nprobe"], c["k"], c["metric"], after=PY.cursor_arrays(mixed), filter=flt)
            m = self.msg("pages", dev, rep, name + " mixed depths")
            pick = np.arange(c["Q"]) % RF.PAGES + 1
            wi = np.stack([want["pages"][pick[i]][0][i] for i in range(c["Q"])])
            wd = np.stack([want["pages"][pick[i]][1][i] for i in range(c["Q"])])
            self.rows(got, (wi, wd), m)
            assert PY.cursor_list(self.host(got[2][0]), self.host(got[2][1])) == [want["cursors"][pick[i]][i] for i in range(c["Q"])], "cursors " + m

    # ---- the store changes under the live context, filters and columns ----
    def mutate(self, seed):
        """add_batch (a short list outgrows its extent), remove_ids (allowed and denied ids, an unknown one), remove_list, refine_lists
        over three lists, Attr.set / unset -- on the store and on a numpy model beside it.  Returns the CSR the store now holds, rows in
        the order get_list reports (every list's content first asserted equal to the model's as a set of (id, vector bits)), and the
        columns"""
        c, s = self.c, self.s
        rng = np.random.default_rng(55000 + seed)
        nlist, d, metric = c["nlist"], c["d"], c["metric"]
        lists = np.repeat(np.arange(nlist, dtype=np.int64), np.diff(c["offsets"]))
        vecs, ids = c["vecs"].copy(), c["ids"].copy()
        present = set(range(nlist))
        cols = {name: RF.column_dict(col) for name, col in self.f["cols"].items()}

        def draw(assign):
            if c["integer"]:
                return (c["cent"][assign] + rng.integers(-2, 3, size=(assign.shape[0], d))).astype(np.float32)
            v = (c["cent"][assign] + 0.5 * rng.standard_normal((assign.shape[0], d))).astype(np.float32)
            if metric == "ip":
                v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-6)
            return v

        # 1. add_batch: a short list that is not the arena's last extent takes more rows than its extent has room for
        sizes = np.bincount(lists, minlength=nlist)
        nonempty = np.nonzero(sizes > 0)[0]
        inner = nonempty[:-1]
        target = int(inner[np.argmin(sizes[inner])]) if inner.shape[0] else int(nonempty[0])
        assign = np.concatenate([np.full(int(sizes[target]) + 40 if inner.shape[0] else 40, target), rng.integers(0, nlist, size=5)]).astype(np.int64)
        new_ids = int(ids.max()) + 1 + np.arange(assign.shape[0], dtype=np.int64)
        new_vecs = draw(assign)
        moved = s.counters()["list_relocations"]
        s.add_batch(new_ids, new_vecs, assign)
        if inner.shape[0]:
            assert s.counters()["list_relocations"] > moved, self.tag
        vecs, ids, lists = np.concatenate([vecs, new_vecs]), np.concatenate([ids, new_ids]), np.concatenate([lists, assign])
        # 2. remove_ids: ids the first filter allows, ids it denies, new rows among them, and an id nobody stores
        S, _ = self.f["sets"][0]
        inS = np.isin(ids, S)
        kill = np.concatenate([rng.permutation(ids[inS])[:60], rng.permutation(ids[~inS])[:60], new_ids[:3]])
        kill = np.unique(kill)[:max(1, ids.shape[0] // 4)]
        assert s.remove_ids(np.concatenate([kill, np.array([10 ** 12], np.int64)])) == kill.shape[0], self.tag
        keep = ~np.isin(ids, kill)
        vecs, ids, lists = vecs[keep], ids[keep], lists[keep]
        # 3. remove_list of a non-empty list (the parent keeps ranking its centroid)
        sizes = np.bincount(lists, minlength=nlist)
        if (sizes > 0).sum() >= 2:
            p = int(rng.choice(np.nonzero(sizes > 0)[0]))
            s.remove_list(p)
            present.discard(p)
            self.absent.add(p)
            keep = lists != p
            vecs, ids, lists = vecs[keep], ids[keep], lists[keep]
        # 4. refine_lists over three lists: the rows are re-assigned among three moved centroids (the oracle's refinement over the
        # lists in the store's own row order)
        if nlist >= 4 and len(present) >= 3:
            sub = np.sort(rng.choice(sorted(present), size=3, replace=False)).astype(np.int64)
            by_id = dict(zip(ids.tolist(), range(ids.shape[0])))
            pi = [s.get_list_ids(int(p)) for p in sub]
            pv = [vecs[[by_id[int(t)] for t in li]].reshape(-1, d) for li in pi]
            if sum(len(li) for li in pi) > 0:
                cent3 = (c["cent"][sub] + (rng.integers(-1, 2, size=(3, d)) if c["integer"] else 0.2 * rng.standard_normal((3, d)))).astype(np.float32)
                rvecs, rids, roffs = O.csr_from_partitions(pv, pi, d)
                rc, rv, ri, ro = O.kmeans_refine_partitions(cent3, rvecs, rids, roffs, metric, 0)
                if not np.isnan(rc).any():  # (an emptied cluster: the store refuses, tests/test_kmeans_gpu.py)
                    gc = s.refine_lists(sub, cent3, metric, 0)
                    np.testing.assert_array_equal(np.asarray(gc).view(np.uint32), rc.view(np.uint32), err_msg=str(self.tag))
                    for j, p in enumerate(sub):
                        lists[[by_id[int(t)] for t in ri[ro[j]:ro[j + 1]]]] = p
        # 5. the columns: new values (ids that had none and new rows among them), values taken away
        for name, col in cols.items():
            some = rng.permutation(ids)[:12]
            vals = rng.integers(0, 7, size=some.shape[0]).astype(np.int64)
            self.attrs[name].set(some, vals)
            col.update(zip(some.tolist(), vals.tolist()))
            gone = rng.permutation(np.fromiter(col.keys(), np.int64, len(col)))[:12]
            self.attrs[name].unset(gone)
            for t in gone.tolist():
                del col[t]
        # the store against the model, list by list; the row order is the store's
        assert sorted(int(p) for p in s.list_ids()) == sorted(present), self.tag
        out_v, out_i, offsets = [], [], np.zeros(nlist + 1, np.int64)
        for p in range(nlist):
            if p in present:
                gv, gi = s.get_list(p)
                mine = np.nonzero(lists == p)[0]
                mine = mine[np.argsort(ids[mine])]
                o = np.argsort(gi)
                np.testing.assert_array_equal(gi[o], ids[mine], err_msg=f"{self.tag} list {p}")
                np.testing.assert_array_equal(gv[o].view(np.uint32), vecs[mine].view(np.uint32), err_msg=f"{self.tag} list {p}")
                out_v.append(gv)
                out_i.append(gi)
            offsets[p + 1] = offsets[p] + (out_i[-1].shape[0] if p in present else 0)
        csr = (np.ascontiguousarray(np.concatenate(out_v)), np.ascontiguousarray(np.concatenate(out_i)), offsets)
        return csr, {name: (np.fromiter(col.keys(), np.int64, len(col)), np.fromiter(col.values(), np.int64, len(col))) for name, col in cols.items()}

    def resume(self, csr):
        """the cursors taken behind page 0 before the store changed, resumed now: the yardstick's page over the changed CSR, and no row
        of page 0 again"""
        c = self.c
        n1 = min(c["Q"], RF.ONE_AT_A_TIME)
        for name, flt, (S, mode) in (("pages", None, (None, "allow")), ("pages_filtered", self.filters[0], self.f["sets"][0])):
            nk, ni, first = self.page0[name]
            cursors = PY.cursor_list(nk[:n1], ni[:n1])
            got = self.ctx.search_after(self.parent, self.s, c["q"][:n1], c["nprobe"], c["k"], c["metric"], after=(nk[:n1], ni[:n1]), filter=flt)
            want = RF.resumed_page(c, csr, cursors, S, mode)
            m = self.msg("pages", False, 0, name + " resumed after the mutation")
            self.rows(got, want, m)
            assert PY.cursor_list(got[2][0], got[2][1]) == want[2], "cursors " + m
            for i in range(n1):
                assert not np.isin(got[0][i][got[0][i] >= 0], first[i]).any(), f"query {i} repeats a row " + m


def _feature_legs(c, device):
    rig = _Rig(c)
    try:
        rig.run(RF.expected(c), device)
        assert not any(rig.skipped.values()), rig.skipped   # (test_random_features_oracle.py: no leg is refused in these sets)
        return rig.ctx.last_scan_kernel()
    finally:
        rig.close()


@pytest.mark.parametrize("seed", RF.default_seeds())
def test_random_shape_features_bit_exact(seed):
    _feature_legs(RF.feature_case(seed), device=seed % 3 == 0)


@pytest.mark.parametrize("i", list(range(len(RF.SEAM_CASES))), ids=lambda i: "d%d" % RF.SEAM_CASES[i]["d"])
def test_random_shape_features_seams(i):
    """d = 256, 260, 1000 and 3000: what _case cannot draw, host and device memory"""
    last = _feature_legs(RF.seam_case(i), device=True)
    assert last.startswith("k_scan_wide") == (RF.SEAM_CASES[i]["d"] == 3000), last


@pytest.mark.parametrize("seed", RF.MUTATION_SEEDS)
def test_random_shape_features_after_mutation(seed):
    """one round of the legs, the store mutated under the live context, filters and columns, every leg again"""
    c = RF.feature_case(seed)
    rig = _Rig(c)
    try:
        rig.run(RF.expected(c), device=False)
        csr, cols = rig.mutate(seed)
        rig.resume(csr)
        rig.run(RF.expected(c, csr=csr, cols=cols), device=seed % 3 == 0)
    finally:
        rig.close()
