"""The per-query merge kernels (quake_amd/csrc/qk_merge.hip: k_merge<2|4|8>, k_merge_flat<2>, k_merge_wide; k_next_cursor of
qk_after.hip; k_merge<16> needs k > QK_MAX_K and cannot be launched) on records a test lays out, through qk_debug_merge_records: ids, distance bits and the next cursor must equal the
yardstick (tests/merge_yardstick.py) for every form that takes (k, P), form 0 -- what a search launches -- included.  Behind a scan
the geometry these kernels meet is a by-product of the scan plan; here every launch holds one query per geometry: no record, mixed
/ full / short records, five key values, ALL KEYS EQUAL (no bound prunes, every pool overflows), a tie on the k-th key across two
records and across two pairs, infinities and signed zeros, a chain of 256 / 257 records holding the best keys, a record that did
not fit.

Coverage of the grid: every k of KS is a test; each takes three values of P (a seeded sample; test_grid_is_covered checks that every
P appears) and both metrics; every admissible form runs on the same records, with sqrt_l2 and out_dist = NULL alternating."""
import numpy as np
import pytest

import merge_yardstick as Y

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = (1, 2, 21, 22, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 448)
PS = (1, 7, 8, 9, 63, 64, 65, 130)
FORMS = ("rule", "chain", "flat", "wide")


def ps_of(k):
    """three values of P for this k: a rotation through PS, so that every P meets small, middle and large k"""
    i = KS.index(k)
    return sorted({PS[i % 8], PS[(3 * i + 1) % 8], PS[(5 * i + 2) % 8]})


def expected_kernel(form, k, P):
    """the rule of the merge launch (DESIGN.md 5.12 / qk_merge.hip): k >= 33 one workgroup per query; k <= 32 the flat form up to 64
    pairs, else the chained walk; MAXCH of the one-wave forms from the pool of k + 64 entries rounded up to 64"""
    if form == "rule":
        form = "wide" if k >= 33 else "flat" if P <= 64 else "chain"
    if form == "wide":
        return "k_merge_wide"
    if form == "flat":
        return "k_merge_flat<2>"
    cm = (k + 64 + 63) // 64 * 64
    return "k_merge<%d>" % (2 if cm <= 128 else 4 if cm <= 256 else 8 if cm <= 512 else 16)


def admits(form, k, P):
    return form != "flat" or (k <= 32 and P <= 64)


def test_grid_is_covered():
    assert {p for k in KS for p in ps_of(k)} == set(PS)
    assert all(len(ps_of(k)) == 3 for k in KS)
    names = {expected_kernel(f, k, p) for k in KS for p in ps_of(k) for f in FORMS if admits(f, k, p)}
    # (k_merge<16> needs a pool beyond 512 entries, i.e. k > QK_MAX_K = 448: no admissible k reaches it)
    assert names == {"k_merge<2>", "k_merge<4>", "k_merge<8>", "k_merge_flat<2>", "k_merge_wide"}


@pytest.fixture(scope="module")
def ctx():
    from quake_amd.capi import Context
    c = Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _device(rb):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    return (t(rb["pair_slots"], np.int32), t(rb["pair_head"], np.int32), t(rb["rec_hdr"], np.int32), t(rb["rec_ord"], np.int32),
            t(rb["rec_id"], np.int64))


def _check(ctx, dev, rb, names, k, P, metric, form, sqrt_l2, dist, launched):
    out = ctx.merge_records(*dev, k=k, metric=metric, form=form, sqrt_l2=sqrt_l2, dist=dist, cursor=True)
    torch.cuda.synchronize()
    assert out["kernel"] == expected_kernel(form, k, P), (form, k, P, out["kernel"])
    launched.add(out["kernel"])
    ri, rd, rk, rn = Y.merge_reference(rb["entries"], k, metric, sqrt_l2)
    gi = out["ids"].cpu().numpy()
    tag = "k=%d P=%d %s form=%s (%s) sqrt=%d" % (k, P, metric, form, out["kernel"], sqrt_l2)
    for q, nm in enumerate(names):
        np.testing.assert_array_equal(gi[q], ri[q], err_msg="ids of query '%s', %s" % (nm, tag))
    if dist:
        gd = out["dist"].cpu().numpy().view(np.uint32)
        for q, nm in enumerate(names):
            np.testing.assert_array_equal(gd[q], rd[q].view(np.uint32), err_msg="distance bits of query '%s', %s" % (nm, tag))
    else:
        assert out["dist"] is None
    gk, gn = out["next_key"].cpu().numpy().view(np.uint32), out["next_id"].cpu().numpy()
    np.testing.assert_array_equal(gk, rk, err_msg="next_key, %s: %s" % (tag, names))
    np.testing.assert_array_equal(gn, rn, err_msg="next_id, %s: %s" % (tag, names))
    return ri


@pytest.mark.parametrize("k", KS)
def test_every_form_equals_the_yardstick(ctx, k):
    launched = set()
    for j, P in enumerate(ps_of(k)):
        metric = ("l2", "ip")[(KS.index(k) + j) % 2]
        names, qs = Y.record_cases(k, P, metric, seed=7919 * k + P)
        rb = Y.build_records(qs, k, np.random.default_rng(k * 131 + P))
        dev = _device(rb)
        ri = None
        for f, form in enumerate(f for f in FORMS if admits(f, k, P)):
            ri = _check(ctx, dev, rb, names, k, P, metric, form, sqrt_l2=(f + j) % 2, dist=(f != 1), launched=launched)
        # what the case families are there for (the yardstick's own answer): padding, a chained k-th result, exhausted cursors
        assert (ri[names.index("empty")] == -1).all() and ri[names.index("short")][-1] == -1
        assert ri[names.index("chain")][-1] >= 0 and ri[names.index("equal")][-1] >= 0
    print("k=%d P=%s launched %s" % (k, ps_of(k), sorted(launched)))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_one_pair_without_a_record_and_the_other_metric(ctx, metric):
    """P = 1: a query whose only pair left nothing takes the flat form's early exit (the rounds of a recall-target search); next to
    it queries with one, 31 and 33 records.  Both metrics at one shape, every form, sqrt_l2 both ways."""
    k, P = 10, 1
    rng = np.random.default_rng(3)
    qs = [Y.make_query([[]], "distinct", metric, rng), Y.make_query([[k]], "distinct", metric, rng),
          Y.make_query([[3]], "special", metric, rng), Y.make_query([[k] * 31], "five", metric, rng),
          Y.make_query([[k, 4] * 16 + [7]], "best_last", metric, rng), Y.make_query([[]], "distinct", metric, rng)]
    names = ["none", "one", "three_entries", "slots_full", "chain_of_two", "none_again"]
    rb = Y.build_records(qs, k, rng)
    dev = _device(rb)
    launched = set()
    for form in FORMS:
        for sqrt_l2 in (0, 1):
            _check(ctx, dev, rb, names, k, P, metric, form, sqrt_l2, dist=True, launched=launched)
    assert launched == {"k_merge<2>", "k_merge_flat<2>", "k_merge_wide"}


def test_forms_the_arguments_do_not_admit_are_refused(ctx):
    from quake_amd._lib import QuakeHipError
    rng = np.random.default_rng(4)

    def launch(k, P, form):
        rb = Y.build_records([Y.make_query([[1]] * P, "distinct", "l2", rng)], k, rng)
        return ctx.merge_records(*_device(rb), k=k, metric="l2", form=form)
    for k, P, form in ((33, 4, "flat"), (8, 65, "flat"), (449, 2, "rule"), (449, 2, "wide"), (449, 2, "chain"), (8, 2, 4), (8, 2, -1)):
        with pytest.raises(QuakeHipError) as e:
            launch(k, P, form)
        assert e.value.status == 1, (k, P, form)          # QK_ERR_INVALID
    assert launch(32, 64, "flat")["kernel"] == "k_merge_flat<2>"
    torch.cuda.synchronize()
