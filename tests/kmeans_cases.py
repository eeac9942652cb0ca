"""The cases of the k-means shape sweep (tests/test_kmeans_shapes_gpu.py runs them on the device, tests/test_kmeans_cases_oracle.py
pins on the CPU what they reach) and a restatement of the dispatch of quake_amd/csrc/qk_kmeans.hip, so that a case can say which
kernel form it is for.  Plain Python and numpy: no GPU, no torch at import.

The restated rules (`assign_form`, `bucket_plan`, `blocked_form`) only choose and label cases.  If one of them drifts from the
library it can lose coverage -- a case then runs another kernel than its label says -- but it cannot pass a wrong answer: every case
compares bits with the oracle whichever kernel ran.

Finite values only: the header puts k-means on non-finite input outside the rule (include/quake_hip.h, "non-finite values")."""
import functools
import zlib

import numpy as np

from helpers import make_ivf

U = 2.0 ** -24                      # unit roundoff of float32
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
METRICS = ("l2", "ip")


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------
APF_MIN_ROWS = 40960                # qk_assign_pf.hip: APF_MIN_ROWS


def assign_pf_supported(n, m, d):
    """qk_assign_pf_supported (qk_assign_pf.hip:445-453), the environment switch aside"""
    return d % 8 == 0 and 8 <= d <= 128 and 64 <= m <= (1 << 24) and n >= APF_MIN_ROWS


def assign_form(n, m, d, metric="l2", aligned=True):
    """which kernel assign_device launches (qk_kmeans.hip:743-767): "pf", "wide" or ("mfma", DB, NQ); the metric picks the
    instantiation of the same form, not the form"""
    if assign_pf_supported(n, m, d) and aligned:                       # :743
        return "pf"
    nblk = (d + 15) // 16                                              # :736
    DB = 8 if nblk % 8 == 0 else 4 if nblk % 4 == 0 else 2 if nblk % 2 == 0 else 1   # :756
    NQ = 4
    while NQ > 1 and NQ * nblk * 1024 > 64 * 1024:                     # :758-759
        NQ >>= 1
    if n <= 16:                                                        # :760
        NQ = 1
    lds = NQ * nblk * 1024 + NQ * 16 * 4 + 4 * NQ * 16 * 8 + 64        # :761
    if lds > 160 * 1024:                                               # :762
        return "wide"
    return ("mfma", DB, NQ)


def assign_tiles(m, d, DB):
    """k_assign's split of the centroid tiles over its four waves (qk_kmeans.hip:101-108): (mt, tpw, [nsteps of every wave with
    t1 > t0])"""
    nblk = (d + 15) // 16
    mt = (m + 15) >> 4
    tpw = (mt + 3) >> 2
    ncd = nblk // DB
    steps = []
    for wave in range(4):
        t0 = wave * tpw
        t1 = min(mt, t0 + tpw)
        if t1 > t0:
            steps.append((t1 - t0) * ncd)
    return mt, tpw, steps


def wave_of_centroid(idx, m):
    mt = (m + 15) >> 4
    tpw = (mt + 3) >> 2
    return (idx >> 4) // tpw


def bucket_plan(n, m):
    """rs_plan (qk_kmeans.hip:787-800): (bits, passes, wave_rows, nchunks); the entry points call it with max(n, 1)"""
    n = max(n, 1)
    kb = 1
    while (1 << kb) < m:
        kb += 1
    bits = 8 if kb <= 8 else 12
    passes = (kb + bits - 1) // bits
    wr = 1024
    while ((n + 4 * wr - 1) // (4 * wr)) * (4 << bits) > (64 << 20):
        wr *= 2
    return bits, passes, wr, max(1, (n + 4 * wr - 1) // (4 * wr))


KM_GROUP, KM_GLANES = 1024, 8


def blocked_form(n, m, d, aligned=True):
    """the launch of k_accumulate_blocked (accumulate_device, qk_kmeans.hip:893-899, and the kernel's :552-555):
    (V, units, TPC, NCH, trips, lanes)"""
    lanes = min(KM_GLANES, max(2, (n + 128 * m - 1) // (128 * m)))
    V = "float4" if d % 4 == 0 and aligned else "float"
    units = d // 4 if V == "float4" else d
    TPC = min(units, 256)
    return V, units, TPC, 256 // TPC, (units + TPC - 1) // TPC, lanes


def reference_order_trips(d):
    """k_accumulate is launched with min(256, round_up(d, 64)) threads (:888); trips of its `k += blockDim.x` loop"""
    threads = min(256, (d + 63) // 64 * 64)
    return (d + threads - 1) // threads


def groups_of(size):
    return (size + KM_GROUP - 1) // KM_GROUP


# ---- assign cases -------------------------------------------------------------------------------------------------------------
ASSIGN_D = (1, 4, 16, 17, 32, 64, 100, 128, 256, 257, 288, 320, 384, 512, 513, 544, 576, 768, 1000, 2528, 2544, 2545, 2560)
ASSIGN_N = (1, 15, 16, 17, 31, 33, 63, 64, 65, 129, 1000)
ASSIGN_M = (1, 2, 15, 16, 17, 31, 33, 47, 48, 49, 63, 64, 65, 130, 1000)
KINDS = ("mixture", "spread", "ties")
PAIRS = 6
PROPS = ("nrag", "mrag", "few", "odd", "even", "tie")


def assign_facts(n, m, d, kind):
    """what a case reaches, from the restated rules alone: a set of (form, property)"""
    form = assign_form(n, m, d)
    DB, NQ = (form[1], form[2]) if form != "wide" else (1, 1)
    mt, tpw, steps = assign_tiles(m, d, DB)
    out = set()
    if n % (16 * NQ):
        out.add((form, "nrag"))           # the `row < P.n` guard of the last tile
    if m % 16:
        out.add((form, "mrag"))           # `idx_ < P.m` in the last centroid tile
    if mt < 4:
        out.add((form, "few"))            # waves with t1 <= t0
    if form != "wide":
        for s in steps:
            out.add((form, "odd" if s % 2 else "even"))   # where the two-buffer loop ends
    if kind == "ties" and m >= 17:
        out.add((form, "tie"))            # a copy of a centroid in another wave's tile range
    if n <= 16 and form != "wide":
        out.add((form, "override"))
    return out


@functools.lru_cache(maxsize=None)
def _fact_table(d):
    return {(n, m, k): frozenset(assign_facts(n, m, d, k)) for n in ASSIGN_N for m in ASSIGN_M for k in KINDS if not (k == "ties" and m < 2)}


@functools.lru_cache(maxsize=None)
def assign_group(d, metric):
    """six (n, m, kind) of one (d, metric): drawn by a seeded generator and redrawn until they reach together every
    (form, property) that any (n, m, kind) of the pools reaches at this d"""
    table = _fact_table(d)
    keys = sorted(table)
    want = frozenset().union(*table.values())
    for attempt in range(200000):
        rng = np.random.default_rng(_seed("assign", d, metric, attempt))
        pick = [keys[i] for i in rng.choice(len(keys), size=PAIRS, replace=False)]
        if frozenset().union(*(table[p] for p in pick)) == want:
            return tuple(pick)
    raise AssertionError("no draw of %d pairs reaches every form at d = %d" % (PAIRS, d))


def assign_groups():
    return [(d, metric) for d in ASSIGN_D for metric in METRICS]


def assign_data(n, m, d, metric, kind):
    """(x [n][d], c [m][d]) of one assign case; finite float32"""
    rng = np.random.default_rng(_seed("assign-data", n, m, d, metric, kind))
    c = rng.standard_normal((m, d)).astype(np.float32)
    x = (c[rng.integers(0, m, size=n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    if kind == "mixture" and m <= min(d, 130):
        # up to three rows whose dot product with EVERY centroid is -1 (the least-norm solution of C x = -1): under IP the best
        # value is negative, so a padded zero centroid taken for a real one (dot 0) would win
        far = -(np.linalg.pinv(c.astype(np.float64)) @ np.ones(m)).astype(np.float32)
        x[rng.permutation(n)[:3]] = far
    if kind == "spread":
        x *= (10.0 ** rng.uniform(-2, 2, size=(n, 1))).astype(np.float32)
        c *= (10.0 ** rng.uniform(-2, 2, size=(m, 1))).astype(np.float32)
    if kind == "ties":
        # centroid i copied to one or two higher indices in other waves' tile ranges (anywhere above i when there is no other
        # wave); the rows of a random half are themselves such centroids: both distances are the same bits, the lower index wins
        mt = (m + 15) >> 4
        tpw = (mt + 3) >> 2
        first_other = min(m, 16 * tpw)          # first centroid of wave 1
        bases = []
        big = 2.0 * float(np.linalg.norm(c, axis=1).max())

        def lift(t):   # IP: a centroid of twice the largest norm is the best match of the row that equals it (L2: distance 0 is)
            if metric == "ip":
                c[t] = (c[t].astype(np.float64) / np.linalg.norm(c[t].astype(np.float64)) * big).astype(np.float32)

        i = int(rng.integers(0, min(first_other, m - 1)))
        lift(i)
        lo = first_other if first_other < m else i + 1
        for j in rng.choice(np.arange(lo, m), size=min(int(rng.integers(1, 3)), m - lo), replace=False):
            c[j] = c[i]
        bases.append(i)
        if m >= 4:
            free = [t for t in range(m - 1) if not (c[t] == c[i]).all()]
            if free:
                i2 = int(rng.choice(free))
                above = [t for t in range(i2 + 1, m) if not (c[t] == c[i]).all()]
                if above:
                    lift(i2)
                    c[int(rng.choice(above))] = c[i2]
                    bases.append(i2)
        rows = rng.permutation(n)[: (n + 1) // 2]
        x[rows] = c[[bases[t % len(bases)] for t in range(rows.shape[0])]]
    return np.ascontiguousarray(x), np.ascontiguousarray(c)


def pad_column(a):
    """the same rows with one more zero column: d = 2544 -> 2545, across the LDS seam"""
    return np.ascontiguousarray(np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], 1))


# ---- accumulate cases ---------------------------------------------------------------------------------------------------------
ACC_D = (1, 3, 4, 6, 63, 64, 65, 255, 256, 257, 260, 1024, 1028, 1101)
ACC_SIZES = (0, 1, 31, 32, 33, 1023, 1024, 1025, 2048, 3 * 1024 + 1, 9 * 1024 + 5)   # prescribed, not drawn
# two arrangements: "lanes8" holds every size (m = 11, ~17 500 rows: 8 group lanes, the largest centroid has G = 10 groups);
# "lanes2" is 20 centroids over ~4 200 rows (2 group lanes) with one of G = 4: a workgroup takes two groups
ARRANGEMENTS = {
    "lanes8": (1025, 0, 9 * 1024 + 5, 1, 2048, 31, 1024, 32, 3 * 1024 + 1, 33, 1023),
    "lanes2": (33, 0, 3 * 1024 + 1, 1, 1023, 31, 32, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1),
}
ORDERS = ("reference", "blocked")


def out_of_range(m):
    """assignments the kernels must ignore; they compare in 64 bits (a truncating compare would count 2^32 + 1 as centroid 1)"""
    return [-1, m, m + 3, 2 ** 32 + 1, INT64_MIN, INT64_MAX]


def _rows_for(sizes, d, tag, oor_each=2):
    m = len(sizes)
    a = np.concatenate([np.full(s, c, np.int64) for c, s in enumerate(sizes)] + [np.array(out_of_range(m) * oor_each, np.int64)])
    rng = np.random.default_rng(_seed("acc", tag, d))
    a = a[rng.permutation(a.shape[0])]                                      # rows interleaved by a permutation
    n = a.shape[0]
    x = rng.standard_normal((n, d), dtype=np.float32) * (10.0 ** rng.integers(-2, 3, size=(n, 1))).astype(np.float32)
    return x, a, m


LARGE = dict(n=2 ** 24 + 4097, d=2, m=300)   # rs_plan's `wr *= 2`: more than 4096 chunks of 4 x 1024 rows at 12 bits


def accumulate_cases():
    """(name, d): the data of a case is accumulate_data(name, d); every case runs in both orders"""
    out = [(arr, d) for d in ACC_D for arr in ("lanes8", "lanes2")]
    out += [("m257", 6), ("all_out_of_range", 5), ("n0", 5), ("large", LARGE["d"])]
    return out


@functools.lru_cache(maxsize=2)
def accumulate_data(name, d):
    """(x [n][d], assign [n], m, sizes): sizes are the prescribed sizes of the centroids, None where they are drawn"""
    if name in ARRANGEMENTS:
        sizes = ARRANGEMENTS[name]
        x, a, m = _rows_for(sizes, d, name)
        return x, a, m, np.array(sizes, np.int64)
    if name == "m257":      # 12 bits, one pass; the seams of m are tests/test_kmeans_gpu.py::test_accumulate_bucket_passes
        sizes = [(0, 1, 31, 32, 33)[c % 5] for c in range(257)]
        sizes[100] = 1025
        x, a, m = _rows_for(sizes, d, name)
        return x, a, m, np.array(sizes, np.int64)
    if name == "all_out_of_range":   # n_dev = 0
        x, a, m = _rows_for([0, 0, 0], d, name, oor_each=80)
        return x, a, m, np.zeros(3, np.int64)
    if name == "n0":
        return np.zeros((0, d), np.float32), np.zeros(0, np.int64), 3, np.zeros(3, np.int64)
    if name == "large":
        rng = np.random.default_rng(_seed("acc", name))
        n, m = LARGE["n"], LARGE["m"]
        x = rng.standard_normal((n, d), dtype=np.float32)
        x *= (10.0 ** rng.integers(-2, 3, size=(n, 1))).astype(np.float32)
        a = rng.integers(0, m, size=n, dtype=np.int64)
        a[:: 2 ** 20] = np.resize(np.array(out_of_range(m), np.int64), a[:: 2 ** 20].shape[0])
        return x, a, m, None
    raise KeyError(name)


MISALIGNED = ("lanes2", 64)   # run once more from a device x that starts 4 bytes into its buffer: k_accumulate_blocked<float>


# ---- update, normalise and permutation cases ----------------------------------------------------------------------------------
UPDATE_M, UPDATE_D = (1, 5, 300), (1, 3, 128, 1101)
UPDATE_PATTERNS = ("full", "donor", "nosplit", "tied")


def update_case(m, d, pattern):
    """(sums [m][d], counts [m], centroids [m][d]) of one qk_kmeans_update"""
    rng = np.random.default_rng(_seed("update", m, d, pattern))
    counts = rng.integers(2, 60, size=m).astype(np.int64)
    if pattern == "donor":          # several empties and a donor (with one centroid: the empty one alone)
        counts[rng.permutation(m)[: max(1, m // 3)]] = 0
    elif pattern == "nosplit":      # empties, every count < 2: nothing splits, the oracle returns the counts unchanged
        counts = rng.integers(0, 2, size=m).astype(np.int64)
        counts[int(rng.integers(0, m))] = 0
    elif pattern == "tied":         # the largest count tied between two clusters: the lower index donates
        counts[rng.permutation(m)[: max(1, m // 4)]] = 0
        if m >= 3:
            i, j = sorted(rng.choice(m, size=2, replace=False))
            counts[i] = counts[j] = 77
    sums = (rng.standard_normal((m, d)) * 10.0 ** rng.integers(-2, 3, size=(m, 1))).astype(np.float32)
    cent = rng.standard_normal((m, d)).astype(np.float32)
    return sums, counts, cent


NORM_N, NORM_D = (1, 255, 256, 257, 1000), (1, 3, 128, 1101)


def normalize_case(n, d):
    """rows with scales 10^-18 .. 10^18 (squares stay inside float32).  No zero rows: 0 / 0 is a NaN whose sign differs between
    the hosts' and the device's division."""
    rng = np.random.default_rng(_seed("norm", n, d))
    x = rng.standard_normal((n, d))
    x = np.where(np.abs(x) < 0.5, np.where(x < 0, -0.5, 0.5), x) / np.sqrt(d)        # row norms near 1 before the scale
    x = (x * 10.0 ** rng.uniform(-18, 18, size=(n, 1))).astype(np.float32)
    assert np.isfinite(x).all() and (x != 0).any(1).all()
    return x


PERM_CASES = tuple((n, m, seed) for (n, m) in ((0, 0), (1, 5), (5, 0), (5, 9), (1000, 10), (1000, 1000)) for seed in (0, 1234, 2 ** 40 + 5))


# ---- driver cases -------------------------------------------------------------------------------------------------------------
DRIVER_CASES = ((2, 2, 8, "l2", 5), (3, 2, 5, "ip", 5), (40, 40, 300, "l2", 2), (50, 1, 17, "l2", 3), (200, 7, 768, "ip", 0),
                (600, 2, 100, "l2", 5), (17, 3, 2544, "l2", 2), (300, 4, 2545, "ip", 2))
DRIVER_SEED = 1234


@functools.lru_cache(maxsize=None)
def driver_data(n, m, d, metric, niter):
    rng = np.random.default_rng(_seed("driver", n, m, d, metric, niter))
    cent = rng.standard_normal((max(m, 2), d)).astype(np.float32)
    return np.ascontiguousarray((cent[rng.integers(0, cent.shape[0], size=n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32))


# ---- refine cases -------------------------------------------------------------------------------------------------------------
REFINE_LISTS, REFINE_EMPTY = 12, 3
REFINE_D = (24, 300)
REFINE_SELECTIONS = {"with_empty": (7, 3, 9, 4), "one_list": (5,)}
REFINE_ITERS = (0, 1, 3)


@functools.lru_cache(maxsize=None)
def refine_store(d, metric):
    """a store of 12 lists, list 3 empty"""
    return make_ivf(1500, d, REFINE_LISTS, seed=31 + d, metric=metric, empty=(REFINE_EMPTY,))


def refine_case(d, metric, selection):
    """(ivf, sel, centroids): slightly off-centre centroids so that vectors really move; the empty list's centroid is another
    slightly off-centre copy of the first selected list's, so that it takes a share of its rows and no cluster empties (asserted on
    the CPU)"""
    ivf = refine_store(d, metric)
    sel = np.array(REFINE_SELECTIONS[selection], np.int64)
    rng = np.random.default_rng(_seed("refine", d, metric, selection))
    off = 0.25 / np.sqrt(d)   # an offset of norm ~0.25 at every d (0.05 per component at d = 24)
    cent = (ivf["centroids"][sel] + off * rng.standard_normal((len(sel), d))).astype(np.float32)
    for j, p in enumerate(sel):
        if p == REFINE_EMPTY:
            cent[j] = (ivf["centroids"][sel[0]] + off * rng.standard_normal(d)).astype(np.float32)
            if metric == "ip":   # (two centroids of one direction do not share a cluster under IP: the longer takes every row.
                rows = ivf["part_vecs"][sel[0]]   # A row of the cluster does: a unit row's best match is itself)
                cent[j] = rows[len(rows) // 2]
    return ivf, sel, cent


def refine_csr(ivf, sel):
    import oracle as O
    return O.csr_from_partitions([ivf["part_vecs"][p] for p in sel], [ivf["part_ids"][p] for p in sel], ivf["d"])


REFUSAL = dict(d=24, metric="l2", sel=(2, 9), iterations=2)


def refusal_case():
    """two selected lists; the second centroid is far from every row, so it receives none at the first assignment, its mean is 0 / 0
    at the second iteration and qk_store_refine_lists refuses"""
    ivf = refine_store(REFUSAL["d"], REFUSAL["metric"])
    sel = np.array(REFUSAL["sel"], np.int64)
    rows = np.concatenate([ivf["part_vecs"][p] for p in sel], 0)
    cent = np.stack([rows.mean(0), rows.mean(0) + 100.0]).astype(np.float32)
    return ivf, sel, cent
