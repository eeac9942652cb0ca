"""The yardstick of diversified search (shared by tests/test_diverse_oracle.py, tests/test_diverse_search.py and
tests/test_diverse_random.py; the definition: include/quake_hip.h, "diversified search").

expected() is the definition in plain numpy float32, one query at a time: every product and the difference of a cost are rounded
separately (numpy's float32 scalars never fuse), a NaN pairwise value is ignored by the min / max, a NaN cost loses to every other
cost, ties go to the smaller rank.  case() builds what it takes from the oracle alone: O.search / O.batched_serial_scan with
k = fetch_k over the probed lists gives a query's candidates in (key, id) order and their distances -- under a filter over the
reduced CSR of tests/filter_yardstick.py, as tests/paging_yardstick.py does it -- and O.pair_values over the candidates' vectors
gives the pairwise values (with sqrt for L2 unless the squared domain is asked for).  Nothing here knows about tables or kernels."""
import numpy as np

import filter_yardstick as FY
import oracle as O
import range_yardstick as RY

NAMES = ("ids", "dist", "rank")


def pad_value(metric):
    return np.float32(-np.inf if metric == "ip" else np.inf)


def better(a, b, metric):
    """is the cost a strictly better than b: smaller for L2, larger for IP; a NaN cost loses to every non-NaN cost and two NaN
    costs tie (-0 and +0 compare equal)"""
    if np.isnan(a):
        return False
    if np.isnan(b):
        return True
    return bool(a > b) if metric == "ip" else bool(a < b)


def expected(cand_ids, cand_dist, pair, k, lam, metric):
    """One query.  cand_ids [n], cand_dist [n]: its candidates in rank order and their reported distances; pair [n, n]: the
    pairwise values in the same domain.  -> (ids [k], dist [k], rank [k] int32) in selection order, padded with -1 / +-inf / -1.
    Every array below is float32 and every numpy operation on it rounds once: lam * r, mu * N and their difference are the three
    roundings of the definition."""
    cand_ids = np.asarray(cand_ids, np.int64)
    r = np.asarray(cand_dist, np.float32)
    pair = np.asarray(pair, np.float32)
    n = cand_ids.shape[0]
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    m = min(k, n)
    out_i = np.full(k, -1, np.int64)
    out_d = np.full(k, pad_value(metric), np.float32)
    out_r = np.full(k, -1, np.int32)
    picked = np.zeros(n, bool)
    N = np.full(n, np.nan, np.float32)   # the most similar pairwise value to the picked set so far; NaN: none counted
    pick = 0
    for j in range(m):
        out_i[j], out_d[j], out_r[j] = cand_ids[pick], r[pick], pick
        picked[pick] = True
        if j == m - 1:
            break
        p = pair[:, pick]
        counts = ~np.isnan(p)                       # a NaN pairwise value is ignored
        have = ~np.isnan(N)
        with np.errstate(invalid="ignore", over="ignore"):
            both = (np.maximum if metric == "ip" else np.minimum)(N, p)
            N = np.where(counts & have, both, np.where(counts, p, N)).astype(np.float32)
            a = (lam * r).astype(np.float32)
            b = (mu * N).astype(np.float32)
            cost = np.where(np.isnan(N), a, (a - b).astype(np.float32)).astype(np.float32)   # no value counted: the term is dropped
        live = ~picked & ~np.isnan(cost)            # a NaN cost loses to every other cost
        if live.any():
            best = cost[live].max() if metric == "ip" else cost[live].min()
            pick = int(np.nonzero(live & (cost == best))[0][0])   # ties (-0 == +0 among them) go to the smaller rank
        else:
            pick = int(np.nonzero(~picked)[0][0])   # every cost NaN: the smaller rank
    return out_i, out_d, out_r


def brute_force(cand_ids, cand_dist, pair, k, lam, metric):
    """The same definition written independently: at every step the min / max over the whole picked set is recomputed from
    scratch with numpy's NaN-ignoring reductions, and the winner is found by sorting (class, cost, rank) triples."""
    cand_ids = np.asarray(cand_ids, np.int64)
    r = np.asarray(cand_dist, np.float32)
    pair = np.asarray(pair, np.float32)
    n = cand_ids.shape[0]
    lam32 = np.float32(lam)
    mu32 = np.float32(np.float32(1.0) - lam32)
    S = [0] if n else []
    while len(S) < min(k, n):
        rows = []
        for i in range(n):
            if i in S:
                continue
            vals = pair[i, S]
            vals = vals[~np.isnan(vals)]
            with np.errstate(invalid="ignore", over="ignore"):
                a = np.float32(lam32 * r[i])
                if vals.shape[0]:
                    Ni = vals.max() if metric == "ip" else vals.min()
                    c = np.float32(a - np.float32(mu32 * Ni))
                else:
                    c = a
            if np.isnan(c):
                rows.append((1, 0.0, i))
            else:
                rows.append((0, float(-c) if metric == "ip" else float(c), i))   # (float32 -> float64 is exact; -0.0 == 0.0)
        rows.sort()
        S.append(rows[0][2])
    out_i = np.full(k, -1, np.int64)
    out_d = np.full(k, pad_value(metric), np.float32)
    out_r = np.full(k, -1, np.int32)
    for j, i in enumerate(S):
        out_i[j], out_d[j], out_r[j] = cand_ids[i], r[i], i
    return out_i, out_d, out_r


def candidates(q, centroids, vecs, ids, offsets, nprobe, C, metric, S=None, mode="allow", pids=None, squared=False):
    """the row a search with k = C returns for every query: (ids [Q, C], dist [Q, C]).  centroids None and pids None: a flat index
    (every list); pids [Q, P]: the scan form; S / mode: a filter, applied by deleting the other rows from the CSR first"""
    q = np.ascontiguousarray(q, np.float32)
    if S is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, FY.allowed_rows(ids, S, mode))
    ids = np.asarray(ids, np.int64)
    if pids is None:
        if centroids is None:
            pids = np.broadcast_to(RY.probed(q, None, offsets, nprobe, metric)[None, :], (q.shape[0], np.asarray(offsets).shape[0] - 1))
            oi, od = O.batched_serial_scan(q, vecs, ids, offsets, np.ascontiguousarray(pids), C, metric)
        else:
            oi, od = O.search(q, centroids, vecs, ids, offsets, nprobe, C, metric, batched_scan=True, num_threads=8)
    else:
        oi, od = O.batched_serial_scan(q, vecs, ids, offsets, np.asarray(pids, np.int64), C, metric)
    if squared and metric == "l2":
        # the squared domain: the canonical squared values themselves (the oracle's search reports their square roots)
        row_of = {int(t): i for i, t in enumerate(ids.tolist())}
        od = od.copy()
        for qi in range(q.shape[0]):
            n = int((oi[qi] >= 0).sum())
            if n:
                rows = np.array([row_of[int(t)] for t in oi[qi, :n]], np.int64)
                od[qi, :n] = O.pair_values(q[qi:qi + 1], vecs[rows], metric)[0]
    return oi, od


def pairwise(V, metric, squared=False):
    """p(i, j) over the vectors V [n, d]: the value a search reports for row i under the query V[j]"""
    V = np.ascontiguousarray(V, np.float32)
    if V.shape[0] == 0:
        return np.zeros((0, 0), np.float32)
    P = O.pair_values(V, V, metric)
    if metric == "l2" and not squared:
        with np.errstate(invalid="ignore"):
            P = np.sqrt(P)
    return np.ascontiguousarray(P.T)   # [row i, query j]


def prepare(q, centroids, vecs, ids, offsets, nprobe, C, metric, S=None, mode="allow", pids=None, squared=False):
    """per query (candidate ids [n], distances [n], pairwise values [n, n]) with fetch_k = C, from the oracle alone"""
    vecs = np.ascontiguousarray(vecs, np.float32)
    ids = np.asarray(ids, np.int64)
    oi, od = candidates(q, centroids, vecs, ids, offsets, nprobe, C, metric, S, mode, pids, squared)
    row_of = {int(t): i for i, t in enumerate(ids.tolist())}
    assert len(row_of) == ids.shape[0], "ids must be unique"
    prep = []
    for qi in range(oi.shape[0]):
        n = int((oi[qi] >= 0).sum())
        assert (oi[qi, n:] == -1).all(), "padding follows the candidates"
        rows = np.array([row_of[int(t)] for t in oi[qi, :n]], np.int64)
        P = pairwise(vecs[rows], metric, squared)
        nan = np.isnan(P)
        assert ((P == P.T) | (nan & nan.T)).all(), "the pairwise values must be symmetric (a precondition of the contract)"
        prep.append((oi[qi, :n].copy(), od[qi, :n].copy(), P))
    return prep


def expected_batch(prep, k, lam, metric):
    """(ids [Q, k], dist [Q, k], rank [Q, k]) of the queries of prepare()"""
    Q = len(prep)
    out = (np.empty((Q, k), np.int64), np.empty((Q, k), np.float32), np.empty((Q, k), np.int32))
    for qi, (ci, cd, P) in enumerate(prep):
        for o, v in zip(out, expected(ci, cd, P, k, lam, metric)):
            o[qi] = v
    return out


def case(q, centroids, vecs, ids, offsets, nprobe, k, C, lam, metric, S=None, mode="allow", pids=None, squared=False):
    """the expected (ids [Q, k], dist [Q, k], rank [Q, k]) of a diversified search"""
    return expected_batch(prepare(q, centroids, vecs, ids, offsets, nprobe, C, metric, S, mode, pids, squared), k, lam, metric)
