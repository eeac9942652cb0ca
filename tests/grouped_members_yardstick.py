"""The yardstick of grouped search with members (shared by tests/test_grouped_members_oracle.py and tests/test_grouped_members.py).

Built on tests/grouped_yardstick.py: the candidates of a query are those of grouped search -- the rows of its probed lists that have
a value in the column, are allowed, and whose canonical value is not NaN -- ordered by (canonical value, id) as GY.reduce orders
them.  Groups are ranked by their first appearance in that order; the first k groups each take their first m rows.  ids / dist are
[Q, k, m], groups [Q, k]; padding as a short search() result (id -1, distance +inf / -inf, group 0), inside a live group too where
it has fewer than m candidates.  Distances are reported as search() does (sqrt of the squared form).  A filter: the same over the
reduced CSR of tests/filter_yardstick.py.  Nothing here knows about keys, hash tables or kernels."""
import numpy as np

import filter_yardstick as FY
import grouped_yardstick as GY


def reduce(cand, ids, rowval, rowhas, k, m, metric):
    lims, rows, val = cand
    ids = np.asarray(ids, np.int64)
    Q = lims.shape[0] - 1
    out_i = np.full((Q, k, m), -1, np.int64)
    out_d = np.full((Q, k, m), -np.inf if metric == "ip" else np.inf, np.float32)
    out_g = np.zeros((Q, k), np.int64)
    for i in range(Q):
        r, v = rows[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
        keep = rowhas[r] & ~np.isnan(v)
        r, v = r[keep], v[keep]
        if r.shape[0] == 0:
            continue
        key = (-v if metric == "ip" else v) + np.float32(0.0)   # (-0 + 0 == +0: both zeros are one value)
        order = np.lexsort((ids[r], key))
        r, v = r[order], v[order]
        g = rowval[r]
        uniq, first, inv = np.unique(g, return_index=True, return_inverse=True)
        rank_of = np.empty(uniq.shape[0], np.int64)
        rank_of[np.argsort(first, kind="stable")] = np.arange(uniq.shape[0])   # groups by first appearance
        grank = rank_of[inv.reshape(-1)]
        # position of every row inside its group, in the candidates' order
        by_group = np.argsort(grank, kind="stable")
        start = np.zeros(uniq.shape[0] + 1, np.int64)
        start[1:] = np.cumsum(np.bincount(grank, minlength=uniq.shape[0]))
        within = np.empty(r.shape[0], np.int64)
        within[by_group] = np.arange(r.shape[0]) - start[grank[by_group]]
        take = (grank < k) & (within < m)
        j, w = grank[take], within[take]
        out_i[i, j, w] = ids[r[take]]
        with np.errstate(invalid="ignore"):
            out_d[i, j, w] = np.sqrt(v[take]) if metric == "l2" else v[take]
        head = take & (within == 0)
        out_g[i, grank[head]] = g[head]
    return out_i, out_d, out_g


def scan(q, vecs, ids, offsets, pids, k, m, metric, attr_ids, attr_vals, S=None, mode="allow", keep=None):
    """scan_grouped(group_size=m)'s expected (ids [Q, k, m], dist [Q, k, m], groups [Q, k]); S / mode (an id set) or keep (bool per
    row): a filter, applied by deleting the other rows from the CSR first"""
    if S is not None:
        keep = FY.allowed_rows(ids, S, mode)
    if keep is not None:
        vecs, ids, offsets = FY.reduced_csr(vecs, ids, offsets, keep)
    rowval, rowhas = GY.row_values(ids, attr_ids, attr_vals)
    return reduce(GY.candidates(q, vecs, ids, offsets, pids, metric), ids, rowval, rowhas, k, m, metric)


def search(q, centroids, vecs, ids, offsets, nprobe, k, m, metric, attr_ids, attr_vals, S=None, mode="allow", keep=None):
    """search_grouped(group_size=m)'s expected result: the lists O.coarse ranks (None: every list)"""
    return scan(q, vecs, ids, offsets, GY.probed(q, centroids, offsets, nprobe, metric), k, m, metric, attr_ids, attr_vals, S, mode, keep)


def group_counts(q, vecs, ids, offsets, pids, metric, attr_ids, attr_vals):
    """per query {group value: candidates of that group} -- for a test's assertions on its own inputs"""
    rowval, rowhas = GY.row_values(ids, attr_ids, attr_vals)
    lims, rows, val = GY.candidates(q, vecs, ids, offsets, pids, metric)
    out = []
    for i in range(lims.shape[0] - 1):
        r, v = rows[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
        r = r[rowhas[r] & ~np.isnan(v)]
        u, n = np.unique(rowval[r], return_counts=True)
        out.append(dict(zip(u.tolist(), n.tolist())))
    return out
