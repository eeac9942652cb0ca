// qk_attr.h -- what qk_filter.hip and qk_attr.hip share: the filter object (id set or predicate) and the device data of an
// attribute column (not part of the C ABI).
#pragma once
#include "qk_internal.h"

#include <memory>

// Device data of one column, shared by the qk_attr handle and every predicate filter that names it (a filter keeps answering
// after qk_attr_destroy).  One of the two layouts is live: the direct table (t_*) or the sorted pairs (s_*).
struct qk_attr_data {
    uint64_t serial = 0;     // unique per column of the process
    uint64_t version = 0;    // bumped by every set / unset
    uint64_t store_uid = 0;
    int device = 0;
    int layout = QK_ATTR_TABLE;
    int64_t n_ids = 0;       // ids that have a value
    int64_t max_id = -1;     // largest of them
    // direct table: t_vals[id] and bit id of t_bits, for id < t_cap (t_cap a multiple of 32)
    int64_t *t_vals = nullptr;
    uint32_t *t_bits = nullptr;
    int64_t t_cap = 0;
    std::vector<uint32_t> h_bits;  // host mirror of t_bits: which ids are new, how many there are, the largest
    // sorted pairs: s_ids ascending, s_vals next to them
    int64_t *s_ids = nullptr, *s_vals = nullptr;
    int64_t s_cap = 0;
    std::vector<int64_t> h_ids, h_vals;  // host mirror of the pairs: an upsert merges into it and uploads
    // staging of a table update (ids, values, word numbers, words), grown geometrically
    char *stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t upd_ev = nullptr;  // behind the last update, on upd_stream
    hipStream_t upd_stream = nullptr;
    bool updated = false;
    // grouped search (qk_grouped.hip): the column's value of every arena row of the store -- rv_vals[row] and a has-value mask in
    // the filter's layout, one 16-bit word per 16-row tile -- stamped with what they were derived from and re-derived in front of
    // a grouped call when a stamp moved
    int64_t *rv_vals = nullptr;
    uint16_t *rv_has = nullptr;
    int64_t rv_cap = 0;              // rows the arrays hold
    bool rv_built = false;
    uint64_t rv_store_version = 0, rv_col_version = 0;
    int64_t rv_cap_rows = 0;
    int64_t rv_builds = 0;           // derivations so far (qk_attr_group_info)
    hipEvent_t rv_ev = nullptr;      // behind the last derivation, on the stream of rv_ctx
    qk_ctx *rv_ctx = nullptr;
    ~qk_attr_data();
};

struct qk_attr {
    std::shared_ptr<qk_attr_data> d;
    qk_ctx *ctx = nullptr;  // the store's context: updates are enqueued on its stream
};

// ---- the lookup ---------------------------------------------------------------------------------------------------------------
struct AttrCol {
    const int64_t *vals;   // table: [n] by id; sorted: [n] next to ids
    const uint32_t *bits;  // table: presence, bit (id & 31) of word id >> 5
    const int64_t *ids;    // sorted: [n] ascending
    int64_t n;             // table: ids covered (>= 32); sorted: pairs (>= 1)
    int layout;
};

static inline AttrCol col_of(const qk_attr_data &d) {
    AttrCol c;
    if (d.layout == QK_ATTR_TABLE) c = AttrCol{d.t_vals, d.t_bits, nullptr, d.t_cap, QK_ATTR_TABLE};
    else c = AttrCol{d.s_vals, nullptr, d.s_ids, d.n_ids, QK_ATTR_SORTED};
    return c;
}

// (false after an update that failed half way, see "Errors" above: no kernel is given such a column)
static inline bool col_usable(const AttrCol &c) { return c.vals && c.n >= 1 && (c.layout == QK_ATTR_TABLE ? c.bits != nullptr : c.ids != nullptr); }

// U ids looked up at once: every load of a step is asked for before the first is used (a lookup is a chain of dependent loads and
// a mask build has nothing else to hide them behind).  live[u] == false: the loads go to element 0 and the result is "no value".
template <int U>
__device__ __forceinline__ void attr_lookup(const AttrCol &c, const int64_t (&id)[U], const bool (&live)[U], int64_t (&v)[U], bool (&has)[U]) {
    if (c.layout == QK_ATTR_TABLE) {
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool in = live[u] && (uint64_t)id[u] < (uint64_t)c.n;  // (a negative id is a huge unsigned one)
            const int64_t i = in ? id[u] : 0;
            w[u] = c.bits[i >> 5];
            v[u] = c.vals[i];
            has[u] = in;
        }
#pragma unroll
        for (int u = 0; u < U; u++) has[u] = has[u] && ((w[u] >> (id[u] & 31)) & 1u);
    } else {
        // the last element <= id, all U searches in step: the answer stays in [base, base + len), every probe lies inside [0, n)
        int64_t base[U];
#pragma unroll
        for (int u = 0; u < U; u++) base[u] = 0;
        for (int64_t len = c.n; len > 1;) {
            const int64_t half = len >> 1;
            int64_t k[U];
#pragma unroll
            for (int u = 0; u < U; u++) k[u] = c.ids[base[u] + half];
#pragma unroll
            for (int u = 0; u < U; u++) base[u] += (live[u] && k[u] <= id[u]) ? half : 0;
            len -= half;
        }
        int64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            k[u] = c.ids[base[u]];
            v[u] = c.vals[base[u]];
        }
#pragma unroll
        for (int u = 0; u < U; u++) has[u] = live[u] && k[u] == id[u];
    }
}


enum { QK_FILTER_KIND_IDS = 0, QK_FILTER_KIND_WHERE = 1, QK_FILTER_KIND_EXPR = 2 };

struct qk_filter_clause {
    std::shared_ptr<qk_attr_data> col;
    int op = QK_OP_RANGE;
    int64_t a = 0, b = 0;
    uint64_t col_version = 0;  // stamp: the column's version the mask was derived for
    int64_t set_off = 0, set_n = 0;  // (expression, the set ops) the clause's slice of qk_filter::d_sets
};

struct qk_filter {
    uint64_t serial = 0;     // unique per filter object of the process: a freed and re-allocated handle is another filter
    uint64_t store_uid = 0;  // the store it was made for (never dereferenced: the store may be destroyed first)
    int device = 0;
    int kind = QK_FILTER_KIND_IDS;
    int mode = QK_FILTER_ALLOW;
    int64_t n_ids = 0;
    int64_t *d_ids = nullptr;  // [n_ids] ascending, no duplicates (id set)
    std::vector<qk_filter_clause> clauses;  // (predicate; expression: the terms one after the other)
    std::vector<int> term_end;              // (expression) term t is the clauses [term_end[t - 1], term_end[t])
    int64_t *d_sets = nullptr;              // (expression) [max(sets_len, 1)] the clauses' value sets, each ascending and distinct
    int64_t sets_len = 0;
    uint16_t *mask = nullptr;  // [mask_words] one word per arena tile
    int64_t mask_words = 0;    // capacity
    bool built = false;
    uint64_t version = 0;      // stamp: the store's version and arena capacity the mask was derived for
    int64_t cap_rows = 0;
    int64_t rebuilds = 0;      // builds after the first
    unsigned long long *d_allowed = nullptr;  // [1] candidates of the last build
    hipEvent_t built_ev = nullptr;            // behind the last build, on the stream that ran it
    qk_ctx *built_ctx = nullptr;
    // adaptive probing (qk_search_filtered_adaptive): candidates per LIST NUMBER of the store -- the popcount of the mask words of
    // the list's extent -- derived from the mask by the first adaptive call behind a mask build (every build drops them), on that
    // call's stream; nobody else allocates or reads them
    int32_t *counts = nullptr;  // [counts_cap]
    int64_t counts_cap = 0;
    bool counts_built = false;
    hipEvent_t counts_ev = nullptr;  // behind the last derivation, on the stream of counts_ctx
    qk_ctx *counts_ctx = nullptr;
    // exact search (qk_search_filtered_exact): the candidate rows gathered into a private store of ONE list -- rows 0 .. n - 1 of its
    // arena in ascending arena-row order of the source, norms and ids copied bit for bit -- which the flat search then takes like
    // any one-list store.  The life cycle of `counts`: derived from the mask by the first exact call behind a mask build (every
    // build drops it: cand_built; the arena is kept and grown geometrically), on that call's stream; nobody else allocates or
    // reads it.  Its id mirror on the host stays empty: no id travels to the host
    qk_store *cand = nullptr;
    bool cand_built = false;
    int64_t cand_builds = 0;        // derivations so far (qk_filter_exact_info)
    int64_t cand_rows = -1;         // candidates of the last mask build, read from d_allowed once per build (-1: not read yet)
    hipEvent_t cand_ev = nullptr;   // behind the last derivation, on the stream of cand_ctx
    qk_ctx *cand_ctx = nullptr;
    // exact search per query (qk_search_filtered_exact_batch): the list of the store's candidate pool that holds a copy of the same
    // rows, -1 = none.  The pool is found through store_uid and knows the slot's owner by serial; every mask build and
    // qk_filter_destroy give the slot back
    int64_t pool_slot = -1;
};

// qk_filter.hip
uint64_t qk_filter_next_serial();
// the first mask of a new filter, on the store's context (the table is synced first)
int qk_filter_first_build(qk_store *s, qk_filter *f);
// qk_attr.hip: the predicate sibling of k_filter_build on ctx's stream (mask and counter already cleared), behind the columns' last
// updates; stamps the clauses with their columns' versions
int qk_launch_filter_build_where(qk_ctx *ctx, qk_store *s, qk_filter *f);
// the same for an expression filter (k_filter_build_expr)
int qk_launch_filter_build_expr(qk_ctx *ctx, qk_store *s, qk_filter *f);
// are the clauses' stamps those of their columns (both predicate kinds)
bool qk_filter_where_current(const qk_filter *f);

// qk_grouped.hip: rv_vals / rv_has of the column brought up to date for the store as it is (the table has been synced) on ctx's
// stream, and the slots of a query's open-addressing table: the power of two >= max(16, 2 * min(per_query_ub, n_ids))
int qk_rowvals_ensure(qk_ctx *ctx, qk_store *s, qk_attr_data &d);
int64_t qk_grouped_table_slots(int64_t per_query_ub, int64_t n_ids);
