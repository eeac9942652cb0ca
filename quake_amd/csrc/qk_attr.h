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
    ~qk_attr_data();
};

enum { QK_FILTER_KIND_IDS = 0, QK_FILTER_KIND_WHERE = 1 };

struct qk_filter_clause {
    std::shared_ptr<qk_attr_data> col;
    int op = QK_OP_RANGE;
    int64_t a = 0, b = 0;
    uint64_t col_version = 0;  // stamp: the column's version the mask was derived for
};

struct qk_filter {
    uint64_t serial = 0;     // unique per filter object of the process: a freed and re-allocated handle is another filter
    uint64_t store_uid = 0;  // the store it was made for (never dereferenced: the store may be destroyed first)
    int device = 0;
    int kind = QK_FILTER_KIND_IDS;
    int mode = QK_FILTER_ALLOW;
    int64_t n_ids = 0;
    int64_t *d_ids = nullptr;  // [n_ids] ascending, no duplicates (id set)
    std::vector<qk_filter_clause> clauses;  // (predicate)
    uint16_t *mask = nullptr;  // [mask_words] one word per arena tile
    int64_t mask_words = 0;    // capacity
    bool built = false;
    uint64_t version = 0;      // stamp: the store's version and arena capacity the mask was derived for
    int64_t cap_rows = 0;
    int64_t rebuilds = 0;      // builds after the first
    unsigned long long *d_allowed = nullptr;  // [1] candidates of the last build
    hipEvent_t built_ev = nullptr;            // behind the last build, on the stream that ran it
    qk_ctx *built_ctx = nullptr;
};

// qk_filter.hip
uint64_t qk_filter_next_serial();
// the first mask of a new filter, on the store's context (the table is synced first)
int qk_filter_first_build(qk_store *s, qk_filter *f);
// qk_attr.hip: the predicate sibling of k_filter_build on ctx's stream (mask and counter already cleared), behind the columns' last
// updates; stamps the clauses with their columns' versions
int qk_launch_filter_build_where(qk_ctx *ctx, qk_store *s, qk_filter *f);
// are the clauses' stamps those of their columns
bool qk_filter_where_current(const qk_filter *f);
