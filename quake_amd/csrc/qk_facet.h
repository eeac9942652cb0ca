// qk_facet.h -- what qk_facet.hip (facet counts, facet statistics) and qk_order.hip (ordered search) share: the sweep over the keys
// of an emission pass in slices of FC_SLICE keys, its parameters and the hit test (not part of the C ABI).
#pragma once
#include "qk_attr.h"

#include "qk_device.h"

constexpr int FC_SLICE = 1024;      // keys per workgroup step: 256 threads x 4 (the decomposition of GROUPED_FOR_EACH_KEY)

struct FacetParams {
    const uint32_t *keys;
    const int64_t *pair_base;  // [npairs + 1]
    const int64_t *pids;       // [nq][P] or nullptr (pair r -> list r)
    const int64_t *pt_off;
    const uint16_t *mask;      // row mask of a filter, or nullptr
    const uint16_t *has[QK_MAX_FACET_COLS];   // has-value mask of every column
    const int64_t *rowval[QK_MAX_FACET_COLS]; // its value per arena row
    unsigned long long *tvals; // [C][ng][T + 1]: the tables of the query group g0 .. g0 + ng of the pass
    uint32_t *tcnt;            // [C][ng][T + 1]
    uint32_t *total;           // [nq]
    uint32_t *missing;         // [C][nq]
    int64_t nq, g0, ng;
    int P, Sg, C;
    uint32_t tmask;            // T - 1 of the reserved tables: the stride of a table is T + 1 slots
    uint32_t key_lo, key_hi;
    int64_t max_ids;           // the largest number of ids with a value among the call's columns
};

// F for a sweep over the whole pass p (one group): every field set, no tables, total and missing still to be placed in the
// caller's bytes of the pass; the entries of has / rowval behind column C repeat column 0.  S: slices a query can have
inline void facet_params_fill(FacetParams &F, const qk_emit_pass &p, const qk_store *s, const uint16_t *mask, qk_attr_data *const *cols, int C,
                              uint32_t key_lo, uint32_t key_hi, int P, int64_t S) {
    F.keys = p.keys;
    F.pair_base = p.pair_base;
    F.pids = p.pids;
    F.pt_off = s->d_off;
    F.mask = mask;
    for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
        F.has[c] = cols[c < C ? c : 0]->rv_has;
        F.rowval[c] = cols[c < C ? c : 0]->rv_vals;
    }
    F.tvals = nullptr;
    F.tcnt = nullptr;
    F.total = nullptr;
    F.missing = nullptr;
    F.nq = p.nq;
    F.g0 = 0;
    F.ng = p.nq;
    F.P = P;
    F.Sg = qk_emit_sg(S, p.nq);
    F.C = C;
    F.tmask = 0;
    F.key_lo = key_lo;
    F.key_hi = key_hi;
    F.max_ids = 0;
}

// The slots a query's tables USE of the T + 1 reserved ones: the power of two >= max(16, 2 * min(hits of the query, max_ids)),
// known once the hits are counted (k_facet_hits) and never more than T -- a query has no more distinct values than hits.  Clearing,
// counting and selecting touch these slots only, so a call costs what its hits cost, not what the largest list of the store would.
// (Also evaluated on the host by multi-vector search, which lays its tables out by it: qk_maxsim.hip.)
__host__ __device__ __forceinline__ uint32_t facet_used_mask(uint64_t hits, int64_t max_ids, uint32_t tmask) {
    const uint64_t ids = (uint64_t)(max_ids > 1 ? max_ids : 1);
    const uint64_t distinct = hits < ids ? hits : ids;
    uint64_t T = 16;
    while (T < 2 * distinct) T <<= 1;
    return (uint32_t)(T - 1 < (uint64_t)tmask ? T - 1 : (uint64_t)tmask);
}

__device__ __forceinline__ uint32_t facet_hash(unsigned long long v) {  // (the 64-bit finaliser of MurmurHash3, as grouped_hash)
    v ^= v >> 33;
    v *= 0xff51afd7ed558ccdull;
    v ^= v >> 33;
    v *= 0xc4ceb9fe1a85ec53ull;
    v ^= v >> 33;
    return (uint32_t)v;
}

// is the key at absolute position pos a hit (k_range_count's test); *row: its arena row when it passed the key interval
__device__ __forceinline__ bool facet_hit(const FacetParams &F, const int64_t *pbase, const int64_t *qpids, int64_t pos, int64_t lim, int64_t *row) {
    const uint32_t key = pos < lim ? F.keys[pos] : 0xFFFFFFFFu;
    bool hit = pos < lim && key >= F.key_lo && key <= F.key_hi;  // (0xFFFFFFFF lies outside every interval)
    *row = 0;
    if (hit) {
        *row = emit_key_row(pbase, qpids, F.P, F.pt_off, pos);
        if (F.mask) hit = (F.mask[*row >> 4] >> (*row & 15)) & 1;
    }
    return hit;
}
