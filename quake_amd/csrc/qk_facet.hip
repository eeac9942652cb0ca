// qk_facet.hip -- facet counts: per query, how many hits of a range call carry each value of up to QK_MAX_FACET_COLS attribute
// columns, and the n_values most frequent values of every column (include/quake_hip.h, "facet counts").
//
// The expensive half is the key-emission scan, run pass by pass by qk_emit_passes (qk_dense.hip) exactly as for range search; the
// hit test is k_range_count's: the key inside the closed interval the host derived from the radius (qk_range_key_bounds) and the
// filter's mask bit of the arena row.  This file's device work, per pass of queries, over one open-addressing table per
// (column, query).  The tables are RESERVED by the grouped rule (T + 1 slots each, T from the largest list of the store) for as
// many queries as fit QK_GROUPED_PASS_BYTES -- a pass's queries go through them group after group, so the emission keeps range
// search's pass size -- but a query USES only the power of two >= max(16, 2 * min(its hits, ids that have a value)) of its slots
// (facet_used_mask).  Per pass k_facet_hits, then per group k_facet_clear, k_facet_count, k_facet_select:
//   k_facet_hits    the hits of every query (ballot + popcount per wave, one atomic add per wave): total
//   k_facet_clear   the used slots of every table: value words all ones, 32-bit counters 0
//   k_facet_count   one sweep over the pass's keys serves every column of the call: per column a hit goes to the query's missing
//                   counter or to the counter of its value's slot (found or claimed like k_grouped_claim: atomicCAS on the value
//                   word, linear probing, at most as many probes as slots) with an atomic add per hit; QK_FACET_WAVE_AGG=1 adds
//                   equal values of a wave up in registers first (measured, not shipped)
//   k_facet_select  one workgroup per (column, query): the occupied slots are compacted to the front of the table, then the n_values
//                   smallest under the 96-bit key (~count, value ^ sign bit) -- count descending, value ascending signed -- are
//                   selected exactly (most significant byte first) and sorted in LDS.  Values are distinct, so keys are: the result
//                   does not depend on which slot a value landed in
// No thread waits for another and every loop is bounded.  Only integer additions decide a counter, so the result is a pure function
// of the store, the columns and the call.  The value whose bits are all ones (-1) is the table's empty marker: it owns the slot
// behind the used ones.
// Second part (behind facet_call): facet statistics -- count, min, max, exact sum and fixed-edge histograms over the same hits, one
// sweep per pass and no table (k_facet_stats, k_facet_stats_finish).
// The host side of both parts is their kernels plus one description each: facet_call / facet_stats_call state the call for
// qk_emit_run (qk_emit.hip), the host body of every entry point on the emission scan, and facet_device / facet_stats_device hang
// the launches into qk_emit_device's skeleton.  FacetParams is filled in one place (facet_params_fill, qk_facet.h).
#include "qk_facet.h"

#include <cstring>

// 0 (shipped): every hit adds 1 to its slot with its own atomic; 1: equal values of a wave are first counted in registers and added
// by one lane.  Measured with scripts/facet_probe.py: at a radius that keeps 1-2 % of the probed rows a wave step
// of 64 keys holds about one hit, there is nothing to add up, and the per-lane form is 1-2 % faster in every case of the probe
#ifndef QK_FACET_WAVE_AGG
#define QK_FACET_WAVE_AGG 0
#endif

namespace {

constexpr unsigned long long FC_EMPTY = ~0ull;
constexpr int FC_AGG_ROUNDS = 4;    // leaders a wave elects per column and step before the lanes that are left add for themselves
constexpr int FC_SEL = QK_MAX_FACET_VALUES;  // entries the selection sorts in LDS

// facet_used_mask (the slots a query's tables USE of the reserved ones) and facet_hash: qk_facet.h

// `add` hits of value v go to v's slot of the table at tv / tc.  Linear probing; the table holds at least twice the values a query
// can meet, so an empty slot ends every chain -- and at most T probes whatever happens: this loop cannot spin.
__device__ __forceinline__ void facet_add(unsigned long long *tv, uint32_t *tc, uint32_t tmask, unsigned long long v, uint32_t add) {
    if (v == FC_EMPTY) {  // the value that looks like an empty slot has a slot of its own
        atomicAdd(&tc[(int64_t)tmask + 1], add);
        return;
    }
    uint32_t h = facet_hash(v) & tmask;
    for (uint32_t n = 0; n <= tmask; n++) {
        unsigned long long cur = __hip_atomic_load(&tv[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == FC_EMPTY) {
            cur = atomicCAS(&tv[h], FC_EMPTY, v);
            if (cur == FC_EMPTY) cur = v;
        }
        if (cur == v) {
            atomicAdd(&tc[h], add);
            return;
        }
        h = (h + 1) & tmask;
    }
}

// blockIdx.x = query * Sg + g: the workgroup takes slices g, g + Sg, ... of its query's segment; every wave runs the same number
// of steps (the ballots below want whole waves), a position behind the segment is no hit.  total[q] = the hits of the query
__global__ __launch_bounds__(256) void k_facet_hits(FacetParams F) {
    const int64_t q = blockIdx.x / F.Sg;
    const int lane = threadIdx.x & 63;
    const int64_t *pbase = F.pair_base + q * F.P;
    const int64_t *qpids = F.pids ? F.pids + q * F.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[F.P];
    uint32_t n_total = 0;  // (wave-uniform)
    for (int64_t s0 = beg + (int64_t)(blockIdx.x - q * F.Sg) * FC_SLICE; s0 < end; s0 += (int64_t)F.Sg * FC_SLICE) {
        const int64_t lim = min(end, s0 + FC_SLICE);
        for (int64_t w0 = s0 + (threadIdx.x & ~63); w0 < lim; w0 += 256) {
            int64_t row;
            n_total += __popcll(__ballot(facet_hit(F, pbase, qpids, w0 + lane, lim, &row)));
        }
    }
    if (lane == 0 && n_total) atomicAdd(&F.total[q], n_total);
}

// blockIdx.x = column * ng + query of the group: the slots the query's table uses become empty (value all ones, counter 0)
__global__ __launch_bounds__(256) void k_facet_clear(FacetParams F) {
    const int64_t q = F.g0 + blockIdx.x % F.ng;
    const int64_t tb = (int64_t)blockIdx.x * ((int64_t)F.tmask + 2);
    const int64_t used = (int64_t)facet_used_mask(F.total[q], F.max_ids, F.tmask) + 2;
    for (int64_t i = threadIdx.x; i < used; i += 256) {
        F.tvals[tb + i] = FC_EMPTY;
        F.tcnt[tb + i] = 0u;
    }
}

// the decomposition of k_facet_hits over the queries of the group; a query without hits is left at once
__global__ __launch_bounds__(256) void k_facet_count(FacetParams F) {
    const int64_t ql = blockIdx.x / F.Sg, q = F.g0 + ql;
    const uint32_t hits = F.total[q];
    if (hits == 0) return;
    const uint32_t umask = facet_used_mask(hits, F.max_ids, F.tmask);
    const int lane = threadIdx.x & 63;
    const int64_t *pbase = F.pair_base + q * F.P;
    const int64_t *qpids = F.pids ? F.pids + q * F.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[F.P];
    const int64_t tstride = (int64_t)F.tmask + 2;
    uint32_t n_missing[QK_MAX_FACET_COLS] = {0, 0, 0, 0};  // (wave-uniform)
    for (int64_t s0 = beg + (int64_t)(blockIdx.x - ql * F.Sg) * FC_SLICE; s0 < end; s0 += (int64_t)F.Sg * FC_SLICE) {
        const int64_t lim = min(end, s0 + FC_SLICE);
        for (int64_t w0 = s0 + (threadIdx.x & ~63); w0 < lim; w0 += 256) {
            int64_t row;
            const bool hit = facet_hit(F, pbase, qpids, w0 + lane, lim, &row);
            const uint64_t hm = __ballot(hit);
            if (hm == 0) continue;
#pragma unroll
            for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
                if (c >= F.C) break;
                const bool has = hit && ((F.has[c][row >> 4] >> (row & 15)) & 1);
                n_missing[c] += __popcll(hm) - __popcll(__ballot(has));
                const unsigned long long v = has ? (unsigned long long)F.rowval[c][row] : 0ull;
                uint32_t add = has ? 1u : 0u;
#if QK_FACET_WAVE_AGG
                bool open = has;  // not yet counted by a leader
                for (int r = 0; r < FC_AGG_ROUNDS; r++) {
                    const uint64_t om = __ballot(open);
                    if (om == 0) break;
                    const int leader = __ffsll((unsigned long long)om) - 1;
                    const unsigned long long lv = __shfl(v, leader);
                    const bool same = open && v == lv;
                    const uint32_t n = __popcll(__ballot(same));
                    if (same) {
                        add = lane == leader ? n : 0u;
                        open = false;
                    }
                }
#endif
                if (add) {
                    const int64_t tb = ((int64_t)c * F.ng + ql) * tstride;
                    facet_add(F.tvals + tb, F.tcnt + tb, umask, v, add);
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < QK_MAX_FACET_COLS; c++)
            if (c < F.C && n_missing[c]) atomicAdd(&F.missing[(int64_t)c * F.nq + q], n_missing[c]);
    }
}

struct FacetSelectParams {
    unsigned long long *tvals;  // [C][ng][T + 1]; compacted in place
    uint32_t *tcnt;             // [C][ng][T + 1]
    const uint32_t *total;      // [nq]
    const uint32_t *missing;    // [C][nq]
    int64_t nq, q0, Q;          // the pass's queries are q0 .. q0 + nq of the call's Q
    int64_t g0, ng;             // the group's are g0 .. g0 + ng of the pass's
    int64_t T1;                 // T + 1: the stride of a table
    int64_t max_ids;
    int n_values;
    int64_t *out_values, *out_counts;    // [C][Q][n_values]
    int64_t *out_distinct, *out_missing; // [C][Q] or nullptr
    int64_t *out_total;                  // [Q] or nullptr
};

// the 96-bit selection key of a (value, count): smaller = more hits, then the smaller signed value
struct FKey {
    uint32_t hi;
    unsigned long long lo;
};
__device__ __forceinline__ FKey facet_key(unsigned long long v, uint32_t c) { return FKey{~c, v ^ 0x8000000000000000ull}; }
__device__ __forceinline__ bool fkey_less(const FKey &a, const FKey &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// byte d (0 = most significant, 11 = least) of a key, and whether the bytes in front of d equal those of p
__device__ __forceinline__ uint32_t fkey_byte(const FKey &k, int d) {
    return d < 4 ? (k.hi >> (24 - 8 * d)) & 255u : (uint32_t)(k.lo >> (56 - 8 * (d - 4))) & 255u;
}
__device__ __forceinline__ bool fkey_prefix(const FKey &k, const FKey &p, int d) {
    if (d == 0) return true;
    if (d <= 4) return d == 4 ? k.hi == p.hi : (k.hi >> (32 - 8 * d)) == (p.hi >> (32 - 8 * d));
    return k.hi == p.hi && (k.lo >> (64 - 8 * (d - 4))) == (p.lo >> (64 - 8 * (d - 4)));
}

// blockIdx.x = column * ng + query of the group
__global__ __launch_bounds__(256) void k_facet_select(FacetSelectParams S) {
    __shared__ uint32_t s_hi[FC_SEL];
    __shared__ unsigned long long s_lo[FC_SEL];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_pick[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = blockIdx.x / S.ng, q = S.g0 + (blockIdx.x - c * S.ng);
    unsigned long long *tv = S.tvals + (int64_t)blockIdx.x * S.T1;
    uint32_t *tc = S.tcnt + (int64_t)blockIdx.x * S.T1;
    // ---- 1. the occupied slots (count > 0; the slot behind the used ones holds the value -1 from k_facet_clear on) to the front,
    //         in any order: a chunk is read into registers before any of it is written, and it is written at or in front of where
    //         it was read
    const int64_t used = (int64_t)facet_used_mask(S.total[q], S.max_ids, (uint32_t)(S.T1 - 2)) + 2;
    uint32_t D = 0;  // (uniform)
    for (int64_t b0 = 0; b0 < used; b0 += 1024) {
        unsigned long long v[4];
        uint32_t n[4];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = b0 + j * 256 + tid;
            n[j] = i < used ? tc[i] : 0u;
            v[j] = i < used ? tv[i] : 0ull;
            mine += n[j] ? 1u : 0u;
        }
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        __syncthreads();  // (the chunk is in registers; s_wave of the previous chunk has been read)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t at = D + incl - mine;
        for (int w = 0; w < wave; w++) at += s_wave[w];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (n[j]) {
                tv[at] = v[j];
                tc[at] = n[j];
                at++;
            }
        D += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
    __syncthreads();  // (the compacted entries are visible to the workgroup)
    // ---- 2. more than FC_SEL entries: the n_values-th smallest key, byte by byte from the top; keys are distinct, so exactly
    //         n_values entries lie at or below it
    const uint32_t want = (uint32_t)S.n_values;
    FKey thr{0xFFFFFFFFu, ~0ull};
    if (D > FC_SEL) {
        FKey pre{0u, 0ull};
        uint32_t need = want;
        for (int d = 0; d < 12; d++) {
            s_hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < D; i += 256) {
                const FKey k = facet_key(tv[i], tc[i]);
                if (fkey_prefix(k, pre, d)) atomicAdd(&s_hist[fkey_byte(k, d)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t run = 0, b = 0;
                for (; b < 255; b++) {
                    if (run + s_hist[b] >= need) break;
                    run += s_hist[b];
                }
                s_pick[0] = b;
                s_pick[1] = need - run;
            }
            __syncthreads();
            const uint32_t b = s_pick[0];
            need = s_pick[1];
            if (d < 4) pre.hi |= b << (24 - 8 * d);
            else pre.lo |= (unsigned long long)b << (56 - 8 * (d - 4));
            __syncthreads();  // (s_pick and s_hist are rewritten by the next byte)
        }
        thr = pre;
    }
    // ---- 3. the survivors into LDS (at most FC_SEL of them), padded with the key no entry has, sorted ascending
    if (tid == 0) s_n = 0;
    s_hi[tid] = 0xFFFFFFFFu;
    s_lo[tid] = ~0ull;
    __syncthreads();
    for (uint32_t i = tid; i < D; i += 256) {
        const FKey k = facet_key(tv[i], tc[i]);
        if (!fkey_less(thr, k)) {
            const uint32_t at = atomicAdd(&s_n, 1u);
            if (at < FC_SEL) {
                s_hi[at] = k.hi;
                s_lo[at] = k.lo;
            }
        }
    }
    __syncthreads();
    for (int k = 2; k <= FC_SEL; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = tid ^ j;
            if (o > tid) {
                const FKey a{s_hi[tid], s_lo[tid]}, b{s_hi[o], s_lo[o]};
                const bool up = (tid & k) == 0;
                if (up ? fkey_less(b, a) : fkey_less(a, b)) {
                    s_hi[tid] = b.hi;
                    s_lo[tid] = b.lo;
                    s_hi[o] = a.hi;
                    s_lo[o] = a.lo;
                }
            }
            __syncthreads();
        }
    // ---- 4. the answer: entries behind the distinct values are padding (value 0, count 0)
    const int64_t oq = c * S.Q + S.q0 + q;
    if (tid < S.n_values) {
        const bool real = (uint32_t)tid < D && s_hi[tid] != 0xFFFFFFFFu;
        S.out_values[oq * S.n_values + tid] = real ? (int64_t)(s_lo[tid] ^ 0x8000000000000000ull) : 0;
        S.out_counts[oq * S.n_values + tid] = real ? (int64_t)(~s_hi[tid]) : 0;
    }
    if (tid == 0) {
        if (S.out_distinct) S.out_distinct[oq] = D;
        if (S.out_missing) S.out_missing[oq] = S.missing[c * S.nq + q];
        if (S.out_total && c == 0) S.out_total[S.q0 + q] = S.total[q];
    }
}

// bytes of the tables one query accounts for: 12 per slot of every column
inline int64_t facet_table_bytes(int64_t T, int C) { return (int64_t)C * (T + 1) * 12; }

// the device half of facet counts; o: the call's output table on the device -- values, counts, distinct, missing, total
int facet_device(const qk_emit_call &c, qk_emit_env &e, int n_values, const qk_emit_out *o) {
    qk_store *s = c.s;
    qk_attr_data *const *cols = c.cols;
    const int C = c.n_cols, P = e.P;
    const int64_t Q = e.a.Q;
    hipStream_t st = c.ctx->stream;
    int64_t *out_values = (int64_t *)o[0].dev, *out_counts = (int64_t *)o[1].dev, *out_distinct = (int64_t *)o[2].dev;
    int64_t *out_missing = (int64_t *)o[3].dev, *out_total = (int64_t *)o[4].dev;
    qk_emit_stages g;
    g.pad = [&]() -> int {  // no hits
        for (int i = 0; i < 5; i++)
            if (o[i].dev) QK_HIP(hipMemsetAsync(o[i].dev, 0, o[i].bytes, st));
        return QK_OK;
    };
    int64_t max_ids = cols[0]->n_ids;  // one table size for every column of the call: that of the column with the most values
    for (int i = 1; i < C; i++) max_ids = std::max(max_ids, cols[i]->n_ids);
    // this pipeline's bytes of the call's buffer, sized for the largest pass: [table values] [table counters] [total] [missing]
    int64_t T = 0, S = 0, qt = 1;  // qt: queries whose tables fit QK_GROUPED_PASS_BYTES -- a pass's queries are counted in groups of qt
    size_t o_tcnt = 0, o_total = 0, o_missing = 0;
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        T = qk_grouped_table_slots(per_query_ub, max_ids);
        const int64_t qbytes = facet_table_bytes(T, C);
        if (qbytes > QK_GROUPED_PASS_BYTES)
            QK_FAIL(QK_ERR_UNSUPPORTED, "facet counts: the tables of one query need %lld bytes, more than QK_GROUPED_PASS_BYTES", (long long)qbytes);
        qt = std::max<int64_t>(1, std::min<int64_t>(*qc, QK_GROUPED_PASS_BYTES / qbytes));
        S = (per_query_ub + FC_SLICE - 1) / FC_SLICE;
        if (*qc * S > 0x7FFFFFF0LL || *qc * (int64_t)C > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "facet counts: Q too large");
        const int64_t nslots = qt * C * (T + 1);
        o_tcnt = qk_al256((size_t)nslots * 8);
        o_total = o_tcnt + qk_al256((size_t)nslots * 4);
        o_missing = o_total + qk_al256((size_t)*qc * 4);
        *extra_bytes = o_missing + qk_al256((size_t)*qc * C * 4);
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        // total and missing of the pass (missing lies behind total: one memset); the tables are cleared behind the hit count, as far
        // as they are used (k_facet_clear)
        QK_HIP(hipMemsetAsync(p.extra + o_total, 0, (o_missing - o_total) + (size_t)p.nq * C * 4, st));
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        FacetParams F;
        facet_params_fill(F, p, s, e.mask, cols, C, e.key_lo, e.key_hi, P, S);
        F.tvals = (unsigned long long *)p.extra;
        F.tcnt = (uint32_t *)(p.extra + o_tcnt);
        F.total = (uint32_t *)(p.extra + o_total);
        F.missing = (uint32_t *)(p.extra + o_missing);
        F.tmask = (uint32_t)(T - 1);
        F.max_ids = max_ids;
        hipLaunchKernelGGL(k_facet_hits, dim3((unsigned)(p.nq * F.Sg)), dim3(256), 0, st, F);
        FacetSelectParams L;
        L.tvals = F.tvals;
        L.tcnt = F.tcnt;
        L.total = F.total;
        L.missing = F.missing;
        L.nq = p.nq;
        L.q0 = p.q0;
        L.Q = Q;
        L.T1 = T + 1;
        L.max_ids = max_ids;
        L.n_values = n_values;
        L.out_values = out_values;
        L.out_counts = out_counts;
        L.out_distinct = out_distinct;
        L.out_missing = out_missing;
        L.out_total = out_total;
        // the pass's queries in groups whose tables fit the workspace: the same tables serve one group after the other
        for (int64_t g0 = 0; g0 < p.nq; g0 += qt) {
            F.g0 = L.g0 = g0;
            F.ng = L.ng = std::min(qt, p.nq - g0);
            F.Sg = qk_emit_sg(S, F.ng);
            hipLaunchKernelGGL(k_facet_clear, dim3((unsigned)(F.ng * C)), dim3(256), 0, st, F);
            hipLaunchKernelGGL(k_facet_count, dim3((unsigned)(F.ng * F.Sg)), dim3(256), 0, st, F);
            hipLaunchKernelGGL(k_facet_select, dim3((unsigned)(F.ng * C)), dim3(256), 0, st, L);
        }
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    return qk_emit_device(c, e, g);
}

// the checks both facet calls make of their columns, behind those of n_cols; fills c.cols / c.n_cols
int facet_check_cols(qk_emit_call &c, qk_attr *const *facet_by, int n_cols) {
    if (!facet_by) QK_FAIL(QK_ERR_INVALID, "%s: facet_by is null", c.who);
    for (int i = 0; i < n_cols; i++) {
        if (!facet_by[i]) QK_FAIL(QK_ERR_INVALID, "%s: facet column %d is null", c.who, i);
        c.cols[i] = facet_by[i]->d.get();
        if (c.cols[i]->store_uid != c.s->uid) QK_FAIL(QK_ERR_INVALID, "%s: facet column %d belongs to another store", c.who, i);
    }
    c.n_cols = n_cols;
    return QK_OK;
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int facet_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
               int metric, float radius, qk_filter *filter, qk_attr *const *facet_by, int n_cols, int n_values, int64_t *out_values,
               int64_t *out_counts, int64_t *out_distinct, int64_t *out_missing, int64_t *out_total, int mem, qk_timing *timing) {
    // [values] [counts] [distinct] [missing] [total]
    const size_t bv = (size_t)n_cols * Q * n_values * 8, bc = (size_t)n_cols * Q * 8;
    qk_emit_out outs[5] = {{out_values, bv, true}, {out_counts, bv, true}, {out_distinct, bc, false}, {out_missing, bc, false},
                           {out_total, (size_t)Q * 8, false}};
    qk_emit_call c;
    c.who = who;
    c.pipeline = "facet counts";
    c.label = "k_scan (facet)";
    c.label_wide = "k_scan_wide (facet)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.Q = Q, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.radius = radius, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 5;
    c.check = [&]() -> int {
        if (n_cols < 1) QK_FAIL(QK_ERR_INVALID, "%s: n_cols=%d must be at least 1", who, n_cols);
        if (n_cols > QK_MAX_FACET_COLS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: n_cols=%d exceeds QK_MAX_FACET_COLS=%d", who, n_cols, QK_MAX_FACET_COLS);
        if (n_values < 1) QK_FAIL(QK_ERR_INVALID, "%s: n_values=%d must be at least 1", who, n_values);
        if (n_values > QK_MAX_FACET_VALUES)
            QK_FAIL(QK_ERR_UNSUPPORTED, "%s: n_values=%d exceeds QK_MAX_FACET_VALUES=%d", who, n_values, QK_MAX_FACET_VALUES);
        return facet_check_cols(c, facet_by, n_cols);
    };
    c.device = [&](qk_emit_env &e) -> int { return facet_device(c, e, n_values, outs); };
    return qk_emit_run(c);
}

// ---- second part: facet statistics (include/quake_hip.h, "facet statistics") ----------------------------------------
// Count, minimum, maximum, exact sum and a histogram with fixed bucket edges of every column over the same hits.  Fixed edges need no
// table sized by hits, no group loop over a pass's queries and no selection: per pass ONE sweep over the emitted keys, k_facet_stats,
// for all columns and all queries, then k_facet_stats_finish.  The accumulators of a pass -- [total] [missing] [sum_lo] [sum_hi]
// [max] [min] [bins] -- lie in the caller's bytes of qk_emit_passes; all start at zero bytes except min, which starts at all ones
// (two memsets on the stream, in front of the emission).  min / max work on sign-flipped words (v ^ 2^63 orders the signed values
// as unsigned ones), so their identities are all ones and zero.  The sum of a query's values is kept as two 64-bit words: SL, the
// low 32 bits of every value added as unsigned, and SH, the high 32 bits added as signed; a query has fewer than 2^30 keys, so
// SL < 2^62 and |SH| < 2^61, and SH * 2^32 + SL is the exact sum.
//
// QK_FACET_STATS_HIT_ATOMICS: 0 (shipped): a lane accumulates in registers, a workgroup reduces through shuffles and LDS and issues
// one global atomic per statistic; 1: every hit issues its global atomics itself (min, max, two adds per column) -- the variant
// DESIGN.md 5.17 prices.  The histogram goes through the workgroup's LDS bins in both.
#ifndef QK_FACET_STATS_HIT_ATOMICS
#define QK_FACET_STATS_HIT_ATOMICS 0
#endif

constexpr unsigned long long FS_SIGN = 0x8000000000000000ull;
constexpr int FS_BINS = QK_MAX_FACET_EDGES + 1;

struct FacetStatsParams {
    FacetParams F;              // keys, segments, mask, columns, total, missing, nq, P, Sg, C, key interval (the tables are unused)
    const int64_t *edges;       // the call's edges, column after column (device)
    int e_off[QK_MAX_FACET_COLS], n_edges[QK_MAX_FACET_COLS];
    int hist_stride;            // of bins; 0: no column has edges to search (no LDS bins, no global ones)
    unsigned long long *sum_lo, *sum_hi, *vmax, *vmin;  // [C][nq]
    uint32_t *bins;             // [C][nq][hist_stride]
};

__device__ __forceinline__ unsigned long long fs_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ unsigned long long fs_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ unsigned long long fs_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor(v, off);
    return v;
}

// b(v) = |{i : e_i <= v}| over E <= 255 ascending edges in LDS: the branch-free binary search of k_filter_build_expr's set
// membership, 8 steps; the probe index stays below 255 and is read only where it is below E
__device__ __forceinline__ int fs_bucket(const long long *ed, int E, long long v) {
    int b = 0;
#pragma unroll
    for (int step = 128; step > 0; step >>= 1) {
        const int i = b + step - 1;
        const bool le = i < E && ed[min(i, E - 1)] <= v;
        b += le ? step : 0;
    }
    return b;
}

// The decomposition of k_facet_hits: blockIdx.x = query * Sg + g, slices of FC_SLICE keys, whole waves per step.  Nothing global is
// written inside the key loop (QK_FACET_STATS_HIT_ATOMICS=0); no thread waits for another, every loop is bounded
__global__ __launch_bounds__(256) void k_facet_stats(FacetStatsParams S) {
    __shared__ long long s_edges[QK_MAX_FACET_COLS * QK_MAX_FACET_EDGES];
    __shared__ uint32_t s_bins[QK_MAX_FACET_COLS * FS_BINS];
    __shared__ unsigned long long s_red[4][QK_MAX_FACET_COLS][4];
    __shared__ uint32_t s_cnt[4][QK_MAX_FACET_COLS + 1];
    const FacetParams &F = S.F;
    const int64_t q = blockIdx.x / F.Sg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t *pbase = F.pair_base + q * F.P;
    const int64_t *qpids = F.pids ? F.pids + q * F.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[F.P];
    const int64_t first = beg + (int64_t)(blockIdx.x - q * F.Sg) * FC_SLICE;
    if (first >= end) return;  // (the whole workgroup: it has no slice)
    const bool bins = S.hist_stride > 0;
    if (bins) {
#pragma unroll
        for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
            if (c >= F.C) break;
            for (int i = tid; i < S.n_edges[c]; i += 256) s_edges[c * QK_MAX_FACET_EDGES + i] = S.edges[S.e_off[c] + i];
        }
        for (int i = tid; i < QK_MAX_FACET_COLS * FS_BINS; i += 256) s_bins[i] = 0u;
        __syncthreads();
    }
    uint32_t n_total = 0, n_missing[QK_MAX_FACET_COLS] = {0, 0, 0, 0};  // (wave-uniform)
    unsigned long long vmin[QK_MAX_FACET_COLS], vmax[QK_MAX_FACET_COLS], sl[QK_MAX_FACET_COLS], sh[QK_MAX_FACET_COLS];
#pragma unroll
    for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
        vmin[c] = ~0ull;
        vmax[c] = sl[c] = sh[c] = 0ull;
    }
    for (int64_t s0 = first; s0 < end; s0 += (int64_t)F.Sg * FC_SLICE) {
        const int64_t lim = min(end, s0 + FC_SLICE);
        for (int64_t w0 = s0 + (tid & ~63); w0 < lim; w0 += 256) {
            int64_t row;
            const bool hit = facet_hit(F, pbase, qpids, w0 + lane, lim, &row);
            const uint64_t hm = __ballot(hit);
            if (hm == 0) continue;
            n_total += __popcll(hm);
#pragma unroll
            for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
                if (c >= F.C) break;
                const bool has = hit && ((F.has[c][row >> 4] >> (row & 15)) & 1);
                n_missing[c] += __popcll(hm) - __popcll(__ballot(has));
                if (has) {
                    const long long v = (long long)F.rowval[c][row];
                    const unsigned long long u = (unsigned long long)v ^ FS_SIGN;
                    const unsigned long long lo = (unsigned long long)(uint32_t)v, hi = (unsigned long long)(v >> 32);  // (hi: sign-extended)
#if QK_FACET_STATS_HIT_ATOMICS
                    const int64_t a = (int64_t)c * F.nq + q;
                    atomicMin(&S.vmin[a], u);
                    atomicMax(&S.vmax[a], u);
                    atomicAdd(&S.sum_lo[a], lo);
                    atomicAdd(&S.sum_hi[a], hi);
#else
                    vmin[c] = min(vmin[c], u);
                    vmax[c] = max(vmax[c], u);
                    sl[c] += lo;
                    sh[c] += hi;
#endif
                    if (bins && S.n_edges[c] > 0)
                        atomicAdd(&s_bins[c * FS_BINS + fs_bucket(s_edges + c * QK_MAX_FACET_EDGES, S.n_edges[c], v)], 1u);
                }
            }
        }
    }
    // ---- the workgroup's statistics: across the wave by shuffles, across the four waves through LDS, one global atomic each
#pragma unroll
    for (int c = 0; c < QK_MAX_FACET_COLS; c++) {
        if (c >= F.C) break;
        const unsigned long long a = fs_wave_min(vmin[c]), b = fs_wave_max(vmax[c]), l = fs_wave_sum(sl[c]), h = fs_wave_sum(sh[c]);
        if (lane == 0) {
            s_red[wave][c][0] = a;
            s_red[wave][c][1] = b;
            s_red[wave][c][2] = l;
            s_red[wave][c][3] = h;
            s_cnt[wave][1 + c] = n_missing[c];
        }
    }
    if (lane == 0) s_cnt[wave][0] = n_total;
    __syncthreads();  // (also: every LDS add of the key loop has landed)
    if (tid < 4 * F.C) {
        const int c = tid >> 2, k = tid & 3;
        const int64_t a = (int64_t)c * F.nq + q;
        const unsigned long long w0 = s_red[0][c][k], w1 = s_red[1][c][k], w2 = s_red[2][c][k], w3 = s_red[3][c][k];
        if (k == 0) {
            const unsigned long long m = min(min(w0, w1), min(w2, w3));
            if (m != ~0ull) atomicMin(&S.vmin[a], m);
        } else if (k == 1) {
            const unsigned long long m = max(max(w0, w1), max(w2, w3));
            if (m != 0ull) atomicMax(&S.vmax[a], m);
        } else {
            const unsigned long long m = w0 + w1 + w2 + w3;
            if (m != 0ull) atomicAdd(k == 2 ? &S.sum_lo[a] : &S.sum_hi[a], m);
        }
    } else if (tid >= 64 && tid < 64 + 1 + F.C) {
        const int k = tid - 64;
        const uint32_t n = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
        if (n) atomicAdd(k == 0 ? &F.total[q] : &F.missing[(int64_t)(k - 1) * F.nq + q], n);
    }
    if (bins) {
        for (int i = tid; i < F.C * FS_BINS; i += 256) {
            const int c = i / FS_BINS, b = i - c * FS_BINS;
            const uint32_t n = s_bins[i];
            if (n) atomicAdd(&S.bins[((int64_t)c * F.nq + q) * S.hist_stride + b], n);  // (n > 0: b <= n_edges[c] < hist_stride)
        }
    }
}

struct FacetStatsFinishParams {
    const uint32_t *total, *missing;                         // [nq], [C][nq]
    const unsigned long long *sum_lo, *sum_hi, *vmax, *vmin;  // [C][nq]
    const uint32_t *bins;                                    // [C][nq][bin_stride], or nullptr: no column has edges
    int64_t nq, q0, Q;
    int C, bin_stride, hist_stride;                           // hist_stride: of out_hist
    int n_edges[QK_MAX_FACET_COLS];
    int64_t *out_count, *out_missing, *out_min, *out_max, *out_sum_lo, *out_sum_hi;  // [C][Q] or nullptr
    int64_t *out_hist;                                       // [C][Q][hist_stride] or nullptr
    int64_t *out_total;                                      // [Q]
};

// thread i < C * nq: the statistics of (column, query) i; thread i < C * nq * hist_stride: one bucket of the histogram
__global__ __launch_bounds__(256) void k_facet_stats_finish(FacetStatsFinishParams L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)L.C * L.nq) {
        const int64_t c = i / L.nq, q = i - c * L.nq, oq = c * L.Q + L.q0 + q;
        const int64_t tot = L.total[q], mis = L.missing[i];
        if (L.out_count) L.out_count[oq] = tot - mis;
        if (L.out_missing) L.out_missing[oq] = mis;
        if (L.out_min) L.out_min[oq] = (int64_t)(L.vmin[i] ^ FS_SIGN);
        if (L.out_max) L.out_max[oq] = (int64_t)(L.vmax[i] ^ FS_SIGN);
        // SH * 2^32 + SL as a 128-bit number: SH << 32 has the low word SH << 32 and the high word SH >> 32 (arithmetic)
        const unsigned long long sl = L.sum_lo[i], shl = L.sum_hi[i] << 32, lo = shl + sl;
        if (L.out_sum_lo) L.out_sum_lo[oq] = (int64_t)lo;
        if (L.out_sum_hi) L.out_sum_hi[oq] = ((int64_t)L.sum_hi[i] >> 32) + (lo < shl ? 1 : 0);
        if (c == 0) L.out_total[L.q0 + q] = tot;
    }
    if (L.out_hist && i < (int64_t)L.C * L.nq * L.hist_stride) {
        const int64_t cq = i / L.hist_stride, b = i - cq * L.hist_stride;
        const int64_t c = cq / L.nq, q = cq - c * L.nq;
        int64_t n = 0;
        if (L.n_edges[c] == 0) n = b == 0 ? (int64_t)L.total[q] - (int64_t)L.missing[cq] : 0;  // the single bucket: count
        else if (b <= L.n_edges[c]) n = L.bins[cq * L.bin_stride + b];
        L.out_hist[(c * L.Q + L.q0 + q) * L.hist_stride + b] = n;
    }
}

__global__ __launch_bounds__(256) void k_facet_stats_fill(int64_t *p, int64_t n, int64_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

struct FacetStatsOut {
    int64_t *count, *missing, *vmin, *vmax, *sum_lo, *sum_hi, *hist, *total;
};

// the device half of facet statistics; o: the call's outputs on the device (nullptr: not wanted), edges / n_edges: host memory
int facet_stats_device(const qk_emit_call &c, qk_emit_env &e, const int64_t *edges, const int *n_edges, int hist_stride,
                       const FacetStatsOut &o) {
    qk_store *s = c.s;
    const int C = c.n_cols, P = e.P;
    const int64_t Q = e.a.Q;
    hipStream_t st = c.ctx->stream;
    const int64_t CQ = (int64_t)C * Q;
    qk_emit_stages g;
    g.pad = [&]() -> int {  // no hits: zeros, and the identities of min / max
        for (int64_t *p : {o.count, o.missing, o.sum_lo, o.sum_hi})
            if (p) QK_HIP(hipMemsetAsync(p, 0, (size_t)CQ * 8, st));
        if (o.hist) QK_HIP(hipMemsetAsync(o.hist, 0, (size_t)CQ * hist_stride * 8, st));
        QK_HIP(hipMemsetAsync(o.total, 0, (size_t)Q * 8, st));
        if (o.vmin) hipLaunchKernelGGL(k_facet_stats_fill, dim3((unsigned)((CQ + 255) / 256)), dim3(256), 0, st, o.vmin, CQ, INT64_MAX);
        if (o.vmax) hipLaunchKernelGGL(k_facet_stats_fill, dim3((unsigned)((CQ + 255) / 256)), dim3(256), 0, st, o.vmax, CQ, INT64_MIN);
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    int n_all = 0, e_off[QK_MAX_FACET_COLS] = {0, 0, 0, 0}, ne[QK_MAX_FACET_COLS] = {0, 0, 0, 0};
    for (int i = 0; i < C; i++) {
        e_off[i] = n_all;
        ne[i] = n_edges ? n_edges[i] : 0;
        n_all += ne[i];
    }
    // bins are kept only where some column of a wanted histogram has edges to search: the single bucket of E == 0 is the count
    const int bin_stride = o.hist && n_all > 0 ? hist_stride : 0;
    // this pipeline's bytes of the call's buffer, sized for the largest pass:
    // [total] [missing] [sum_lo] [sum_hi] [max] [bins] | [min] | [edges]   (zero bytes | all ones | uploaded once)
    int64_t S = 0;
    size_t o_missing = 0, o_sum_lo = 0, o_sum_hi = 0, o_max = 0, o_bins = 0, o_min = 0, o_edges = 0;
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        const int64_t qbytes = 4 + (int64_t)C * 36 + (int64_t)C * bin_stride * 4;
        *qc = std::max<int64_t>(1, std::min<int64_t>(*qc, QK_GROUPED_PASS_BYTES / qbytes));
        S = (per_query_ub + FC_SLICE - 1) / FC_SLICE;
        if (*qc * S > 0x7FFFFFF0LL || *qc * (int64_t)C > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "facet statistics: Q too large");
        const size_t w = qk_al256((size_t)*qc * C * 8);
        o_missing = qk_al256((size_t)*qc * 4);
        o_sum_lo = o_missing + qk_al256((size_t)*qc * C * 4);
        o_sum_hi = o_sum_lo + w;
        o_max = o_sum_hi + w;
        o_bins = o_max + w;
        o_min = o_bins + qk_al256((size_t)*qc * C * bin_stride * 4);
        o_edges = o_min + w;
        *extra_bytes = o_edges + qk_al256((size_t)n_all * 8);
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        QK_HIP(hipMemsetAsync(p.extra, 0, o_min, st));
        QK_HIP(hipMemsetAsync(p.extra + o_min, 0xFF, (size_t)p.nq * C * 8, st));
        // the edges, once per call: a stream-ordered copy from the caller's pageable memory.  As everywhere in this library
        // (qk_attr.hip, qk_store.hip) it relies on the runtime having staged a pageable source when hipMemcpyAsync returns, so the
        // caller's array may go when the call returns; the host may wait here once, in front of the first emission, never
        // between passes
        if (p.q0 == 0 && bin_stride > 0)
            QK_HIP(hipMemcpyAsync(p.extra + o_edges, edges, (size_t)n_all * 8, hipMemcpyHostToDevice, st));
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        FacetStatsParams T;
        FacetParams &F = T.F;
        facet_params_fill(F, p, s, e.mask, c.cols, C, e.key_lo, e.key_hi, P, S);
        F.total = (uint32_t *)p.extra;
        F.missing = (uint32_t *)(p.extra + o_missing);
        for (int i = 0; i < QK_MAX_FACET_COLS; i++) {
            T.e_off[i] = e_off[i];
            T.n_edges[i] = ne[i];
        }
        T.edges = (const int64_t *)(p.extra + o_edges);
        T.hist_stride = bin_stride;
        T.sum_lo = (unsigned long long *)(p.extra + o_sum_lo);
        T.sum_hi = (unsigned long long *)(p.extra + o_sum_hi);
        T.vmax = (unsigned long long *)(p.extra + o_max);
        T.vmin = (unsigned long long *)(p.extra + o_min);
        T.bins = (uint32_t *)(p.extra + o_bins);
        hipLaunchKernelGGL(k_facet_stats, dim3((unsigned)(p.nq * F.Sg)), dim3(256), 0, st, T);
        FacetStatsFinishParams L;
        L.total = F.total;
        L.missing = F.missing;
        L.sum_lo = T.sum_lo;
        L.sum_hi = T.sum_hi;
        L.vmax = T.vmax;
        L.vmin = T.vmin;
        L.bins = bin_stride > 0 ? T.bins : nullptr;
        L.nq = p.nq;
        L.q0 = p.q0;
        L.Q = Q;
        L.C = C;
        L.bin_stride = bin_stride;
        L.hist_stride = hist_stride;
        for (int i = 0; i < QK_MAX_FACET_COLS; i++) L.n_edges[i] = ne[i];
        L.out_count = o.count;
        L.out_missing = o.missing;
        L.out_min = o.vmin;
        L.out_max = o.vmax;
        L.out_sum_lo = o.sum_lo;
        L.out_sum_hi = o.sum_hi;
        L.out_hist = o.hist;
        L.out_total = o.total;
        const int64_t nthr = (int64_t)C * p.nq * (o.hist ? hist_stride : 1);
        hipLaunchKernelGGL(k_facet_stats_finish, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, L);
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    return qk_emit_device(c, e, g);
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int facet_stats_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P,
                     int nprobe, int metric, float radius, qk_filter *filter, qk_attr *const *facet_by, int n_cols, const int64_t *edges,
                     const int *n_edges, const FacetStatsOut &out, int mem, qk_timing *timing) {
    // six [C][Q] words, [hist], [total]; the histogram's bytes are known once the edges are checked
    const size_t bc = (size_t)n_cols * Q * 8;
    qk_emit_out outs[8] = {{out.count, bc, false},  {out.missing, bc, false}, {out.vmin, bc, false}, {out.vmax, bc, false},
                           {out.sum_lo, bc, false}, {out.sum_hi, bc, false},  {out.hist, 0, false},  {out.total, (size_t)Q * 8, true}};
    int hist_stride = 1;
    qk_emit_call c;
    c.who = who;
    c.pipeline = "facet statistics";
    c.label = "k_scan (facet stats)";
    c.label_wide = "k_scan_wide (facet stats)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.Q = Q, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.radius = radius, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 8;
    c.check = [&]() -> int {
        if (n_cols < 1) QK_FAIL(QK_ERR_INVALID, "%s: n_cols=%d must be at least 1", who, n_cols);
        if (n_cols > QK_MAX_FACET_COLS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: n_cols=%d exceeds QK_MAX_FACET_COLS=%d", who, n_cols, QK_MAX_FACET_COLS);
        QK_TRY(facet_check_cols(c, facet_by, n_cols));
        // ---- the edges: host memory, checked here, uploaded once (facet_stats_device)
        if (edges && !n_edges) QK_FAIL(QK_ERR_INVALID, "%s: edges without n_edges", who);
        int max_e = 0;
        int64_t n_all = 0;
        if (n_edges)
            for (int i = 0; i < n_cols; i++) {
                const int E = n_edges[i];
                if (E < 0) QK_FAIL(QK_ERR_INVALID, "%s: n_edges[%d]=%d is negative", who, i, E);
                if (E > QK_MAX_FACET_EDGES)
                    QK_FAIL(QK_ERR_UNSUPPORTED, "%s: n_edges[%d]=%d exceeds QK_MAX_FACET_EDGES=%d", who, i, E, QK_MAX_FACET_EDGES);
                if (E > 0 && !edges) QK_FAIL(QK_ERR_INVALID, "%s: n_edges names edges, edges is null", who);
                for (int j = 1; j < E; j++)
                    if (edges[n_all + j - 1] >= edges[n_all + j])
                        QK_FAIL(QK_ERR_INVALID, "%s: the edges of column %d are not strictly ascending (edge %d)", who, i, j);
                n_all += E;
                max_e = std::max(max_e, E);
            }
        hist_stride = 1 + max_e;
        outs[6].bytes = bc * hist_stride;
        return QK_OK;
    };
    c.device = [&](qk_emit_env &e) -> int {
        int64_t *d[8];
        for (int i = 0; i < 8; i++) d[i] = (int64_t *)outs[i].dev;
        return facet_stats_device(c, e, edges, n_edges, hist_stride, FacetStatsOut{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]});
    };
    return qk_emit_run(c);
}

}  // namespace

extern "C" {

int qk_facet_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                    qk_filter *filter, qk_attr *const *facet_by, int n_cols, int n_values, int64_t *out_values, int64_t *out_counts,
                    int64_t *out_distinct, int64_t *out_missing, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_facet_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_facet_search: nprobe must be positive");
    return facet_call("qk_facet_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, metric, radius, filter, facet_by, n_cols, n_values,
                     out_values, out_counts, out_distinct, out_missing, out_total, mem, timing);
}

int qk_facet_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                  qk_filter *filter, qk_attr *const *facet_by, int n_cols, int n_values, int64_t *out_values, int64_t *out_counts,
                  int64_t *out_distinct, int64_t *out_missing, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_facet_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_facet_scan: bad partition id list");
    return facet_call("qk_facet_scan", ctx, nullptr, s, x, Q, pids, P, 0, metric, radius, filter, facet_by, n_cols, n_values, out_values,
                     out_counts, out_distinct, out_missing, out_total, mem, timing);
}

int qk_facet_stats_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                          qk_filter *filter, qk_attr *const *facet_by, int n_cols, const int64_t *edges, const int *n_edges,
                          int64_t *out_count, int64_t *out_missing, int64_t *out_min, int64_t *out_max, int64_t *out_sum_lo,
                          int64_t *out_sum_hi, int64_t *out_hist, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_facet_stats_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_facet_stats_search: nprobe must be positive");
    const FacetStatsOut out{out_count, out_missing, out_min, out_max, out_sum_lo, out_sum_hi, out_hist, out_total};
    return facet_stats_call("qk_facet_stats_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, metric, radius, filter, facet_by, n_cols,
                            edges, n_edges, out, mem, timing);
}

int qk_facet_stats_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                        qk_filter *filter, qk_attr *const *facet_by, int n_cols, const int64_t *edges, const int *n_edges,
                        int64_t *out_count, int64_t *out_missing, int64_t *out_min, int64_t *out_max, int64_t *out_sum_lo,
                        int64_t *out_sum_hi, int64_t *out_hist, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_facet_stats_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_facet_stats_scan: bad partition id list");
    const FacetStatsOut out{out_count, out_missing, out_min, out_max, out_sum_lo, out_sum_hi, out_hist, out_total};
    return facet_stats_call("qk_facet_stats_scan", ctx, nullptr, s, x, Q, pids, P, 0, metric, radius, filter, facet_by, n_cols, edges,
                            n_edges, out, mem, timing);
}

}  // extern "C"
