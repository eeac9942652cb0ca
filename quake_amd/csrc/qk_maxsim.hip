// qk_maxsim.hip -- multi-vector search: a logical query is T sub-queries (token vectors); a document is the rows whose ids share a
// value of an attribute column; score(doc) = sum over the sub-queries of the best hit of the sub-query inside the document, the
// late interaction of ColBERT / ColPali (include/quake_hip.h, "multi-vector search").
//
// The expensive half is the key-emission scan over all L * T sub-queries, run pass by pass by qk_emit_passes (qk_dense.hip) exactly
// as for range search and the facets; the hit test is facet_hit (qk_facet.h).  A pass holds whole logical queries (its size is a
// multiple of T).  One open-addressing table per LOGICAL query: a slot is a value word and T key words, word t = the smallest key
// sub-query t met among the rows of that value.  The tables live in a pool of slots that is reserved once (at most
// QK_GROUPED_PASS_BYTES) and laid out per pass by the HITS: behind k_maxsim_hits the host reads the hit counts back, gives every
// logical query the power of two >= max(16, 2 * min(its hits, ids that have a value)) of slots plus 2 (facet_used_mask, the
// function the kernels evaluate too) and sends the pass's logical queries through the pool in groups that fit it.  Per pass
// k_maxsim_hits, then per group k_maxsim_clear, k_maxsim_claim, k_maxsim_select:
//   k_maxsim_hits    the hits of every participating sub-query (ballot + popcount per wave, one atomic add per wave)
//   k_maxsim_clear   the used slots of every table: value word and key words all ones
//   k_maxsim_claim   one workgroup sweeps slices of one sub-query: a hit whose id has a value finds or claims the slot of the value
//                    in its logical query's table (atomicCAS on the value word, linear probing, at most as many probes as slots;
//                    the value -1 owns the slot behind the used ones) and lowers word t of the slot (atomicMin)
//   k_maxsim_select  one workgroup per logical query: per occupied slot the terms from the key words (the epilogue conversion of
//                    k_select_pairs_large), their float32 sum in token order (one rounded addition after the other) and the matched
//                    count; the records (score word, value ^ sign bit, matched) are compacted to the front; more than 1024 of them
//                    are cut to the k smallest under the 96-bit key, byte by byte (k_facet_select's selection); the survivors are
//                    sorted in LDS (bitonic) and written with the padding
// No thread waits for another, every loop is bounded, phases are separated by kernel boundaries, only commutative minima decide a
// key word and values are distinct, so order keys are: the result is a pure function of the store, the column, the filter and the
// call.  The host side is one description, maxsim_call, for qk_emit_run (qk_emit.hip) and maxsim_device in qk_emit_device's skeleton.
#include "qk_facet.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr unsigned long long MS_EMPTY = ~0ull;
constexpr unsigned long long MS_SIGN = 0x8000000000000000ull;
constexpr int MS_SEL = QK_MAXSIM_MAX_K;  // records the selection sorts in LDS

struct MaxsimParams {
    FacetParams F;             // keys, segments, mask, has[0] / rowval[0], nq, P, Sg, the key interval, tmask, max_ids; total = the
                               // hits of every sub-query of the pass [nq]
    const int32_t *n_tokens;   // [L] of the call (device) or nullptr: T for every logical query
    int64_t l0;                // the pass's logical queries are l0 .. l0 + nq / T of the call's
    int64_t g0, ng;            // the group's are g0 .. g0 + ng of the pass's
    int T;
    const int64_t *toff;       // [nq / T] first slot of every logical query's table in the pool (the tables of a group lie one behind
                               // the other, each as long as the query uses: facet_used_mask + 2 slots)
    unsigned long long *tvals; // [pool slots] value words; k_maxsim_select leaves value ^ sign bit of the records at a table's front
    uint32_t *tkeys;           // [pool slots][T]
    uint32_t *rhi, *rm;        // [pool slots] score word and matched count of the records
    uint32_t *err;             // [1] set when a probe ran through a whole table without finding or claiming its value
};

// sub-queries of logical query lq (of the pass) that take part: a device value is clamped to [0, T]
__device__ __forceinline__ int maxsim_ntok(const MaxsimParams &M, int64_t lq) {
    return M.n_tokens ? min(max(M.n_tokens[M.l0 + lq], 0), M.T) : M.T;
}
// hits of logical query lq over its nt participating sub-queries
__device__ __forceinline__ uint64_t maxsim_hits_of(const MaxsimParams &M, int64_t lq, int nt) {
    uint64_t n = 0;
    for (int t = 0; t < nt; t++) n += M.F.total[lq * M.T + t];
    return n;
}

// blockIdx.x = sub-query of the pass * Sg + g: k_facet_hits' decomposition; a sub-query that does not take part has no hits
__global__ __launch_bounds__(256) void k_maxsim_hits(MaxsimParams M) {
    const FacetParams &F = M.F;
    const int64_t q = blockIdx.x / F.Sg, lq = q / M.T;
    if ((int)(q - lq * M.T) >= maxsim_ntok(M, lq)) return;
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

// blockIdx.x = logical query of the group: the slots its table uses become empty
__global__ __launch_bounds__(256) void k_maxsim_clear(MaxsimParams M) {
    const int64_t lq = M.g0 + blockIdx.x;
    const int64_t tb = M.toff[lq];
    const int64_t used = (int64_t)facet_used_mask(maxsim_hits_of(M, lq, maxsim_ntok(M, lq)), M.F.max_ids, M.F.tmask) + 2;
    for (int64_t i = threadIdx.x; i < used; i += 256) M.tvals[tb + i] = MS_EMPTY;
    for (int64_t i = threadIdx.x; i < used * M.T; i += 256) M.tkeys[tb * M.T + i] = 0xFFFFFFFFu;
}

// blockIdx.x = (logical query of the group * T + t) * Sg + g; a sub-query without hits is left at once
__global__ __launch_bounds__(256) void k_maxsim_claim(MaxsimParams M) {
    const FacetParams &F = M.F;
    const int64_t sq = blockIdx.x / F.Sg, ll = sq / M.T, lq = M.g0 + ll;
    const int t = (int)(sq - ll * M.T);
    const int nt = maxsim_ntok(M, lq);
    const int64_t q = lq * M.T + t;
    if (t >= nt || F.total[q] == 0) return;
    const uint32_t umask = facet_used_mask(maxsim_hits_of(M, lq, nt), F.max_ids, F.tmask);
    const int64_t *pbase = F.pair_base + q * F.P;
    const int64_t *qpids = F.pids ? F.pids + q * F.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[F.P];
    const int64_t tb = M.toff[lq];
    unsigned long long *tv = M.tvals + tb;
    uint32_t *tk = M.tkeys + tb * M.T;
    for (int64_t s0 = beg + (int64_t)(blockIdx.x - sq * F.Sg) * FC_SLICE; s0 < end; s0 += (int64_t)F.Sg * FC_SLICE) {
        const int64_t lim = min(end, s0 + FC_SLICE);
        for (int64_t pos = s0 + threadIdx.x; pos < lim; pos += 256) {
            int64_t row;
            if (!facet_hit(F, pbase, qpids, pos, lim, &row)) continue;
            if (!((F.has[0][row >> 4] >> (row & 15)) & 1)) continue;
            const unsigned long long v = (unsigned long long)F.rowval[0][row];
            int64_t sl = -1;
            if (v == MS_EMPTY) {
                sl = (int64_t)umask + 1;  // the value that looks like an empty slot has a slot of its own
            } else {
                // linear probing; the table holds at least twice the values a logical query can meet, so an empty slot ends every
                // chain -- and at most as many probes as slots whatever happens: this loop cannot spin
                uint32_t h = facet_hash(v) & umask;
                for (uint32_t n = 0; n <= umask; n++) {
                    unsigned long long cur = __hip_atomic_load(&tv[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == MS_EMPTY) {
                        cur = atomicCAS(&tv[h], MS_EMPTY, v);
                        if (cur == MS_EMPTY) cur = v;
                    }
                    if (cur == v) {
                        sl = h;
                        break;
                    }
                    h = (h + 1) & umask;
                }
            }
            if (sl >= 0) atomicMin(&tk[sl * M.T + t], F.keys[pos]);
            else *M.err = 1u;  // (cannot happen while the table holds twice the values; the host reports it if it ever does)
        }
    }
}

// the score as an unsigned word that orders as asked (smaller = better): -0 counts as +0, a NaN is 0xFFFFFFFF, the word no number has
__device__ __forceinline__ uint32_t maxsim_score_word(float s, int metric) {
    if (s != s) return 0xFFFFFFFFu;
    uint32_t b = __float_as_uint(s);
    b = b == 0x80000000u ? 0u : b;
    const uint32_t asc = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return metric == QK_METRIC_IP ? ~asc : asc;
}
__device__ __forceinline__ float maxsim_score_of(uint32_t w, int metric) {
    if (w == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    const uint32_t asc = metric == QK_METRIC_IP ? ~w : w;
    return __uint_as_float((asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc);
}

struct MaxsimSelectParams {
    MaxsimParams M;
    int64_t L;                 // of the call
    int k, metric, sqrt_l2;
    float missing;
    int64_t *out_groups;       // [L][k]
    float *out_scores;         // [L][k] or nullptr
    int32_t *out_matched;      // [L][k] or nullptr
    int64_t *out_n_groups;     // [L] or nullptr
    int64_t *out_hits;         // [L][T] or nullptr
};

// a record of the selection: (score word, value ^ sign bit) is the 96-bit order key; m (the matched count, all ones for padding)
// only separates a record from padding that looks like it
struct MKey {
    uint32_t hi;
    unsigned long long lo;
    uint32_t m;
};
__device__ __forceinline__ bool mkey_less(const MKey &a, const MKey &b) {
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.m < b.m;
}
// byte d (0 = most significant, 11 = least) of an order key, and whether the bytes in front of d equal those of p (fkey_byte /
// fkey_prefix of qk_facet.hip)
__device__ __forceinline__ uint32_t mkey_byte(uint32_t hi, unsigned long long lo, int d) {
    return d < 4 ? (hi >> (24 - 8 * d)) & 255u : (uint32_t)(lo >> (56 - 8 * (d - 4))) & 255u;
}
__device__ __forceinline__ bool mkey_prefix(uint32_t hi, unsigned long long lo, uint32_t phi, unsigned long long plo, int d) {
    if (d == 0) return true;
    if (d <= 4) return d == 4 ? hi == phi : (hi >> (32 - 8 * d)) == (phi >> (32 - 8 * d));
    return hi == phi && (lo >> (64 - 8 * (d - 4))) == (plo >> (64 - 8 * (d - 4)));
}

// blockIdx.x = logical query of the group
__global__ __launch_bounds__(256) void k_maxsim_select(MaxsimSelectParams S) {
    __shared__ uint32_t s_hi[MS_SEL];
    __shared__ unsigned long long s_lo[MS_SEL];
    __shared__ uint32_t s_m[MS_SEL];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_pick[2];
    const MaxsimParams &M = S.M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lq = M.g0 + blockIdx.x, ol = M.l0 + lq;
    const int T = M.T, nt = maxsim_ntok(M, lq);
    const int64_t tb = M.toff[lq];
    unsigned long long *tv = M.tvals + tb;
    const uint32_t *tk = M.tkeys + tb * T;
    uint32_t *rhi = M.rhi + tb, *rm = M.rm + tb;
    const int64_t used = (int64_t)facet_used_mask(maxsim_hits_of(M, lq, nt), M.F.max_ids, M.F.tmask) + 2;
    // ---- 1. the record of every occupied slot (a claimed one, or the slot of -1 behind the used ones when a key reached it) to the
    //         front, in any order (k_facet_select's compaction).  The whole chunk of 1024 slots is in registers behind the first
    //         barrier before any of it is written, and the D records written so far satisfy D <= b0: every write of the chunk
    //         lands in [D, b0 + 1024), slots that were read in this chunk or an earlier one and are never read again by this step
    uint32_t D = 0;  // (uniform)
    for (int64_t b0 = 0; b0 < used; b0 += 1024) {
        unsigned long long v[4];
        uint32_t hi[4], mt[4];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = b0 + j * 256 + tid;
            v[j] = i < used ? tv[i] : MS_EMPTY;
            hi[j] = 0u;
            mt[j] = 0u;
            if (i < used && (v[j] != MS_EMPTY || i == used - 1)) {
                float s = 0.0f;
                for (int t = 0; t < nt; t++) {  // one rounded float32 addition per term, in token order
                    const uint32_t o = tk[i * T + t];
                    float term = S.missing;
                    if (o != 0xFFFFFFFFu) {
                        mt[j]++;
                        if (S.metric == QK_METRIC_L2) {
                            const float d2 = __uint_as_float(o);
                            term = S.sqrt_l2 ? sqrtf(d2) : d2;
                        } else {
                            term = ip_from_ord(o);
                        }
                    }
                    s = s + term;
                }
                hi[j] = maxsim_score_word(s, S.metric);
            }
            mine += mt[j] ? 1u : 0u;
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
            if (mt[j]) {
                tv[at] = v[j] ^ MS_SIGN;
                rhi[at] = hi[j];
                rm[at] = mt[j];
                at++;
            }
        D += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
    __syncthreads();  // (the records are visible to the workgroup)
    // ---- 2. more than MS_SEL records: the k-th smallest order key, byte by byte from the top; values are distinct, so keys are and
    //         exactly k records lie at or below it
    uint32_t thi = 0xFFFFFFFFu;
    unsigned long long tlo = ~0ull;
    if (D > MS_SEL) {
        uint32_t phi = 0u;
        unsigned long long plo = 0ull;
        uint32_t need = (uint32_t)S.k;
        for (int d = 0; d < 12; d++) {
            s_hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < D; i += 256) {
                const uint32_t h = rhi[i];
                const unsigned long long l = tv[i];
                if (mkey_prefix(h, l, phi, plo, d)) atomicAdd(&s_hist[mkey_byte(h, l, d)], 1u);
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
            if (d < 4) phi |= b << (24 - 8 * d);
            else plo |= (unsigned long long)b << (56 - 8 * (d - 4));
            __syncthreads();  // (s_pick and s_hist are rewritten by the next byte)
        }
        thi = phi;
        tlo = plo;
    }
    // ---- 3. the survivors into LDS (at most MS_SEL of them), padded behind every record, sorted ascending over the power of two
    //         that holds them
    const uint32_t nsurv = D > MS_SEL ? (uint32_t)S.k : D;  // (uniform)
    int n2 = 2;
    while ((uint32_t)n2 < nsurv) n2 <<= 1;  // (<= MS_SEL)
    if (tid == 0) s_n = 0;
    for (int i = tid; i < n2; i += 256) {
        s_hi[i] = 0xFFFFFFFFu;
        s_lo[i] = ~0ull;
        s_m[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (uint32_t i = tid; i < D; i += 256) {
        const uint32_t h = rhi[i];
        const unsigned long long l = tv[i];
        if (h < thi || (h == thi && l <= tlo)) {
            const uint32_t at = atomicAdd(&s_n, 1u);
            if (at < (uint32_t)n2) {
                s_hi[at] = h;
                s_lo[at] = l;
                s_m[at] = rm[i];
            }
        }
    }
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
                const MKey a{s_hi[i], s_lo[i], s_m[i]}, b{s_hi[o], s_lo[o], s_m[o]};
                const bool up = (i & kk) == 0;
                if (up ? mkey_less(b, a) : mkey_less(a, b)) {
                    s_hi[i] = b.hi;
                    s_lo[i] = b.lo;
                    s_m[i] = b.m;
                    s_hi[o] = a.hi;
                    s_lo[o] = a.lo;
                    s_m[o] = a.m;
                }
            }
            __syncthreads();
        }
    // ---- 4. the answer: entries behind the candidate values are padding
    const uint32_t nreal = min(nsurv, (uint32_t)S.k);
    for (int j = tid; j < S.k; j += 256) {
        const bool real = (uint32_t)j < nreal;
        S.out_groups[ol * S.k + j] = real ? (int64_t)(s_lo[j] ^ MS_SIGN) : 0;
        if (S.out_scores)
            S.out_scores[ol * S.k + j] = real ? maxsim_score_of(s_hi[j], S.metric) : (S.metric == QK_METRIC_L2 ? INFINITY : -INFINITY);
        if (S.out_matched) S.out_matched[ol * S.k + j] = real ? (int32_t)s_m[j] : 0;
    }
    if (tid == 0 && S.out_n_groups) S.out_n_groups[ol] = D;
    if (S.out_hits && tid < T) S.out_hits[ol * T + tid] = tid < nt ? (int64_t)M.F.total[lq * T + tid] : 0;
}

__global__ __launch_bounds__(256) void k_maxsim_fill(float *p, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

struct MaxsimOut {
    int64_t *groups;
    float *scores;
    int32_t *matched;
    int64_t *n_groups, *hits;
};

// bytes of a table slot: the value word, T key words, the score word and the matched count
inline int64_t qk_maxsim_slot_bytes(int T) { return 16 + 4 * (int64_t)T; }

// the device half; o: the call's outputs on the device (nullptr: not wanted); n_tokens: the caller's pointer in the call's `mem`
int maxsim_device(const qk_emit_call &c, qk_emit_env &e, int64_t L, int T, const int32_t *n_tokens, float missing, int k,
                  const MaxsimOut &o) {
    qk_store *s = c.s;
    const qk_scan_args &a = e.a;
    const int P = e.P;
    const bool host = c.mem == QK_MEM_HOST;
    hipStream_t st = c.ctx->stream;
    qk_emit_stages g;
    g.pad = [&]() -> int {  // no lists: no candidates
        QK_HIP(hipMemsetAsync(o.groups, 0, (size_t)L * k * 8, st));
        if (o.scores)
            hipLaunchKernelGGL(k_maxsim_fill, dim3((unsigned)((L * k + 255) / 256)), dim3(256), 0, st, o.scores, L * k,
                               a.metric == QK_METRIC_L2 ? INFINITY : -INFINITY);
        if (o.matched) QK_HIP(hipMemsetAsync(o.matched, 0, (size_t)L * k * 4, st));
        if (o.n_groups) QK_HIP(hipMemsetAsync(o.n_groups, 0, (size_t)L * 8, st));
        if (o.hits) QK_HIP(hipMemsetAsync(o.hits, 0, (size_t)L * T * 8, st));
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    const int64_t max_ids = c.cols[0]->n_ids;
    // this pipeline's bytes of the call's buffer, sized for the largest pass: the pool of table slots
    // [values] [keys] [score words] [matched counts], then [hits] [table offsets] [error word] [n_tokens of a host caller].
    // NS bounds the slots one logical query can ever use (the grouped rule over T * per_query_ub keys); the pool holds
    // min(that bound for every logical query of a pass, QK_GROUPED_PASS_BYTES) and is laid out per pass by the hits (consume)
    int64_t NS = 0, S = 0, pool = 0;
    size_t o_tkeys = 0, o_rhi = 0, o_rm = 0, o_hits = 0, o_toff = 0, o_err = 0, o_ntok = 0;
    std::vector<uint32_t> h_hits;  // the pass's hits and table offsets on the host (alive until the call returns)
    std::vector<int64_t> h_toff;
    uint32_t *err_dev = nullptr;   // the error word (the same address in every pass)
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        *qc = *qc / T * T;  // a logical query never straddles a pass
        if (*qc < T)
            QK_FAIL(QK_ERR_UNSUPPORTED, "multi-vector search: the %d sub-queries of a logical query with room for %lld keys each do not fit one pass",
                    T, (long long)per_query_ub);
        NS = qk_grouped_table_slots((int64_t)T * per_query_ub, max_ids);
        pool = std::min<int64_t>((*qc / T) * (NS + 1), QK_GROUPED_PASS_BYTES / qk_maxsim_slot_bytes(T));
        S = (per_query_ub + FC_SLICE - 1) / FC_SLICE;
        if (*qc * S > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "multi-vector search: L * T too large");
        o_tkeys = qk_al256((size_t)pool * 8);
        o_rhi = o_tkeys + qk_al256((size_t)pool * T * 4);
        o_rm = o_rhi + qk_al256((size_t)pool * 4);
        o_hits = o_rm + qk_al256((size_t)pool * 4);
        o_toff = o_hits + qk_al256((size_t)*qc * 4);
        o_err = o_toff + qk_al256((size_t)(*qc / T) * 8);
        o_ntok = o_err + 256;
        *extra_bytes = o_ntok + (host && n_tokens ? qk_al256((size_t)L * 4) : 0);
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        QK_HIP(hipMemsetAsync(p.extra + o_hits, 0, (size_t)p.nq * 4, st));
        if (p.q0 == 0) QK_HIP(hipMemsetAsync(p.extra + o_err, 0, 4, st));
        // a host caller's n_tokens, once per call: a stream-ordered copy from pageable memory, as the edges of facet statistics
        if (p.q0 == 0 && host && n_tokens) QK_HIP(hipMemcpyAsync(p.extra + o_ntok, n_tokens, (size_t)L * 4, hipMemcpyHostToDevice, st));
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        MaxsimSelectParams R;
        MaxsimParams &M = R.M;
        FacetParams &F = M.F;
        facet_params_fill(F, p, s, e.mask, c.cols, 1, e.key_lo, e.key_hi, P, S);
        F.total = (uint32_t *)(p.extra + o_hits);
        F.tmask = (uint32_t)(NS - 1);
        F.max_ids = max_ids;
        M.n_tokens = !n_tokens ? nullptr : host ? (const int32_t *)(p.extra + o_ntok) : n_tokens;
        M.l0 = p.q0 / T;
        M.T = T;
        M.tvals = (unsigned long long *)p.extra;
        M.tkeys = (uint32_t *)(p.extra + o_tkeys);
        M.rhi = (uint32_t *)(p.extra + o_rhi);
        M.rm = (uint32_t *)(p.extra + o_rm);
        M.toff = (const int64_t *)(p.extra + o_toff);
        M.err = err_dev = (uint32_t *)(p.extra + o_err);
        M.g0 = 0;
        M.ng = 0;
        hipLaunchKernelGGL(k_maxsim_hits, dim3((unsigned)(p.nq * F.Sg)), dim3(256), 0, st, M);
        R.L = L;
        R.k = k;
        R.metric = a.metric;
        R.sqrt_l2 = a.sqrt_l2 ? 1 : 0;
        R.missing = missing;
        R.out_groups = o.groups;
        R.out_scores = o.scores;
        R.out_matched = o.matched;
        R.out_n_groups = o.n_groups;
        R.out_hits = o.hits;
        // The tables are laid out by the hits, which only the device knows: the one place where the host waits inside a pass
        // (4 bytes per sub-query come back).  A logical query's table is as long as it uses -- facet_used_mask + 2 slots, the same
        // function the kernels evaluate -- and the pass's logical queries go through the pool in groups that fit it, one group
        // after the other.  (A sub-query that does not take part has no hits: the sum over all T is the sum the kernels take.)
        const int64_t nl = p.nq / T;
        h_hits.resize((size_t)p.nq);
        h_toff.resize((size_t)nl);
        QK_HIP(hipMemcpyAsync(h_hits.data(), F.total, (size_t)p.nq * 4, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
        std::vector<int64_t> first;  // first logical query of every group, then nl
        int64_t cur = 0;
        for (int64_t l = 0; l < nl; l++) {
            uint64_t hits = 0;
            for (int t = 0; t < T; t++) hits += h_hits[(size_t)(l * T + t)];
            const int64_t used = (int64_t)facet_used_mask(hits, max_ids, F.tmask) + 2;
            if (used > pool)
                QK_FAIL(QK_ERR_UNSUPPORTED, "multi-vector search: the table of a logical query with %llu hits needs %lld bytes, more than QK_GROUPED_PASS_BYTES",
                        (unsigned long long)hits, (long long)(used * qk_maxsim_slot_bytes(T)));
            if (l == 0 || cur + used > pool) {
                first.push_back(l);
                cur = 0;
            }
            h_toff[(size_t)l] = cur;
            cur += used;
        }
        first.push_back(nl);
        QK_HIP(hipMemcpyAsync(p.extra + o_toff, h_toff.data(), (size_t)nl * 8, hipMemcpyHostToDevice, st));
        for (size_t gi = 0; gi + 1 < first.size(); gi++) {
            M.g0 = first[gi];
            M.ng = first[gi + 1] - first[gi];
            F.Sg = qk_emit_sg(S, M.ng * T);
            hipLaunchKernelGGL(k_maxsim_clear, dim3((unsigned)M.ng), dim3(256), 0, st, M);
            hipLaunchKernelGGL(k_maxsim_claim, dim3((unsigned)(M.ng * T * F.Sg)), dim3(256), 0, st, M);
            hipLaunchKernelGGL(k_maxsim_select, dim3((unsigned)M.ng), dim3(256), 0, st, R);
        }
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    g.tail = [&]() -> int {  // the error word of k_maxsim_claim: never set while a table holds twice its values
        if (!err_dev) return QK_OK;
        uint32_t err = 0;
        QK_HIP(hipMemcpyAsync(&err, err_dev, 4, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
        if (err) QK_FAIL(QK_ERR_HIP, "multi-vector search: a table probe found no slot: the results of this call are incomplete");
        return QK_OK;
    };
    return qk_emit_device(c, e, g);
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int maxsim_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens,
                const int64_t *pids, int P, int nprobe, int metric, float radius, qk_filter *filter, qk_attr *group_by, float missing, int k,
                const MaxsimOut &out, int mem, qk_timing *timing) {
    // [groups] [scores] [matched] [n_groups] [hits]; the bytes are filled in once T and k are checked
    qk_emit_out outs[5] = {{out.groups, 0, true}, {out.scores, 0, false}, {out.matched, 0, false}, {out.n_groups, 0, false}, {out.hits, 0, false}};
    qk_emit_call c;
    c.who = who;
    c.pipeline = "multi-vector search";
    c.label = "k_scan (maxsim)";
    c.label_wide = "k_scan_wide (maxsim)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.radius = radius, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 5;
    // the driver's Q: the sub-queries (the driver reads it before `check` runs, which refuses every T and L this line leaves alone)
    c.Q = (L > 0 && T >= 1 && T <= QK_MAXSIM_MAX_TOKENS && L <= (int64_t)0x7FFFFFF0 / T) ? L * T : L;
    c.check = [&]() -> int {
        if (T < 1) QK_FAIL(QK_ERR_INVALID, "%s: T=%d must be at least 1", who, T);
        if (T > QK_MAXSIM_MAX_TOKENS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: T=%d exceeds QK_MAXSIM_MAX_TOKENS=%d", who, T, QK_MAXSIM_MAX_TOKENS);
        if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
        if (k > QK_MAXSIM_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAXSIM_MAX_K=%d", who, k, QK_MAXSIM_MAX_K);
        if (missing != missing) QK_FAIL(QK_ERR_INVALID, "%s: missing is NaN", who);
        if (!group_by) QK_FAIL(QK_ERR_INVALID, "%s: group_by is null", who);
        c.cols[0] = group_by->d.get();
        c.n_cols = 1;
        if (c.cols[0]->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "%s: the group column belongs to another store", who);
        if (L > (int64_t)0x7FFFFFF0 / T) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: L * T too large", who);
        if (n_tokens && mem == QK_MEM_HOST)
            for (int64_t l = 0; l < L; l++)
                if (n_tokens[l] < 0 || n_tokens[l] > T)
                    QK_FAIL(QK_ERR_INVALID, "%s: n_tokens[%lld]=%d lies outside [0, T=%d]", who, (long long)l, n_tokens[l], T);
        if (L > 0) {
            const size_t lk = (size_t)L * k;
            outs[0].bytes = lk * 8, outs[1].bytes = lk * 4, outs[2].bytes = lk * 4, outs[3].bytes = (size_t)L * 8, outs[4].bytes = (size_t)L * T * 8;
        }
        return QK_OK;
    };
    c.device = [&](qk_emit_env &e) -> int {
        const MaxsimOut dv{(int64_t *)outs[0].dev, (float *)outs[1].dev, (int32_t *)outs[2].dev, (int64_t *)outs[3].dev, (int64_t *)outs[4].dev};
        return maxsim_device(c, e, L, T, n_tokens, missing, k, dv);
    };
    return qk_emit_run(c);
}

}  // namespace

extern "C" {

int qk_maxsim_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens, int nprobe,
                     int metric, float radius, qk_filter *filter, qk_attr *group_by, float missing, int k, int64_t *out_groups,
                     float *out_scores, int32_t *out_matched, int64_t *out_n_groups, int64_t *out_hits, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_maxsim_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_maxsim_search: nprobe must be positive");
    const MaxsimOut out{out_groups, out_scores, out_matched, out_n_groups, out_hits};
    return maxsim_call("qk_maxsim_search", ctx, parent, s, x, L, T, n_tokens, nullptr, 0, nprobe, metric, radius, filter, group_by, missing, k,
                       out, mem, timing);
}

int qk_maxsim_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens, const int64_t *pids, int P,
                   int metric, float radius, qk_filter *filter, qk_attr *group_by, float missing, int k, int64_t *out_groups,
                   float *out_scores, int32_t *out_matched, int64_t *out_n_groups, int64_t *out_hits, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_maxsim_scan: null argument");
    if (P <= 0 || (L > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_maxsim_scan: bad partition id list");
    const MaxsimOut out{out_groups, out_scores, out_matched, out_n_groups, out_hits};
    return maxsim_call("qk_maxsim_scan", ctx, nullptr, s, x, L, T, n_tokens, pids, P, 0, metric, radius, filter, group_by, missing, k, out, mem,
                       timing);
}

}  // extern "C"
