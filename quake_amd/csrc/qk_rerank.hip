// qk_rerank.hip -- multi-vector rerank (include/quake_hip.h, "multi-vector rerank"): the exact stage behind
// multi-vector search (qk_maxsim.hip).  For a shortlist of candidate values per logical query every participating token is compared
// with EVERY live row of the document, not with range hits of probed lists.  No parent, no nprobe, no key emission:
//   k_rerank_insert   the distinct candidate values of a group of logical queries claim slots of one open-addressing table
//                     (atomicCAS, bounded probing); a document IS its slot.  The value -1 looks like a free slot and owns the slot
//                     behind the table
//   k_rerank_count    one sweep over the row values of every live arena row, list by list (filter mask first, then the has-value
//                     mask): a row whose value sits in the table counts for its slot
//   k_rerank_offsets  exclusive scan of the counts (one workgroup), the total for the host, the counts cleared
//   k_rerank_fill     the same sweep writes the arena row into its document's segment (arrival order: a minimum over exact keys, a
//                     count and `matched` cannot see it)
//   k_rerank_score    the hot kernel, below
//   k_rerank_select   per logical query the <= 1024 records sorted in LDS under k_maxsim_select's order (mkey_less), a value named
//                     twice kept once, outputs and padding
// No kernel waits or spins; the host waits once per group, for the 8 bytes that size the row buffer.
#include "qk_maxsim.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int RR_FN_U = 4;              // blocks per load group (k_funnel_finish's double buffer)
constexpr int RR_SPLIT_ROWS = 512;      // a longer document is walked by all four waves of the workgroup
constexpr size_t RR_QUERY_LDS = 64 << 10;  // the staged tokens of a logical query; wider rows are walked in chunks of blocks
constexpr int64_t RR_GROUP_CANDS = (int64_t)1 << 22;  // candidates per table
constexpr int RR_TARGET_WGS = 2048;     // workgroups a launch of k_rerank_score aims at (256 CUs, several resident each)

// n_cand[l] of the call clamped to [0, C]; nullptr: C
__device__ __forceinline__ int rerank_ncand(const int32_t *n_cand, int64_t l, int C) { return n_cand ? min(max(n_cand[l], 0), C) : C; }

// the slot of value v, or -1: tvals has tmask + 1 slots and the slot of -1 behind them
__device__ __forceinline__ int64_t rerank_find(const unsigned long long *tvals, uint32_t tmask, unsigned long long v) {
    if (v == MS_EMPTY) return tvals[(int64_t)tmask + 1] != MS_EMPTY ? (int64_t)tmask + 1 : -1;
    uint32_t h = facet_hash(v) & tmask;
    for (uint32_t n = 0; n <= tmask; n++) {  // (the table holds twice its values: a free slot ends every chain)
        const unsigned long long cur = tvals[h];
        if (cur == v) return h;
        if (cur == MS_EMPTY) return -1;
        h = (h + 1) & tmask;
    }
    return -1;
}

// candidates l0 .. l0 + nl of the call, C each: tvals all ones before
__global__ __launch_bounds__(256) void k_rerank_insert(const int64_t *cand, const int32_t *n_cand, int64_t l0, int64_t nl, int C,
                                                       unsigned long long *tvals, uint32_t tmask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nl * C) return;
    const int64_t l = l0 + i / C;
    if ((int)(i % C) >= rerank_ncand(n_cand, l, C)) return;
    const unsigned long long v = (unsigned long long)cand[l0 * C + i];
    if (v == MS_EMPTY) {
        tvals[(int64_t)tmask + 1] = 0ull;  // (named: any word but all ones)
        return;
    }
    uint32_t h = facet_hash(v) & tmask;
    for (uint32_t n = 0; n <= tmask; n++) {
        unsigned long long cur = __hip_atomic_load(&tvals[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MS_EMPTY) {
            cur = atomicCAS(&tvals[h], MS_EMPTY, v);
            if (cur == MS_EMPTY) cur = v;
        }
        if (cur == v) return;
        h = (h + 1) & tmask;
    }
}

struct RerankSweep {
    const int64_t *pt_off;
    const int32_t *pt_size;
    const uint16_t *mask;  // row mask of a filter, or nullptr
    const uint16_t *has;   // has-value mask of the column
    const int64_t *rowval; // its value per arena row
    const unsigned long long *tvals;
    uint32_t tmask;
    uint32_t *cnt;         // [tmask + 2] rows per slot (count), the fill cursor (fill)
    const int64_t *off;    // [tmask + 2] first entry of every slot's segment
    int64_t *rows;         // the segments
};

// blockIdx.x = list number, blockIdx.y = slice (k_diverse_rows' decomposition): four rows in flight per lane
template <bool FILL>
__device__ __forceinline__ void rerank_sweep(const RerankSweep &W) {
    const int size = W.pt_size[blockIdx.x];  // (-1: no such list)
    if (size <= 0) return;
    const int64_t off = W.pt_off[blockIdx.x];
    for (int64_t r0 = (int64_t)blockIdx.y * 1024 + threadIdx.x; r0 < size; r0 += (int64_t)gridDim.y * 1024) {
        unsigned long long v[4];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t row = off + r0 + 256 * u;
            live[u] = r0 + 256 * u < size;
            if (live[u] && W.mask) live[u] = (W.mask[row >> 4] >> (row & 15)) & 1;
            if (live[u]) live[u] = (W.has[row >> 4] >> (row & 15)) & 1;
            v[u] = live[u] ? (unsigned long long)W.rowval[row] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!live[u]) continue;
            const int64_t sl = rerank_find(W.tvals, W.tmask, v[u]);
            if (sl < 0) continue;
            const uint32_t at = atomicAdd(&W.cnt[sl], 1u);
            if (FILL) W.rows[W.off[sl] + at] = off + r0 + 256 * u;
        }
    }
}
__global__ __launch_bounds__(256) void k_rerank_count(RerankSweep W) { rerank_sweep<false>(W); }
__global__ __launch_bounds__(256) void k_rerank_fill(RerankSweep W) { rerank_sweep<true>(W); }

// one workgroup: off[i] = sum of cnt[0 .. i), cnt cleared (it becomes the fill cursor and ends as the count again), *total = the sum
__global__ __launch_bounds__(1024) void k_rerank_offsets(uint32_t *cnt, int64_t *off, int64_t n, int64_t *total) {
    __shared__ uint32_t s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;  // (uniform)
    for (int64_t b0 = 0; b0 < n; b0 += 1024) {
        const int64_t i = b0 + tid;
        const uint32_t c = i < n ? cnt[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t base = 0, tot = 0;
        for (int w = 0; w < 16; w++) {
            base += w < wave ? s_wave[w] : 0u;
            tot += s_wave[w];
        }
        if (i < n) {
            off[i] = carry + base + incl - c;
            cnt[i] = 0u;
        }
        carry += tot;
        __syncthreads();  // (s_wave is rewritten by the next chunk)
    }
    if (tid == 0) *total = carry;
}

struct RerankParams {
    const float4 *xq4;         // [L * T][nblk][4] the prepared sub-queries (k_prep_queries)
    const float *xn;           // [L * T]
    const int32_t *n_tokens;   // [L] (device) or nullptr
    const int64_t *cand;       // [L][C]
    const int32_t *n_cand;     // [L] (device) or nullptr
    const unsigned long long *tvals;
    const uint32_t *cnt;       // rows of every slot's document
    const int64_t *off;        // its segment of rows
    const int64_t *rows;
    uint32_t tmask;
    const float4 *vecs;        // arena
    const float *norms;
    int nblk, cb;              // blocks of a row; blocks of the tokens staged at once (nblk unless CHUNK)
    int T, C, S, per;          // S slices of `per` candidates per logical query
    int metric, sqrt_l2;
    float missing;
    int64_t l0;                // the group's logical queries are l0 .. of the call's; blockIdx.x = (l - l0) * S + slice
    uint32_t *rhi;             // [group][C] score word of candidate c (all ones: no record)
    unsigned long long *rlo;   // [group][C] value ^ sign bit
    uint32_t *rm;              // [group][C] matched (0: no record)
    int32_t *rrows;            // [group][C] |D(g)|
};

// blocks b0 .. b0 + nb of the logical query's tokens into LDS in B-operand lane order: qs[(c * 4 + g) * TP + t] = piece g of block
// b0 + c of token t (zeros behind T), so lane (g, r) of column tile ct reads qs[(c * 4 + g) * TP + 16 ct + r]
template <int NT>
__device__ __forceinline__ void rerank_stage(const RerankParams &R, float4 *qs, int64_t lT, int b0, int nb, int tid) {
    constexpr int TP = NT * 16;
    // (threads run along t: 16 consecutive float4 of LDS per write, no bank conflict; the 16-byte reads, a token's row apart, hit L2)
    for (int e = tid; e < TP * nb * 4; e += 256) {
        const int cg = e / TP, t = e - cg * TP;
        qs[e] = t < R.T ? R.xq4[((lT + t) * R.nblk + b0) * 4 + cg] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// A wave walks tiles tile0, tile0 + tstep, .. of a document's rows dr[0 .. n): lane (g, r) gathers row r of the tile as the A operand
// of v_mfma_f32_16x16x4_f32 (k_funnel_finish's gather: the float4 at (tile_r nblk + c) 64 + 16 g + pos_r is in lane order already),
// column tile ct takes the tokens 16 ct .. 16 ct + 15 from LDS, x, y, z, w of every block in ascending c: the canonical chain.
// acc[ct][reg] of lane (g, j) = row 4 g + reg against token 16 ct + j; its ordered key lowers mk[ct], which stays in registers over
// the whole walk.  Rows behind the document's end gather the document's first row and get the largest key; so does a NaN pair.
// CHUNK: the tokens do not fit LDS; every tile step walks d in chunks of R.cb blocks re-staged by the whole workgroup with the
// accumulators live -- the chain simply continues -- so all four waves take every step (a wave without a tile only stages).
template <int NT, bool CHUNK>
__device__ __forceinline__ void rerank_walk(const RerankParams &R, float4 *qs, int64_t lT, const int64_t *dr, int n, int tile0, int tstep,
                                            const float (&xnq)[NT], uint32_t (&mk)[NT], int tid) {
    constexpr int TP = NT * 16;
    const int lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int nblk = R.nblk, ntiles = (n + 15) >> 4;
    const bool l2 = R.metric == QK_METRIC_L2;
    for (int tb = 0; tb < ntiles; tb += tstep) {
        const int tile = tb + tile0;
        const bool act = tile < ntiles;  // (wave-uniform)
        if (!CHUNK && !act) break;
        const int idx = tile * 16 + r;
        const int64_t row = act && idx < n ? dr[idx] : -1;
        const int64_t rs = row >= 0 ? row : dr[0];
        const float4 *base = R.vecs + ((rs >> 4) * nblk) * 64 + 16 * g + (rs & 15);
        const float nrm_r = R.norms[rs];
        f32x4 acc[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int b0 = 0; b0 < nblk; b0 += R.cb) {  // (one round unless CHUNK)
            const int bend = min(nblk, b0 + R.cb);
            if (CHUNK) {
                __syncthreads();  // (the readers of the previous chunk are done)
                rerank_stage<NT>(R, qs, lT, b0, bend - b0, tid);
                __syncthreads();
                if (!act) continue;
            }
            float4 a0[RR_FN_U], a1[RR_FN_U];
#define RR_LOAD(A, C0) \
    _Pragma("unroll") for (int u_ = 0; u_ < RR_FN_U; u_++) A[u_] = base[(int64_t)min((C0) + u_, bend - 1) * 64];
#define RR_STEP(A, C0)                                                                               \
    _Pragma("unroll") for (int u_ = 0; u_ < RR_FN_U; u_++) if ((C0) + u_ < bend) {                   \
        const float4 *bq_ = qs + (((C0) + u_ - b0) * 4 + g) * TP + r;                                \
        _Pragma("unroll") for (int ct = 0; ct < NT; ct++) {                                          \
            const float4 b_ = bq_[ct * 16];                                                          \
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].x, b_.x, acc[ct], 0, 0, 0);         \
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].y, b_.y, acc[ct], 0, 0, 0);         \
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].z, b_.z, acc[ct], 0, 0, 0);         \
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].w, b_.w, acc[ct], 0, 0, 0);         \
        }                                                                                            \
    }
            RR_LOAD(a0, b0)
            for (int c0 = b0; c0 < bend; c0 += 2 * RR_FN_U) {
                RR_LOAD(a1, c0 + RR_FN_U)
                RR_STEP(a0, c0)
                RR_LOAD(a0, c0 + 2 * RR_FN_U)
                RR_STEP(a1, c0 + RR_FN_U)
            }
#undef RR_LOAD
#undef RR_STEP
        }
        if (!act) continue;
        const int ok_r = row >= 0 ? 1 : 0;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int src = 4 * g + reg;  // the lane of group 0 that loaded row 4 g + reg
            const float nrm = __shfl(nrm_r, src, 64);
            const bool ok = __shfl(ok_r, src, 64) != 0;
#pragma unroll
            for (int ct = 0; ct < NT; ct++) {
                const float v = acc[ct][reg];
                const uint32_t o = l2 ? ord_from_l2(l2_expanded(xnq[ct], nrm, v)) : ord_from_ip(v);
                mk[ct] = min(mk[ct], ok ? o : 0xFFFFFFFFu);
            }
        }
    }
}

// the four row groups of a wave joined: every lane (g, j) ends with the minimum of token 16 ct + j
template <int NT>
__device__ __forceinline__ void rerank_join(uint32_t (&mk)[NT]) {
#pragma unroll
    for (int ct = 0; ct < NT; ct++) {
        mk[ct] = min(mk[ct], (uint32_t)__shfl_xor((int)mk[ct], 16, 64));
        mk[ct] = min(mk[ct], (uint32_t)__shfl_xor((int)mk[ct], 32, 64));
    }
}

// the end of a document, by one wave whose lanes (g, j) hold best(l, 16 ct + j, g) in mk[ct]: the terms in parallel, the float32
// sum one rounded addition after the other in token order, the record of candidate slot `at`
template <int NT>
__device__ __forceinline__ void rerank_finish(const RerankParams &R, int64_t at, unsigned long long v, int n, int nt, const uint32_t (&mk)[NT],
                                              int lane) {
    const int r = lane & 15;
    float term[NT];
    uint32_t matched = 0;
#pragma unroll
    for (int ct = 0; ct < NT; ct++) {
        const uint32_t o = mk[ct];
        const bool has = 16 * ct + r < nt && o != 0xFFFFFFFFu;
        matched += (uint32_t)__popcll(__ballot(has && lane < 16));
        float t = R.missing;
        if (has) {
            if (R.metric == QK_METRIC_L2) {
                const float d2 = __uint_as_float(o);
                t = R.sqrt_l2 ? sqrtf(d2) : d2;
            } else {
                t = ip_from_ord(o);
            }
        }
        term[ct] = t;
    }
    float s = 0.0f;
#pragma unroll
    for (int ct = 0; ct < NT; ct++)
        for (int j = 0; j < 16; j++) {
            const float t = __shfl(term[ct], j, 64);
            if (16 * ct + j < nt) s = s + t;
        }
    if (lane == 0) {
        R.rhi[at] = matched ? maxsim_score_word(s, R.metric) : 0xFFFFFFFFu;
        R.rlo[at] = v ^ MS_SIGN;
        R.rm[at] = matched;
        R.rrows[at] = n;
    }
}

// Work item = (logical query, slice of its candidates); four waves.  The logical query's tokens are staged once (dynamic LDS:
// [cb * 4][NT * 16] float4).  Then a wave takes a document of the slice at a time and walks its rows 16 at a time; a document
// longer than RR_SPLIT_ROWS -- and, under CHUNK, every document -- is walked by all four waves, tile w, w + 4, .. each, and joined by
// atomicMin on 64 key words in LDS, which is exact and independent of order.  NT = column tiles = ceil(T / 16).
template <int NT, bool CHUNK>
__global__ __launch_bounds__(256) void k_rerank_score(RerankParams R) {
    extern __shared__ float4 rr_lds4[];
    __shared__ uint32_t s_min[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15;
    const int64_t ll = blockIdx.x / R.S, l = R.l0 + ll, lT = l * R.T;
    const int slice = (int)(blockIdx.x - ll * R.S);
    const int nt = R.n_tokens ? min(max(R.n_tokens[l], 0), R.T) : R.T;
    const int c0 = slice * R.per, c1 = min(rerank_ncand(R.n_cand, l, R.C), c0 + R.per);
    if (c0 >= c1) return;
    if (nt == 0) {  // no token takes part: no candidate has a record
        for (int c = c0 + tid; c < c1; c += 256) {
            R.rhi[ll * R.C + c] = 0xFFFFFFFFu;
            R.rm[ll * R.C + c] = 0u;
            R.rrows[ll * R.C + c] = 0;
        }
        return;
    }
    float xnq[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ct++) xnq[ct] = (R.metric == QK_METRIC_L2 && 16 * ct + r < R.T) ? R.xn[lT + 16 * ct + r] : 0.f;
    if (!CHUNK) {
        rerank_stage<NT>(R, rr_lds4, lT, 0, R.nblk, tid);
        __syncthreads();
        // ---- a wave per document
        for (int c = c0 + wave; c < c1; c += 4) {
            const unsigned long long v = (unsigned long long)R.cand[l * R.C + c];
            const int64_t sl = rerank_find(R.tvals, R.tmask, v);
            const int n = sl >= 0 ? (int)R.cnt[sl] : 0;
            if (n > RR_SPLIT_ROWS) continue;
            uint32_t mk[NT];
#pragma unroll
            for (int ct = 0; ct < NT; ct++) mk[ct] = 0xFFFFFFFFu;
            if (n > 0) {
                rerank_walk<NT, false>(R, rr_lds4, lT, R.rows + R.off[sl], n, 0, 1, xnq, mk, tid);
                rerank_join<NT>(mk);
            }
            rerank_finish<NT>(R, ll * R.C + c, v, n, nt, mk, lane);
        }
    }
    // ---- the workgroup per document
    for (int c = c0; c < c1; c++) {
        const unsigned long long v = (unsigned long long)R.cand[l * R.C + c];
        const int64_t sl = rerank_find(R.tvals, R.tmask, v);
        const int n = sl >= 0 ? (int)R.cnt[sl] : 0;  // (uniform)
        if (!CHUNK && n <= RR_SPLIT_ROWS) continue;
        if (tid < 64) s_min[tid] = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t mk[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) mk[ct] = 0xFFFFFFFFu;
        if (n > 0) {
            rerank_walk<NT, CHUNK>(R, rr_lds4, lT, R.rows + R.off[sl], n, wave, 4, xnq, mk, tid);
            rerank_join<NT>(mk);
            if (lane < 16) {
#pragma unroll
                for (int ct = 0; ct < NT; ct++) atomicMin(&s_min[16 * ct + r], mk[ct]);
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int ct = 0; ct < NT; ct++) mk[ct] = s_min[16 * ct + r];
            rerank_finish<NT>(R, ll * R.C + c, v, n, nt, mk, lane);
        }
        __syncthreads();  // (s_min is cleared for the next document)
    }
}

struct RerankSelectParams {
    const int32_t *n_cand;  // [L] (device) or nullptr
    const uint32_t *rhi;
    const unsigned long long *rlo;
    const uint32_t *rm;
    const int32_t *rrows;
    int64_t l0;
    int C, k, metric;
    int64_t *out_groups;    // [L][k]
    float *out_scores;      // [L][k] or nullptr
    int32_t *out_matched;   // [L][k] or nullptr
    int32_t *out_rows;      // [L][k] or nullptr
    int64_t *out_n_groups;  // [L] or nullptr
    unsigned long long *gathered;  // [1] rows the score kernel gathered, summed over every (logical query, named candidate)
};

// blockIdx.x = logical query of the group: its records sorted under (score word, value ^ sign bit) -- k_maxsim_select's order --, the
// copies of a value named twice (equal records, so neighbours) dropped, the first k written, padding behind them
__global__ __launch_bounds__(256) void k_rerank_select(RerankSelectParams S) {
    __shared__ uint32_t s_hi[MS_SEL];
    __shared__ unsigned long long s_lo[MS_SEL];
    __shared__ uint32_t s_m[MS_SEL];
    __shared__ int32_t s_rows[MS_SEL];
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ll = blockIdx.x, ol = S.l0 + ll;
    const int nc = rerank_ncand(S.n_cand, ol, S.C);
    int n2 = 2;
    while (n2 < nc) n2 <<= 1;  // (<= MS_SEL)
    unsigned long long walked = 0;
    for (int i = tid; i < nc; i += 256) walked += (unsigned long long)S.rrows[ll * S.C + i];
    if (walked) atomicAdd(S.gathered, walked);
    for (int i = tid; i < n2; i += 256) {
        const bool rec = i < nc && S.rm[ll * S.C + i] != 0u;
        s_hi[i] = rec ? S.rhi[ll * S.C + i] : 0xFFFFFFFFu;
        s_lo[i] = rec ? S.rlo[ll * S.C + i] : ~0ull;
        s_m[i] = rec ? S.rm[ll * S.C + i] : 0xFFFFFFFFu;
        s_rows[i] = rec ? S.rrows[ll * S.C + i] : 0;
    }
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
                const MKey a{s_hi[i], s_lo[i], s_m[i]}, b{s_hi[o], s_lo[o], s_m[o]};
                const bool up = (i & kk) == 0;
                if (up ? mkey_less(b, a) : mkey_less(a, b)) {
                    const int32_t ra = s_rows[i], rb = s_rows[o];
                    s_hi[i] = b.hi, s_lo[i] = b.lo, s_m[i] = b.m, s_rows[i] = rb;
                    s_hi[o] = a.hi, s_lo[o] = a.lo, s_m[o] = a.m, s_rows[o] = ra;
                }
            }
            __syncthreads();
        }
    // entries 4 tid .. 4 tid + 3: a record that differs from the entry in front of it is a candidate of its own
    bool keep[4];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = 4 * tid + j;
        keep[j] = i < n2 && s_m[i] != 0xFFFFFFFFu && (i == 0 || s_hi[i] != s_hi[i - 1] || s_lo[i] != s_lo[i - 1]);
        mine += keep[j] ? 1u : 0u;
    }
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t at = incl - mine;
    for (int w = 0; w < wave; w++) at += s_wave[w];
    const uint32_t D = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (keep[j]) {
            const int i = 4 * tid + j;
            if (at < (uint32_t)S.k) {
                S.out_groups[ol * S.k + at] = (int64_t)(s_lo[i] ^ MS_SIGN);
                if (S.out_scores) S.out_scores[ol * S.k + at] = maxsim_score_of(s_hi[i], S.metric);
                if (S.out_matched) S.out_matched[ol * S.k + at] = (int32_t)s_m[i];
                if (S.out_rows) S.out_rows[ol * S.k + at] = s_rows[i];
            }
            at++;
        }
    for (int64_t j = (int64_t)min(D, (uint32_t)S.k) + tid; j < S.k; j += 256) {
        S.out_groups[ol * S.k + j] = 0;
        if (S.out_scores) S.out_scores[ol * S.k + j] = S.metric == QK_METRIC_L2 ? INFINITY : -INFINITY;
        if (S.out_matched) S.out_matched[ol * S.k + j] = 0;
        if (S.out_rows) S.out_rows[ol * S.k + j] = 0;
    }
    if (tid == 0 && S.out_n_groups) S.out_n_groups[ol] = D;
}

template <int NT>
int launch_rerank_score(hipStream_t st, const RerankParams &R, unsigned grid, size_t lds, bool chunk) {
    if (chunk) {
        QK_HIP(hipFuncSetAttribute((const void *)k_rerank_score<NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_rerank_score<NT, true>), dim3(grid), dim3(256), lds, st, R);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_rerank_score<NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_rerank_score<NT, false>), dim3(grid), dim3(256), lds, st, R);
    }
    return QK_OK;
}

// a buffer of the context grown to `need` bytes; QK_ERR_OOM leaves it as it was
int rerank_reserve(qk_ctx *ctx, char **buf, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return QK_OK;
    char *nb = nullptr;
    const size_t ncap = need + need / 4;
    if (hipMalloc((void **)&nb, ncap) != hipSuccess) {
        (void)hipGetLastError();
        QK_FAIL(QK_ERR_OOM, "multi-vector rerank: no device memory for %zu bytes of %s", ncap, what);
    }
    // (an earlier call's kernels may still read the old buffer: hipFree waits for the device)
    if (*buf) (void)hipFree(*buf);
    *buf = nb;
    *cap = ncap;
    ctx->scratch_reallocs++;
    return QK_OK;
}

}  // namespace

extern "C" {

int qk_maxsim_rerank(qk_ctx *ctx, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens, int metric, qk_filter *filter,
                     qk_attr *group_by, float missing, const int64_t *cand, const int32_t *n_cand, int C, int k, int64_t *out_groups,
                     float *out_scores, int32_t *out_matched, int32_t *out_rows, int64_t *out_n_groups, int mem, qk_timing *timing) {
    const char *who = "qk_maxsim_rerank";
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (T < 1) QK_FAIL(QK_ERR_INVALID, "%s: T=%d must be at least 1", who, T);
    if (T > QK_MAXSIM_MAX_TOKENS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: T=%d exceeds QK_MAXSIM_MAX_TOKENS=%d", who, T, QK_MAXSIM_MAX_TOKENS);
    if (C < 0) QK_FAIL(QK_ERR_INVALID, "%s: C=%d must not be negative", who, C);
    if (C > QK_MAXSIM_RERANK_MAX_CAND)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: C=%d exceeds QK_MAXSIM_RERANK_MAX_CAND=%d", who, C, QK_MAXSIM_RERANK_MAX_CAND);
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (missing != missing) QK_FAIL(QK_ERR_INVALID, "%s: missing is NaN", who);
    if (!group_by) QK_FAIL(QK_ERR_INVALID, "%s: group_by is null", who);
    qk_attr_data *col = group_by->d.get();
    if (col->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "%s: the group column belongs to another store", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (s->d > QK_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_MAX_D=%d", who, s->d, QK_MAX_D);
    if (L < 0 || (L > 0 && (!x || !out_groups || (C > 0 && !cand)))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (L > (int64_t)0x7FFFFFF0 / T || L > (int64_t)0x7FFFFFF0 / k) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: L * T or L * k too large", who);
    const bool host = mem == QK_MEM_HOST;
    if (host)
        for (int64_t l = 0; l < L; l++) {
            if (n_tokens && (n_tokens[l] < 0 || n_tokens[l] > T))
                QK_FAIL(QK_ERR_INVALID, "%s: n_tokens[%lld]=%d lies outside [0, T=%d]", who, (long long)l, n_tokens[l], T);
            if (n_cand && (n_cand[l] < 0 || n_cand[l] > C))
                QK_FAIL(QK_ERR_INVALID, "%s: n_cand[%lld]=%d lies outside [0, C=%d]", who, (long long)l, n_cand[l], C);
        }
    QK_TRY(qk_check_overflow(ctx));
    QK_HIP(hipSetDevice(ctx->device));
    if (timing) memset(timing, 0, sizeof(*timing));
    if (L == 0) return QK_OK;
    hipStream_t st = ctx->stream;
    const int nblk = s->nblk, NT = (T + 15) / 16, TP = NT * 16;
    // ---- what can fail for want of memory comes first: the call's buffer
    //      [table values] [counts] [offsets] [total] [score words] [values] [matched] [rows] and, for a host caller, [cand] [n_cand] [n_tokens]
    const int64_t Cs = std::max(C, 1);
    const int64_t gq = std::max<int64_t>(1, std::min<int64_t>(L, RR_GROUP_CANDS / Cs));  // logical queries per table
    int64_t Tn = 64;
    while (Tn < 2 * gq * Cs) Tn <<= 1;
    const size_t b_tv = qk_al256((size_t)(Tn + 1) * 8), b_cnt = qk_al256((size_t)(Tn + 1) * 4), b_off = qk_al256((size_t)(Tn + 1) * 8);
    const size_t b_r4 = qk_al256((size_t)gq * Cs * 4), b_r8 = qk_al256((size_t)gq * Cs * 8);
    const size_t b_cd = host ? qk_al256((size_t)L * Cs * 8) : 0, b_l4 = host ? qk_al256((size_t)L * 4) : 0;
    QK_TRY(rerank_reserve(ctx, &ctx->rr_buf, &ctx->rr_cap, b_tv + b_cnt + b_off + 256 + 3 * b_r4 + b_r8 + b_cd + 2 * b_l4, "tables and records"));
    char *b = ctx->rr_buf;
    unsigned long long *tvals = (unsigned long long *)b;
    uint32_t *cnt = (uint32_t *)(b + b_tv);
    int64_t *off = (int64_t *)(b + b_tv + b_cnt);
    int64_t *total = (int64_t *)(b + b_tv + b_cnt + b_off);
    char *rb = b + b_tv + b_cnt + b_off + 256;
    uint32_t *rhi = (uint32_t *)rb, *rm = (uint32_t *)(rb + b_r4);
    int32_t *rrows = (int32_t *)(rb + 2 * b_r4);
    unsigned long long *rlo = (unsigned long long *)(rb + 3 * b_r4);
    char *hb = rb + 3 * b_r4 + b_r8;
    // ---- staging and query preparation (the front end of every emission call, without parent and lists), the caller's outputs
    const size_t lk = (size_t)L * k;
    const size_t o_g = qk_al256(lk * 8), o_4 = qk_al256(lk * 4), o_n = qk_al256((size_t)L * 8);
    qk_scan_args sa;
    char *stage = nullptr;
    bool have_coarse = false;
    QK_TRY(qk_emit_front_end(ctx, nullptr, s, x, L * T, nullptr, 0, 0, metric, mem, o_g + 3 * o_4 + o_n, timing != nullptr, &sa, &stage,
                             &have_coarse));
    RerankSelectParams S;
    S.out_groups = host ? (int64_t *)stage : out_groups;
    S.out_scores = !out_scores ? nullptr : host ? (float *)(stage + o_g) : out_scores;
    S.out_matched = !out_matched ? nullptr : host ? (int32_t *)(stage + o_g + o_4) : out_matched;
    S.out_rows = !out_rows ? nullptr : host ? (int32_t *)(stage + o_g + 2 * o_4) : out_rows;
    S.out_n_groups = !out_n_groups ? nullptr : host ? (int64_t *)(stage + o_g + 3 * o_4) : out_n_groups;
    const int64_t *d_cand = cand;
    const int32_t *d_ncand = n_cand, *d_ntok = n_tokens;
    if (host) {  // (pageable sources: copied out when the calls return)
        if (C > 0) QK_HIP(hipMemcpyAsync(hb, cand, (size_t)L * C * 8, hipMemcpyHostToDevice, st));
        d_cand = (const int64_t *)hb;
        if (n_cand) QK_HIP(hipMemcpyAsync(hb + b_cd, n_cand, (size_t)L * 4, hipMemcpyHostToDevice, st));
        if (n_cand) d_ncand = (const int32_t *)(hb + b_cd);
        if (n_tokens) QK_HIP(hipMemcpyAsync(hb + b_cd + b_l4, n_tokens, (size_t)L * 4, hipMemcpyHostToDevice, st));
        if (n_tokens) d_ntok = (const int32_t *)(hb + b_cd + b_l4);
    }
    // ---- mask and row values
    const uint16_t *mask = nullptr;
    if (filter) QK_TRY(qk_filter_ensure(ctx, s, filter, &mask));
    QK_TRY(qk_store_sync_table(s));
    QK_TRY(qk_rowvals_ensure(ctx, s, *col));
    qk_phase_events pe;
    pe.ctx = ctx;
    pe.tm = ctx->timing && timing;
    pe.dtm = false;
    pe.ev_base = 4;
    QK_TRY(pe.mark(0));
    QK_TRY(pe.mark(1));
    // ---- per group of logical queries: table, sweep, score, select
    RerankSweep W;
    W.pt_off = s->d_off;
    W.pt_size = s->d_size;
    W.mask = mask;
    W.has = col->rv_has;
    W.rowval = col->rv_vals;
    W.tvals = tvals;
    W.tmask = (uint32_t)(Tn - 1);
    W.cnt = cnt;
    W.off = off;
    RerankParams R;
    R.xq4 = sa.xq4;
    R.xn = sa.xn;
    R.n_tokens = d_ntok;
    R.cand = d_cand;
    R.n_cand = d_ncand;
    R.tvals = tvals;
    R.cnt = cnt;
    R.off = off;
    R.tmask = W.tmask;
    R.vecs = (const float4 *)s->vecs;
    R.norms = s->norms;
    R.nblk = nblk;
    const bool chunk = (size_t)TP * nblk * 64 > RR_QUERY_LDS;
    R.cb = chunk ? (int)(RR_QUERY_LDS / ((size_t)TP * 64)) : nblk;
    R.T = T;
    R.C = C;
    R.metric = metric;
    R.sqrt_l2 = ctx->squared_l2 ? 0 : 1;
    R.missing = missing;
    R.rhi = rhi;
    R.rlo = rlo;
    R.rm = rm;
    R.rrows = rrows;
    S.n_cand = d_ncand;
    S.rhi = rhi;
    S.rlo = rlo;
    S.rm = rm;
    S.rrows = rrows;
    S.C = C;
    S.k = k;
    S.metric = metric;
    const size_t lds = (size_t)TP * R.cb * 64;
    const int64_t nl = (int64_t)s->parts.size();
    const unsigned ny = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (s->max_size + 1023) / 1024));
    S.gathered = (unsigned long long *)(total + 1);
    QK_HIP(hipMemsetAsync(S.gathered, 0, 8, st));
    for (int64_t l0 = 0; l0 < L; l0 += gq) {
        const int64_t ng = std::min(gq, L - l0);
        int64_t h_total = 0;
        if (C > 0) {
            QK_HIP(hipMemsetAsync(tvals, 0xFF, b_tv, st));
            QK_HIP(hipMemsetAsync(cnt, 0, b_cnt, st));
            hipLaunchKernelGGL(k_rerank_insert, dim3((unsigned)((ng * C + 255) / 256)), dim3(256), 0, st, d_cand, d_ncand, l0, ng, C, tvals, W.tmask);
            if (nl > 0) hipLaunchKernelGGL(k_rerank_count, dim3((unsigned)nl, ny), dim3(256), 0, st, W);
            hipLaunchKernelGGL(k_rerank_offsets, dim3(1), dim3(1024), 0, st, cnt, off, Tn + 1, total);
            QK_HIP(hipGetLastError());
            // the one wait of a group: the rows of its documents size the row buffer
            QK_HIP(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st));
            QK_HIP(hipStreamSynchronize(st));
            QK_TRY(rerank_reserve(ctx, &ctx->rr_rows, &ctx->rr_rows_cap, (size_t)std::max<int64_t>(h_total, 1) * 8, "document rows"));
            W.rows = (int64_t *)ctx->rr_rows;
            if (nl > 0 && h_total > 0) hipLaunchKernelGGL(k_rerank_fill, dim3((unsigned)nl, ny), dim3(256), 0, st, W);
        }
        if (l0 + gq >= L) QK_TRY(pe.mark(2));
        if (C > 0) {
            R.rows = (const int64_t *)ctx->rr_rows;
            R.l0 = l0;
            // slices: enough workgroups to fill the machine when L is small, at least one candidate per wave
            R.S = (int)std::max<int64_t>(1, std::min<int64_t>((C + 3) / 4, (RR_TARGET_WGS + ng - 1) / ng));
            R.per = (C + R.S - 1) / R.S;
            R.S = (C + R.per - 1) / R.per;
            const unsigned grid = (unsigned)(ng * R.S);
            QK_TRY(NT == 1 ? launch_rerank_score<1>(st, R, grid, lds, chunk) : NT == 2 ? launch_rerank_score<2>(st, R, grid, lds, chunk)
                 : NT == 3 ? launch_rerank_score<3>(st, R, grid, lds, chunk) : launch_rerank_score<4>(st, R, grid, lds, chunk));
        }
        S.l0 = l0;
        hipLaunchKernelGGL(k_rerank_select, dim3((unsigned)ng), dim3(256), 0, st, S);
        QK_HIP(hipGetLastError());
    }
    QK_TRY(pe.mark(3));
    if (host) {
        QK_HIP(hipMemcpyAsync(out_groups, S.out_groups, lk * 8, hipMemcpyDeviceToHost, st));
        if (out_scores) QK_HIP(hipMemcpyAsync(out_scores, S.out_scores, lk * 4, hipMemcpyDeviceToHost, st));
        if (out_matched) QK_HIP(hipMemcpyAsync(out_matched, S.out_matched, lk * 4, hipMemcpyDeviceToHost, st));
        if (out_rows) QK_HIP(hipMemcpyAsync(out_rows, S.out_rows, lk * 4, hipMemcpyDeviceToHost, st));
        if (out_n_groups) QK_HIP(hipMemcpyAsync(out_n_groups, S.out_n_groups, (size_t)L * 8, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
    }
    if (timing) {
        QK_HIP(hipStreamSynchronize(st));
        timing->n_items = (L + gq - 1) / gq;  // groups of the call
        unsigned long long gathered = 0;  // (a named candidate without a token that takes part walks no row and counts none)
        QK_HIP(hipMemcpy(&gathered, S.gathered, 8, hipMemcpyDeviceToHost));
        timing->scan_bytes = (int64_t)gathered * nblk * 64;
        QK_TRY(qk_read_phase_ms(ctx, timing, false, 4));
    }
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

}  // extern "C"
