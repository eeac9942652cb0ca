// qk_diverse.hip -- diversified search (include/quake_hip.h, "diversified search"): the fetch_k nearest rows of
// every query, re-ranked on the device by maximal marginal relevance.
// The candidate search is the shipped one (qk_run_search with k = fetch_k, filtered or not) and nothing here changes it.  Behind it,
// on the same stream and without a host wait:
//   k_diverse_insert   the distinct candidate ids of a group of queries claim slots of an open-addressing table (atomicCAS)
//   k_diverse_rows     one sweep over the stored ids of every live row of the arena; a row whose id is in the table writes its arena
//                      row there (atomicMin: an id stored twice takes its smallest row)
//   k_diverse_select   one workgroup per query, one lane per candidate: the greedy selection.  Every step needs the pairwise value
//                      of each unpicked candidate against the vector picked last -- the canonical k-ordered fmaf chain over the
//                      tile-major row, l2_expanded over the stored norms.  Two forms: STAGE_ALL copies the query's C rows into LDS
//                      once and reads both operands from there; the other stages the picked vector only and re-reads every
//                      candidate row from global memory at every step (the form for rows that do not fit, d up to QK_MAX_D).
#include "qk_internal.h"

#include "qk_device.h"

#include <cmath>
#include <cstring>

#ifndef QK_DIVERSE_STAGE_ALL
#define QK_DIVERSE_STAGE_ALL 1  // 0: always the re-read form (the A/B of scripts/diverse_probe.py)
#endif

namespace {

constexpr unsigned long long DV_EMPTY = ~0ull;          // a free slot / "no row": the id -1 is padding and never inserted
constexpr int64_t DV_GROUP_CANDS = (int64_t)1 << 22;    // candidates per table: at most 2^23 slots of 16 bytes
constexpr size_t DV_STAGE_ALL_LDS = (size_t)144 << 10;  // the rows of a query in LDS: up to 144 KiB of the CU's 160

__device__ __forceinline__ uint32_t dv_hash(unsigned long long v) {
    v ^= v >> 33;
    v *= 0xff51afd7ed558ccdULL;
    v ^= v >> 33;
    v *= 0xc4ceb9fe1a85ec53ULL;
    v ^= v >> 33;
    return (uint32_t)v;
}

// n candidate ids (padding -1 skipped) -> keys [tmask + 1], all DV_EMPTY before.  The table has at least 2 n slots: a probe
// sequence always meets a free one.
__global__ __launch_bounds__(256) void k_diverse_insert(const int64_t *cand, int64_t n, unsigned long long *keys, uint32_t tmask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long id = (unsigned long long)cand[i];
    if (id == DV_EMPTY) return;
    uint32_t h = dv_hash(id) & tmask;
    for (;;) {
        const unsigned long long prev = atomicCAS(&keys[h], DV_EMPTY, id);
        if (prev == DV_EMPTY || prev == id) break;
        h = (h + 1) & tmask;
    }
}

__device__ __forceinline__ void dv_note_row(const unsigned long long *keys, unsigned long long *rows, uint32_t tmask, unsigned long long id,
                                            int64_t row) {
    if (id == DV_EMPTY) return;
    uint32_t h = dv_hash(id) & tmask;
    for (;;) {
        const unsigned long long kx = keys[h];
        if (kx == DV_EMPTY) return;
        if (kx == id) {
            atomicMin(&rows[h], (unsigned long long)row);
            return;
        }
        h = (h + 1) & tmask;
    }
}

// blockIdx.x = list number, blockIdx.y = slice: rows slice * 1024 + {0, 256, 512, 768} + thread of the list, then gridDim.y * 1024
// further on -- four ids in flight per lane, each read coalesced
__global__ __launch_bounds__(256) void k_diverse_rows(const int64_t *ids, const int64_t *pt_off, const int32_t *pt_size,
                                                      const unsigned long long *keys, unsigned long long *rows, uint32_t tmask) {
    const int size = pt_size[blockIdx.x];  // (-1: no such list)
    if (size <= 0) return;
    const int64_t off = pt_off[blockIdx.x];
    for (int64_t r0 = (int64_t)blockIdx.y * 1024 + threadIdx.x; r0 < size; r0 += (int64_t)gridDim.y * 1024) {
        unsigned long long id[4];
#pragma unroll
        for (int u = 0; u < 4; u++) id[u] = r0 + 256 * u < size ? (unsigned long long)ids[off + r0 + 256 * u] : DV_EMPTY;
#pragma unroll
        for (int u = 0; u < 4; u++) dv_note_row(keys, rows, tmask, id[u], off + r0 + 256 * u);
    }
}

struct DivSelParams {
    const int64_t *cand_ids;  // [nq][C] the candidate search's rows: (key, id) order, padding -1 behind the candidates
    const float *cand_dist;   // [nq][C]
    const unsigned long long *keys, *rows;
    uint32_t tmask;
    const float4 *vecs;  // arena
    const float *norms;
    int nblk, C, k, metric, sqrt_l2;
    float lambda, mu;
    int64_t *out_ids;   // [nq][k]
    float *out_dist;    // [nq][k] or nullptr
    int32_t *out_rank;  // [nq][k] or nullptr
};

// ascending image of a float's order with -0 == +0 (NaN is classed apart by the caller)
__device__ __forceinline__ uint32_t dv_asc(float v) {
    uint32_t b = __float_as_uint(v);
    b = b == 0x80000000u ? 0u : b;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// One workgroup of 256 threads per query; thread i holds the candidate of rank i.  Dynamic LDS: STAGE_ALL: C rows of
// nblk * 16 + 4 floats (the pad keeps the 16-byte reads of 16 lanes on different banks); else one row of nblk * 16 floats.
template <bool STAGE_ALL>
__global__ __launch_bounds__(256) void k_diverse_select(DivSelParams S) {
    extern __shared__ float4 dv_lds4[];
    float *lds = (float *)dv_lds4;
    __shared__ unsigned long long wmin[4];
    __shared__ long long s_row[256];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = S.C, nblk = S.nblk, dpad = nblk * 16;
    const int64_t q = blockIdx.x;
    const bool l2 = S.metric == QK_METRIC_L2;
    const int64_t id = tid < C ? S.cand_ids[q * C + tid] : -1;
    const bool valid = id != -1;
    const float r = valid ? S.cand_dist[q * C + tid] : 0.f;
    // the arena row behind the id; -1 where the sweep found none (cannot happen for an id the search has just returned: such a
    // candidate's pairwise values are NaN, which the selection ignores)
    long long row = -1;
    if (valid) {
        uint32_t h = dv_hash((unsigned long long)id) & S.tmask;
        for (;;) {
            const unsigned long long kx = S.keys[h];
            if (kx == DV_EMPTY) break;
            if (kx == (unsigned long long)id) {
                const unsigned long long rr = S.rows[h];
                row = rr == DV_EMPTY ? -1 : (long long)rr;
                break;
            }
            h = (h + 1) & S.tmask;
        }
    }
    const float nrm = row >= 0 ? S.norms[row] : 0.f;
    s_row[tid] = row;
    const int cnt = __popcll(__ballot(valid));
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    const int n = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const int m = min(S.k, n);
    // padding behind the picks
    for (int j = m + tid; j < S.k; j += 256) {
        S.out_ids[q * S.k + j] = -1;
        if (S.out_dist) S.out_dist[q * S.k + j] = l2 ? INFINITY : -INFINITY;
        if (S.out_rank) S.out_rank[q * S.k + j] = -1;
    }
    if (m == 0) return;
    const int stride = dpad + 4;
    if (STAGE_ALL && m > 1) {
        // piece t of a row: block c = t / 4, g = t % 4 -> the float4 with columns 16 c + {g, 4 + g, 8 + g, 12 + g}
        const int per = nblk * 4;
        for (int e = tid; e < n * per; e += 256) {
            const int i = e / per, t = e - i * per, c = t >> 2, g = t & 3;
            const long long ri = s_row[i];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ri >= 0) v = S.vecs[((ri >> 4) * nblk + c) * 64 + g * 16 + (ri & 15)];
            float *dst = lds + (size_t)i * stride + 16 * c + g;
            dst[0] = v.x;
            dst[4] = v.y;
            dst[8] = v.z;
            dst[12] = v.w;
        }
    }
    bool picked = false;
    float N = NAN;  // the most similar pairwise value to the picked set; NaN: none yet
    int pick = 0;
    for (int j = 0;; j++) {
        if (tid == pick) {
            picked = true;
            S.out_ids[q * S.k + j] = id;
            if (S.out_dist) S.out_dist[q * S.k + j] = r;
            if (S.out_rank) S.out_rank[q * S.k + j] = pick;
        }
        if (j == m - 1) break;
        const long long prow = s_row[pick];
        const float pn = prow >= 0 ? S.norms[prow] : 0.f;
        if (!STAGE_ALL) {
            __syncthreads();  // (the readers of the previous step's vector are done)
            for (int t = tid; t < nblk * 4; t += 256) {
                const int c = t >> 2, g = t & 3;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (prow >= 0) v = S.vecs[((prow >> 4) * nblk + c) * 64 + g * 16 + (prow & 15)];
                float *dst = lds + 16 * c + g;
                dst[0] = v.x;
                dst[4] = v.y;
                dst[8] = v.z;
                dst[12] = v.w;
            }
        }
        __syncthreads();
        unsigned long long key = DV_EMPTY;
        if (valid && !picked) {
            float p = NAN;
            if (row >= 0 && prow >= 0) {
                float acc = 0.f;  // one chain, columns in natural order; the padded columns add +0 * +0
                if (STAGE_ALL) {
                    const float4 *a4 = (const float4 *)(lds + (size_t)tid * stride);
                    const float4 *b4 = (const float4 *)(lds + (size_t)pick * stride);
                    for (int c4 = 0; c4 < nblk * 4; c4++) {
                        const float4 a = a4[c4], b = b4[c4];
                        acc = __fmaf_rn(a.x, b.x, acc);
                        acc = __fmaf_rn(a.y, b.y, acc);
                        acc = __fmaf_rn(a.z, b.z, acc);
                        acc = __fmaf_rn(a.w, b.w, acc);
                    }
                } else {
                    const float4 *base = S.vecs + ((row >> 4) * nblk) * 64 + (row & 15);
                    for (int c = 0; c < nblk; c++) {
                        const float4 v0 = base[c * 64], v1 = base[c * 64 + 16], v2 = base[c * 64 + 32], v3 = base[c * 64 + 48];
                        const float4 *b4 = (const float4 *)(lds + 16 * c);
                        const float4 b0 = b4[0], b1 = b4[1], b2 = b4[2], b3 = b4[3];
                        acc = __fmaf_rn(v0.x, b0.x, acc);
                        acc = __fmaf_rn(v1.x, b0.y, acc);
                        acc = __fmaf_rn(v2.x, b0.z, acc);
                        acc = __fmaf_rn(v3.x, b0.w, acc);
                        acc = __fmaf_rn(v0.y, b1.x, acc);
                        acc = __fmaf_rn(v1.y, b1.y, acc);
                        acc = __fmaf_rn(v2.y, b1.z, acc);
                        acc = __fmaf_rn(v3.y, b1.w, acc);
                        acc = __fmaf_rn(v0.z, b2.x, acc);
                        acc = __fmaf_rn(v1.z, b2.y, acc);
                        acc = __fmaf_rn(v2.z, b2.z, acc);
                        acc = __fmaf_rn(v3.z, b2.w, acc);
                        acc = __fmaf_rn(v0.w, b3.x, acc);
                        acc = __fmaf_rn(v1.w, b3.y, acc);
                        acc = __fmaf_rn(v2.w, b3.z, acc);
                        acc = __fmaf_rn(v3.w, b3.w, acc);
                    }
                }
                if (l2) {
                    p = l2_expanded(nrm, pn, acc);
                    if (S.sqrt_l2) p = sqrtf(p);
                } else {
                    p = acc;
                }
            }
            if (p == p) N = (N != N) ? p : (l2 ? (p < N ? p : N) : (p > N ? p : N));
            const float a = __fmul_rn(S.lambda, r);
            const float cost = (N == N) ? __fsub_rn(a, __fmul_rn(S.mu, N)) : a;
            const bool isnan_ = cost != cost;
            const uint32_t o = isnan_ ? 0u : (l2 ? dv_asc(cost) : ~dv_asc(cost));
            key = ((unsigned long long)(isnan_ ? 1 : 0) << 40) | ((unsigned long long)o << 8) | (unsigned long long)tid;
        }
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) {
            const unsigned long long other = __shfl_xor(key, sft, 64);
            key = other < key ? other : key;
        }
        if (lane == 0) wmin[wave] = key;
        __syncthreads();
        unsigned long long best = wmin[0];
#pragma unroll
        for (int w = 1; w < 4; w++) best = wmin[w] < best ? wmin[w] : best;
        if (best == DV_EMPTY) break;  // (m <= n: an unpicked candidate always remains)
        pick = (int)(best & 0xFF);  // (wmin is rewritten behind the next step's barrier)
    }
}

struct DivOut {
    int64_t *ids;
    float *dist;
    int32_t *rank;
};

int dv_reserve(qk_ctx *ctx, size_t need) {
    if (need <= ctx->div_cap) return QK_OK;
    // (an earlier call's kernels may still read the old buffer: hipFree waits for the device)
    if (ctx->div_buf) QK_HIP(hipFree(ctx->div_buf));
    ctx->div_buf = nullptr;
    ctx->div_cap = 0;
    ctx->scratch_reallocs++;
    const size_t cap = need + need / 4;
    if (hipMalloc((void **)&ctx->div_buf, cap) != hipSuccess) {
        (void)hipGetLastError();
        QK_FAIL(QK_ERR_OOM, "diversified search: no device memory for %zu bytes of candidates", cap);
    }
    ctx->div_cap = cap;
    return QK_OK;
}

// the body of both entry points: parent == nullptr && pids == nullptr -> every list
int diverse_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
                int k, int fetch_k, float lambda, int metric, qk_filter *filter, const DivOut &out, int mem, qk_timing *timing) {
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (fetch_k < k) QK_FAIL(QK_ERR_INVALID, "%s: fetch_k=%d must be at least k=%d", who, fetch_k, k);
    if (fetch_k > QK_MAX_FETCH_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_MAX_FETCH_K=%d", who, fetch_k, QK_MAX_FETCH_K);
    if (!(lambda >= 0.0f && lambda <= 1.0f)) QK_FAIL(QK_ERR_INVALID, "%s: lambda=%g must lie in [0, 1]", who, (double)lambda);
    if (Q < 0 || (Q > 0 && (!x || !out.ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (mem == QK_MEM_HOST && pids) {
        for (int64_t i = 0; i < Q * (int64_t)P; i++) {
            const int64_t p = pids[i];
            if (p < 0) continue;
            if (p >= (int64_t)s->parts.size() || !s->parts[p].present)
                QK_FAIL(QK_ERR_NOT_FOUND, "List does not exist in get_codes (list %lld)", (long long)p);
        }
    }
    QK_TRY(qk_check_overflow(ctx));
    QK_HIP(hipSetDevice(ctx->device));
    if (timing) memset(timing, 0, sizeof(*timing));
    if (Q == 0) return QK_OK;
    const int C = fetch_k, d = s->d;
    hipStream_t st = ctx->stream;
    const bool host = mem == QK_MEM_HOST;
    // ---- the call's buffer: [candidate ids] [candidate distances] [table keys | table rows], and for a host caller [x] [pids]
    // [out ids] [out dist] [out rank]
    const int64_t gq = std::max<int64_t>(1, std::min<int64_t>(Q, DV_GROUP_CANDS / C));  // queries per table
    int64_t T = 64;
    while (T < 2 * gq * C) T <<= 1;
    const size_t b_ci = qk_al256((size_t)Q * C * 8), b_cd = qk_al256((size_t)Q * C * 4), b_t = qk_al256((size_t)T * 8);
    const size_t b_x = host ? qk_al256((size_t)Q * d * 4) : 0, b_p = host && pids ? qk_al256((size_t)Q * P * 8) : 0;
    const size_t b_oi = host ? qk_al256((size_t)Q * k * 8) : 0, b_o4 = host ? qk_al256((size_t)Q * k * 4) : 0;
    QK_TRY(dv_reserve(ctx, b_ci + b_cd + 2 * b_t + b_x + b_p + b_oi + 2 * b_o4));
    char *b = ctx->div_buf;
    int64_t *cand_ids = (int64_t *)b;
    float *cand_dist = (float *)(b + b_ci);
    unsigned long long *tkeys = (unsigned long long *)(b + b_ci + b_cd), *trows = (unsigned long long *)(b + b_ci + b_cd + b_t);
    char *hb = b + b_ci + b_cd + 2 * b_t;
    const float *dx = x;
    const int64_t *dpids = pids;
    DivOut dv = out;
    if (host) {
        // (pageable sources: copied out when the calls return)
        QK_HIP(hipMemcpyAsync(hb, x, (size_t)Q * d * 4, hipMemcpyHostToDevice, st));
        dx = (const float *)hb;
        if (pids) {
            QK_HIP(hipMemcpyAsync(hb + b_x, pids, (size_t)Q * P * 8, hipMemcpyHostToDevice, st));
            dpids = (const int64_t *)(hb + b_x);
        }
        dv.ids = (int64_t *)(hb + b_x + b_p);
        dv.dist = out.dist ? (float *)(hb + b_x + b_p + b_oi) : nullptr;
        dv.rank = out.rank ? (int32_t *)(hb + b_x + b_p + b_oi + b_o4) : nullptr;
    }
    // ---- the candidates: the shipped search with k = fetch_k into the call's buffer; its scalars and events are read behind the tail
    QK_TRY(qk_store_sync_table(s));
    qk_timing ct;
    memset(&ct, 0, sizeof(ct));
    QK_TRY(qk_run_search(ctx, parent, s, dx, Q, dpids, P, nprobe, C, metric, cand_ids, cand_dist, QK_MEM_DEVICE, timing ? &ct : nullptr, false,
                         true, nullptr, filter));
    // ---- the tail, per group of queries: table, sweep, selection
    DivSelParams S;
    S.keys = tkeys;
    S.rows = trows;
    S.tmask = (uint32_t)(T - 1);
    S.vecs = (const float4 *)s->vecs;
    S.norms = s->norms;
    S.nblk = s->nblk;
    S.C = C;
    S.k = k;
    S.metric = metric;
    S.sqrt_l2 = ctx->squared_l2 ? 0 : 1;
    S.lambda = lambda;
    S.mu = 1.0f - lambda;
    const size_t lds_all = (size_t)C * (s->nblk * 16 + 4) * 4, lds_one = (size_t)s->nblk * 16 * 4;
    const bool stage_all = QK_DIVERSE_STAGE_ALL && k > 1 && lds_all <= DV_STAGE_ALL_LDS;
    const size_t lds = stage_all ? lds_all : lds_one;
    if (lds > 48 * 1024) {
        if (stage_all) QK_HIP(hipFuncSetAttribute((const void *)k_diverse_select<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        else QK_HIP(hipFuncSetAttribute((const void *)k_diverse_select<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const int64_t nl = (int64_t)s->parts.size();
    const unsigned ny = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (s->max_size + 1023) / 1024));
    for (int64_t q0 = 0; q0 < Q; q0 += gq) {
        const int64_t nq = std::min(gq, Q - q0);
        QK_HIP(hipMemsetAsync(tkeys, 0xFF, 2 * b_t, st));  // keys and rows, adjacent
        hipLaunchKernelGGL(k_diverse_insert, dim3((unsigned)((nq * C + 255) / 256)), dim3(256), 0, st, cand_ids + q0 * C, nq * C, tkeys,
                           S.tmask);
        if (nl > 0)
            hipLaunchKernelGGL(k_diverse_rows, dim3((unsigned)nl, ny), dim3(256), 0, st, (const int64_t *)s->ids, (const int64_t *)s->d_off,
                               (const int32_t *)s->d_size, (const unsigned long long *)tkeys, trows, S.tmask);
        S.cand_ids = cand_ids + q0 * C;
        S.cand_dist = cand_dist + q0 * C;
        S.out_ids = dv.ids + q0 * k;
        S.out_dist = dv.dist ? dv.dist + q0 * k : nullptr;
        S.out_rank = dv.rank ? dv.rank + q0 * k : nullptr;
        if (stage_all) hipLaunchKernelGGL(k_diverse_select<true>, dim3((unsigned)nq), dim3(256), lds, st, S);
        else hipLaunchKernelGGL(k_diverse_select<false>, dim3((unsigned)nq), dim3(256), lds, st, S);
        QK_HIP(hipGetLastError());
    }
    const bool tm = ctx->timing && timing;
    hipEvent_t tail_end = nullptr;
    if (tm) {
        QK_HIP(hipEventCreate(&tail_end));
        if (hipEventRecord(tail_end, st) != hipSuccess) {
            (void)hipEventDestroy(tail_end);
            QK_FAIL(QK_ERR_HIP, "%s: hipEventRecord failed", who);
        }
    }
    // ---- results back ------------------------------------------------------------------------------------------------------------
    int rc = QK_OK;
    if (host) {
        hipError_t e = hipMemcpyAsync(out.ids, dv.ids, (size_t)Q * k * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out.dist) e = hipMemcpyAsync(out.dist, dv.dist, (size_t)Q * k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out.rank) e = hipMemcpyAsync(out.rank, dv.rank, (size_t)Q * k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            qk_set_error("%s: copying the results back -> %s", who, hipGetErrorString(e));
            rc = QK_ERR_HIP;
        }
    }
    if (rc == QK_OK && timing) {
        // the candidate search's figures (the one-launch small-batch search leaves no scalars: n_items -1), then the tail on top of
        // total_ms
        *timing = ct;
        if (ct.n_items < 0) {
            timing->n_items = 0;
            if (hipStreamSynchronize(st) != hipSuccess) rc = QK_ERR_HIP;
            float ms = 0.f;
            if (rc == QK_OK && tm && hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[7]) == hipSuccess) timing->scan_ms = timing->total_ms = ms;
        } else {
            rc = qk_finish_timing(ctx, s, timing, parent != nullptr, 4);
        }
        float ms = 0.f;
        if (rc == QK_OK && tm && hipEventElapsedTime(&ms, ctx->ev[7], tail_end) == hipSuccess) timing->total_ms += ms;
    }
    if (tail_end) (void)hipEventDestroy(tail_end);
    QK_TRY(rc);
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

}  // namespace

extern "C" {

int qk_diverse_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, float lambda,
                      int metric, qk_filter *filter, int64_t *out_ids, float *out_dist, int32_t *out_rank, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_diverse_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_diverse_search: nprobe must be positive");
    const DivOut out{out_ids, out_dist, out_rank};
    return diverse_run("qk_diverse_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, lambda, metric, filter, out, mem, timing);
}

int qk_diverse_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, float lambda,
                    int metric, qk_filter *filter, int64_t *out_ids, float *out_dist, int32_t *out_rank, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_diverse_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_diverse_scan: bad partition id list");
    const DivOut out{out_ids, out_dist, out_rank};
    return diverse_run("qk_diverse_scan", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, lambda, metric, filter, out, mem, timing);
}

}  // extern "C"
