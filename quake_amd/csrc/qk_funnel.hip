// qk_funnel.hip -- funnel search (include/quake_hip.h, "funnel search"): the fetch_k rows of every query's probed
// lists with the smallest keys over a column PREFIX, re-scored on the full vector, the k best under (exact key, id) returned.
// The store is tile-major: block c of every 16-row tile holds columns 16c .. 16c+15, so the first d' columns of every row are the
// first d'/16 blocks of every tile -- contiguous 1 KiB pieces.  One enqueue on the context's stream, no host wait inside:
//   k_funnel_prep      the queries' prefix in B-operand lane order (nblk' blocks) and its canonical norms
//   (coarse, grouping: the shipped ones)
//   k_scan_prefix      the tile form's body (qk_scan_body.inc, QK_SCAN_PREFIX) walking the first nblk' blocks of every tile, tiles
//                      strided by the store's nblk; norms of the prefixes; candidates named by arena row, no id stream; unseeded
//   (record merge: the shipped one, over (prefix key, arena row) with k = fetch_k, into the context's funnel buffer)
//   k_funnel_finish    one workgroup per query: exact keys of the candidates by a gathered MFMA, selection of the k best in LDS
// and, once per (store version, prefix_dim) and only for L2, k_prefix_norms: the store's norm arithmetic over d' columns.
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"
#include "qk_scan_opts.h"

#include <algorithm>
#include <cstring>

namespace {

// ---- prefix side data ------------------------------------------------------------------------------------------------------------
// blockIdx.x = list, blockIdx.y = slice of its rows: pn[row] = the k-ordered fmaf chain over columns 0 .. 16 nbp - 1 of the row (the
// padded columns of a last block hold +0: they leave the chain's value as it is, so nbp == nblk gives the stored norm's bits)
__global__ __launch_bounds__(256) void k_prefix_norms(const float4 *__restrict__ vecs, int nblk, int nbp, const int64_t *pt_off,
                                                      const int32_t *pt_size, float *__restrict__ pn) {
    const int size = pt_size[blockIdx.x];  // (-1: no such list)
    if (size <= 0) return;
    const int64_t off = pt_off[blockIdx.x];
    for (int64_t r = (int64_t)blockIdx.y * 256 + threadIdx.x; r < size; r += (int64_t)gridDim.y * 256) {
        const int64_t row = off + r;
        const float4 *base = vecs + ((row >> 4) * nblk) * 64 + (row & 15);
        float acc = 0.f;
        for (int c = 0; c < nbp; c++) {
            const float4 v0 = base[c * 64], v1 = base[c * 64 + 16], v2 = base[c * 64 + 32], v3 = base[c * 64 + 48];
            // piece g holds columns 16 c + {g, 4 + g, 8 + g, 12 + g}: ascending columns are v0.x v1.x v2.x v3.x v0.y ...
            acc = __fmaf_rn(v0.x, v0.x, acc);
            acc = __fmaf_rn(v1.x, v1.x, acc);
            acc = __fmaf_rn(v2.x, v2.x, acc);
            acc = __fmaf_rn(v3.x, v3.x, acc);
            acc = __fmaf_rn(v0.y, v0.y, acc);
            acc = __fmaf_rn(v1.y, v1.y, acc);
            acc = __fmaf_rn(v2.y, v2.y, acc);
            acc = __fmaf_rn(v3.y, v3.y, acc);
            acc = __fmaf_rn(v0.z, v0.z, acc);
            acc = __fmaf_rn(v1.z, v1.z, acc);
            acc = __fmaf_rn(v2.z, v2.z, acc);
            acc = __fmaf_rn(v3.z, v3.z, acc);
            acc = __fmaf_rn(v0.w, v0.w, acc);
            acc = __fmaf_rn(v1.w, v1.w, acc);
            acc = __fmaf_rn(v2.w, v2.w, acc);
            acc = __fmaf_rn(v3.w, v3.w, acc);
        }
        pn[row] = acc;
    }
}

// ---- query preparation ------------------------------------------------------------------------------------------------------------
// One wave per query: xq4p[(q nbp + c) 4 + g] = {x[q][16c+g], x[q][16c+g+4], x[q][16c+g+8], x[q][16c+g+12]} for the columns under dp
// (+0 beyond), xnp[q] = the canonical norm of x[q][0 .. dp).  (A sibling of k_prep_queries: that kernel's launches stay as they are.)
__global__ __launch_bounds__(64) void k_funnel_prep(const float *__restrict__ x, int d, int dp, int nbp, float4 *__restrict__ xq4p,
                                                    float *__restrict__ xnp) {
    const int64_t q = blockIdx.x;
    const float *s = x + q * d;
    for (int t = threadIdx.x; t < nbp * 4; t += 64) {
        const int col = 16 * (t >> 2) + (t & 3);
        float4 v;
        v.x = col < dp ? s[col] : 0.0f;
        v.y = col + 4 < dp ? s[col + 4] : 0.0f;
        v.z = col + 8 < dp ? s[col + 8] : 0.0f;
        v.w = col + 12 < dp ? s[col + 12] : 0.0f;
        xq4p[q * nbp * 4 + t] = v;
    }
    if (threadIdx.x == 0) {
        float acc = 0.0f;
        for (int k = 0; k < dp; k++) acc = __fmaf_rn(s[k], s[k], acc);
        xnp[q] = acc;
    }
}

// ---- the prefix scan --------------------------------------------------------------------------------------------------------------
// The tile form's body once more (see qk_scan_body.inc).  Its own kernel in its own translation unit: no instantiation of k_scan
// changes.
template <int DB, int MAXCH, bool L2>
__global__ __launch_bounds__(256) void k_scan_prefix(ScanParams P) {
    constexpr int MODE = 0;
#define QK_SCAN_FILT 0
#define QK_SCAN_PREFIX
#include "qk_scan_body.inc"
#undef QK_SCAN_PREFIX
#undef QK_SCAN_FILT
}

template <int DB, int MAXCH>
int launch_scan_prefix(dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_prefix<DB, MAXCH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_prefix<DB, MAXCH, true>), grid, block, lds, st, sp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_prefix<DB, MAXCH, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_prefix<DB, MAXCH, false>), grid, block, lds, st, sp);
    }
    return QK_OK;
}

// ---- the exact finish -------------------------------------------------------------------------------------------------------------
constexpr int FN_U = 4;  // blocks per load group: two groups of 4 x 16 B per lane in flight

// One workgroup of four waves per query.  A wave takes 16 candidates at a time and gathers them as the A operand of
// v_mfma_f32_16x16x4_f32: lane (g, r) loads, for every block c, the float4 of candidate r at (tile_r nblk + c) 64 + 16 g + pos_r --
// that piece is in the operand's lane order already.  The B operand is the query's block from LDS (staged once per workgroup),
// the same for all 16 columns: 15 of the 16 output columns repeat the first, which is fine -- the kernel is a gather bound by its
// loads, and this way all 64 lanes carry useful 16-byte loads.  x, y, z, w of every block in ascending c is the canonical chain
// (DESIGN.md 3): the key is the one the scan computes for the pair.  Lane (j < 4, g) then owns candidate 4 g + j of the 16: its norm
// and id come from the lane that loaded them (issued with the first block), its exact ordered key and id go to the workgroup's
// pool in LDS -- unless the key is NaN's.  Wave 0 selects the k best under (key, id) with compact_pool and writes the row as the
// merge writes it.  Dynamic LDS: [nblk * 4] float4 query | [64 MAXCH] int64 ids | [64 MAXCH] uint32 keys.
template <int MAXCH>
__global__ __launch_bounds__(256) void k_funnel_finish(FunnelFinishParams F) {
    extern __shared__ float4 fn_lds4[];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nblk = F.nblk, C = F.C, k = F.k;
    const int64_t q = blockIdx.x;
    const bool l2 = F.metric == QK_METRIC_L2;
    float4 *qs = fn_lds4;
    int64_t *pool_id = (int64_t *)(fn_lds4 + (size_t)nblk * 4);
    uint32_t *pool_ord = (uint32_t *)(pool_id + 64 * MAXCH);
    for (int t = tid; t < nblk * 4; t += 256) qs[t] = F.xq4[q * nblk * 4 + t];
    if (tid == 0) s_cnt = 0;
    const float xnq = l2 ? F.xn[q] : 0.f;
    __syncthreads();
    for (int b0 = wave * 16; b0 < C; b0 += 64) {
        const int ci = b0 + r;
        const int64_t row = ci < C ? F.cand[q * C + ci] : -1;
        if (__ballot(row >= 0) == 0) continue;  // (padding only: nothing to gather; uniform)
        const int64_t rs = row >= 0 ? row : 0;  // (a lane without a candidate gathers row 0 of the arena and drops the result)
        const float4 *base = F.vecs + ((rs >> 4) * nblk) * 64 + 16 * g + (rs & 15);
        float4 a0[FN_U], a1[FN_U];
#define FN_LOAD(A, C0)                                                                       \
    _Pragma("unroll") for (int u_ = 0; u_ < FN_U; u_++) A[u_] = base[(int64_t)min((C0) + u_, nblk - 1) * 64];
#define FN_STEP(A, C0)                                                                       \
    _Pragma("unroll") for (int u_ = 0; u_ < FN_U; u_++) if ((C0) + u_ < nblk) {              \
        const float4 bq_ = qs[((C0) + u_) * 4 + g];                                          \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].x, bq_.x, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].y, bq_.y, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].z, bq_.z, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].w, bq_.w, acc, 0, 0, 0);            \
    }
        FN_LOAD(a0, 0)
        const float nrm_r = F.norms[rs];
        const int64_t id_r = F.ids[rs];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < nblk; c0 += 2 * FN_U) {
            FN_LOAD(a1, c0 + FN_U)
            FN_STEP(a0, c0)
            FN_LOAD(a0, c0 + 2 * FN_U)
            FN_STEP(a1, c0 + FN_U)
        }
#undef FN_LOAD
#undef FN_STEP
        // acc[reg] of lane (j, g) = candidate 4 g + reg against the query (the same in every column j)
        const int src = 4 * g + (r & 3);  // the lane of group 0 that loaded the candidate this lane owns
        const float nrm = __shfl(nrm_r, src, 64);
        const int64_t id = __shfl(id_r, src, 64);
        const int64_t row_o = __shfl(row, src, 64);
        const float v = (r & 3) == 0 ? acc[0] : (r & 3) == 1 ? acc[1] : (r & 3) == 2 ? acc[2] : acc[3];
        const uint32_t o = l2 ? ord_from_l2(l2_expanded(xnq, nrm, v)) : ord_from_ip(v);
        if (r < 4 && row_o >= 0 && o != 0xFFFFFFFFu) {
            const int slot = atomicAdd(&s_cnt, 1);  // (at most C <= 64 MAXCH; the order of arrival does not reach the result)
            pool_ord[slot] = o;
            pool_id[slot] = id;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    const int cnt = compact_pool<MAXCH>(pool_ord, pool_id, s_cnt, k, lane);
    for (int e = lane; e < k; e += 64) {
        int64_t oid = -1;
        float od = l2 ? INFINITY : -INFINITY;
        if (e < cnt) {
            oid = pool_id[e];
            const uint32_t o = pool_ord[e];
            if (l2) {
                const float d2 = __uint_as_float(o);
                od = F.sqrt_l2 ? sqrtf(d2) : d2;
            } else {
                od = ip_from_ord(o);
            }
        }
        F.out_ids[q * k + e] = oid;
        if (F.out_dist) F.out_dist[q * k + e] = od;
    }
}

template <int MAXCH>
int launch_finish(hipStream_t st, const FunnelFinishParams &fp, int64_t Q) {
    const size_t lds = (size_t)fp.nblk * 64 + (size_t)64 * MAXCH * 12;
    if (lds > 48 * 1024) QK_HIP(hipFuncSetAttribute((const void *)k_funnel_finish<MAXCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_funnel_finish<MAXCH>, dim3((unsigned)Q), dim3(256), lds, st, fp);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

}  // namespace

int qk_launch_funnel_finish(hipStream_t st, const FunnelFinishParams &fp, int64_t Q) {
    const int maxch = pick_maxch(fp.C);
    return maxch == 1 ? launch_finish<1>(st, fp, Q) : maxch == 2 ? launch_finish<2>(st, fp, Q) : maxch == 4 ? launch_finish<4>(st, fp, Q)
                                                                                                       : launch_finish<8>(st, fp, Q);
}

int qk_fn_reserve(qk_ctx *ctx, size_t need) {
    if (need <= ctx->fn_cap) return QK_OK;
    // (an earlier call's kernels may still read the old buffer: hipFree waits for the device)
    if (ctx->fn_buf) QK_HIP(hipFree(ctx->fn_buf));
    ctx->fn_buf = nullptr;
    ctx->fn_cap = 0;
    ctx->scratch_reallocs++;
    const size_t cap = need + need / 4;
    if (hipMalloc((void **)&ctx->fn_buf, cap) != hipSuccess) {
        (void)hipGetLastError();
        QK_FAIL(QK_ERR_OOM, "funnel search: no device memory for %zu bytes of prefix queries and candidates", cap);
    }
    ctx->fn_cap = cap;
    return QK_OK;
}

namespace {

// the body of both entry points: parent == nullptr && pids == nullptr -> every list
int funnel_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
               int k, int fetch_k, int prefix_dim, int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    const int d = s->d;
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (prefix_dim < 16 || prefix_dim > d || (prefix_dim % 16 != 0 && prefix_dim != d))
        QK_FAIL(QK_ERR_INVALID, "%s: prefix_dim=%d must lie in [16, d=%d] and be a multiple of 16 or equal to d", who, prefix_dim, d);
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (fetch_k < k) QK_FAIL(QK_ERR_INVALID, "%s: fetch_k=%d must be at least k=%d", who, fetch_k, k);
    if (Q < 0 || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (prefix_dim > QK_FUNNEL_MAX_PREFIX)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: prefix_dim=%d exceeds QK_FUNNEL_MAX_PREFIX=%d", who, prefix_dim, QK_FUNNEL_MAX_PREFIX);
    if (fetch_k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_MAX_K=%d", who, fetch_k, QK_MAX_K);
    if (d > QK_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_MAX_D=%d", who, d, QK_MAX_D);
    if (!parent && !pids && s->nlist == 1)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a flat index without lists of its own takes the dense path, which has no prefix form", who);
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
    hipStream_t st = ctx->stream;
    const bool host = mem == QK_MEM_HOST;
    const bool l2 = metric == QK_METRIC_L2;
    const int C = fetch_k, nblk = s->nblk, nbp = (prefix_dim + 15) / 16;
    // ---- side data and the call's buffer: what can fail for want of memory comes first ----------------------------------------------
    QK_TRY(qk_store_sync_table(s));
    const float *pnorms = s->norms;  // (IP: the key reads no norm; the scan's norm stream still needs memory to load from)
    if (l2) QK_TRY(qk_store_prefix_norms(ctx, s, prefix_dim, &pnorms));
    const size_t b_q = qk_al256((size_t)Q * nbp * 64), b_n = qk_al256((size_t)Q * 4), b_c = qk_al256((size_t)Q * C * 8);
    QK_TRY(qk_fn_reserve(ctx, b_q + b_n + b_c));
    float4 *xq4p = (float4 *)ctx->fn_buf;
    float *xnp = (float *)(ctx->fn_buf + b_q);
    int64_t *cand = (int64_t *)(ctx->fn_buf + b_q + b_n);
    // ---- staging, full query preparation, coarse (the unfiltered qk_search's) -------------------------------------------------------
    const size_t b_oi = qk_al256((size_t)Q * k * 8), b_od = qk_al256((size_t)Q * k * 4);
    qk_scan_args sa;
    char *stage = nullptr;
    bool have_coarse = false;
    QK_TRY(qk_emit_front_end(ctx, parent, s, x, Q, pids, P, nprobe, metric, mem, b_oi + b_od, timing != nullptr, &sa, &stage, &have_coarse));
    int64_t *d_ids = host ? (int64_t *)stage : out_ids;
    float *d_dist = host ? (out_dist ? (float *)(stage + b_oi) : nullptr) : out_dist;
    const float4 *xq4_full = sa.xq4;
    const float *xn_full = sa.xn;
    hipLaunchKernelGGL(k_funnel_prep, dim3((unsigned)Q), dim3(64), 0, st, sa.x, d, prefix_dim, nbp, xq4p, xnp);
    QK_HIP(hipGetLastError());
    // ---- the candidates: the prefix scan with k = fetch_k; the merge leaves arena rows in the call's buffer --------------------------
    sa.xq4 = xq4p;
    sa.xn = xnp;
    sa.prefix_nblk = nbp;
    sa.prefix_norms = pnorms;
    sa.k = C;
    sa.out_ids = cand;
    sa.out_dist = nullptr;
    sa.record_events = timing != nullptr;
    QK_TRY(qk_scan_device(ctx, s, sa, timing, 4));
    // ---- the exact finish -----------------------------------------------------------------------------------------------------------
    FunnelFinishParams fp;
    fp.cand = cand;
    fp.xq4 = xq4_full;
    fp.xn = xn_full;
    fp.vecs = (const float4 *)s->vecs;
    fp.norms = s->norms;
    fp.ids = s->ids;
    fp.nblk = nblk;
    fp.C = C;
    fp.k = k;
    fp.metric = metric;
    fp.sqrt_l2 = ctx->squared_l2 ? 0 : 1;
    fp.out_ids = d_ids;
    fp.out_dist = d_dist;
    QK_TRY(qk_launch_funnel_finish(st, fp, Q));
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
        hipError_t e = hipMemcpyAsync(out_ids, d_ids, (size_t)Q * k * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out_dist) e = hipMemcpyAsync(out_dist, d_dist, (size_t)Q * k * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            qk_set_error("%s: copying the results back -> %s", who, hipGetErrorString(e));
            rc = QK_ERR_HIP;
        }
    }
    if (rc == QK_OK && timing) {
        // the candidate search's figures, then the finish on top of total_ms
        rc = qk_finish_timing(ctx, s, timing, have_coarse, 4);
        float ms = 0.f;
        if (rc == QK_OK && tm && hipEventElapsedTime(&ms, ctx->ev[7], tail_end) == hipSuccess) timing->total_ms += ms;
    }
    if (tail_end) (void)hipEventDestroy(tail_end);
    QK_TRY(rc);
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

}  // namespace

int qk_launch_scan_prefix(int db, int maxch, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
#define QK_CASEP(D, M) \
    if (db == D && maxch == M) return launch_scan_prefix<D, M>(grid, block, lds, st, sp);
    QK_CASEP(1, 1) QK_CASEP(1, 2) QK_CASEP(1, 4) QK_CASEP(1, 8) QK_CASEP(2, 1) QK_CASEP(2, 2) QK_CASEP(2, 4) QK_CASEP(2, 8)
    QK_CASEP(4, 1) QK_CASEP(4, 2) QK_CASEP(4, 4) QK_CASEP(4, 8) QK_CASEP(8, 1) QK_CASEP(8, 2) QK_CASEP(8, 4) QK_CASEP(8, 8)
#undef QK_CASEP
    QK_FAIL(QK_ERR_UNSUPPORTED, "no prefix scan kernel for DB=%d MAXCH=%d", db, maxch);
}

void qk_store_prefix_free(qk_store *s) {
    if (s->pnorms) hipFree(s->pnorms);
    s->pnorms = nullptr;
    s->pnorms_cap_rows = 0;
    s->pnorms_dim = 0;
}

int qk_store_prefix_norms(qk_ctx *ctx, qk_store *s, int prefix_dim, const float **out) {
    if (s->pnorms && s->pnorms_dim == prefix_dim && s->pnorms_version == s->version && s->pnorms_cap_rows >= s->cap_rows) {
        *out = s->pnorms;
        return QK_OK;
    }
    if (s->pnorms_cap_rows < s->cap_rows || !s->pnorms) {
        float *nn = nullptr;
        const int64_t rows = std::max<int64_t>(s->cap_rows, 16);
        if (hipMalloc((void **)&nn, (size_t)rows * 4) != hipSuccess) {
            (void)hipGetLastError();
            QK_FAIL(QK_ERR_OOM, "funnel search: no device memory for %lld bytes of prefix norms", (long long)rows * 4);
        }
        if (s->pnorms) hipFree(s->pnorms);  // (waits for the device: an earlier call may still read it)
        s->pnorms = nn;
        s->pnorms_cap_rows = rows;
    }
    s->pnorms_dim = 0;
    hipStream_t st = ctx->stream;
    // (rows of a last tile beyond its list's size are loaded by the scan and masked: keep them defined)
    QK_HIP(hipMemsetAsync(s->pnorms, 0, (size_t)s->pnorms_cap_rows * 4, st));
    const int64_t nl = (int64_t)s->parts.size();
    if (nl > 0 && s->vecs) {
        const unsigned ny = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (s->max_size + 255) / 256));
        hipLaunchKernelGGL(k_prefix_norms, dim3((unsigned)nl, ny), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, (prefix_dim + 15) / 16,
                           (const int64_t *)s->d_off, (const int32_t *)s->d_size, s->pnorms);
        QK_HIP(hipGetLastError());
    }
    QK_HIP(hipStreamSynchronize(st));  // (the one-off build: from here on every stream of the device may read the norms)
    s->pnorms_dim = prefix_dim;
    s->pnorms_version = s->version;
    *out = s->pnorms;
    return QK_OK;
}

extern "C" {

int qk_funnel_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int prefix_dim,
                     int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_funnel_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_funnel_search: nprobe must be positive");
    return funnel_run("qk_funnel_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, prefix_dim, metric, out_ids, out_dist, mem, timing);
}

int qk_funnel_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int prefix_dim,
                   int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_funnel_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_funnel_scan: bad partition id list");
    return funnel_run("qk_funnel_scan", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, prefix_dim, metric, out_ids, out_dist, mem, timing);
}

}  // extern "C"
