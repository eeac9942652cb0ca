// qk_sq8.hip -- quantized search (include/quake_hip.h, "quantized search"): scalar quantization with oversampling and
// rescoring.  Every coordinate of the store is mirrored as one int8 code; per query the fetch_k rows of its probed lists with the
// smallest integer keys over the codes are re-scored on the float32 rows, the k best under (exact key, id) returned.
// The code mirror keeps the arena's tile indexing: code row r is arena row r, and a 1 KiB code block holds 64 columns of a 16-row
// tile, lane (r, g) of the scan owning the 16 bytes of row r, columns 64c + 16g .. 64c + 16g + 15.  One enqueue on the context's
// stream, no host wait inside -- except the one-off build of the mirror:
//   k_sq8_range        min / max of every column (L2) or max |x| (IP) over the live rows, "non-finite seen"
//   k_sq8_encode       arena tiles -> code tiles and the rows' code norms
//   k_sq8_prep         the queries' codes in B-operand lane order and their code norms
//   (coarse, grouping: the shipped ones)
//   k_scan_sq8         the tile form's body (qk_scan_body.inc, QK_SCAN_SQ8): one v_mfma_i32_16x16x64_i8 per code block, exact integer keys,
//                      candidates named by arena row, no id stream; unseeded
//   (record merge: the shipped one, over (integer key, arena row) with k = fetch_k, into the context's candidate buffer)
//   (k_funnel_finish: the exact finish of funnel search, unchanged)
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"
#include "qk_scan_opts.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

typedef int qk_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ qk_i32x4 qk_as_i4(const float4 v) { return __builtin_bit_cast(qk_i32x4, v); }

// order-preserving image of a float (any sign) in the unsigned integers
__device__ __forceinline__ uint32_t sq8_img(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float sq8_from_img(uint32_t i) {
    const uint32_t b = (i & 0x80000000u) ? (i ^ 0x80000000u) : ~i;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// c = clamp(rint((x - m) / s), -127, 127): one float32 subtraction, one IEEE division, round half to even; NaN -> 0 (a query's only:
// the store refuses non-finite rows), +-inf -> +-127 by the clamp
__device__ __forceinline__ int sq8_code(float x, float m, float s) {
    if (x != x) return 0;
    const float r = rintf(__fdiv_rn(__fsub_rn(x, m), s));
    return (int)fminf(fmaxf(r, -127.0f), 127.0f);
}
__device__ __forceinline__ uint32_t sq8_pack(int a, int b, int c, int d) {
    return (uint32_t)(a & 0xFF) | ((uint32_t)(b & 0xFF) << 8) | ((uint32_t)(c & 0xFF) << 16) | ((uint32_t)(d & 0xFF) << 24);
}

// ---- the code parameters ---------------------------------------------------------------------------------------------------------
// stats [2 ncol + 4]: lo images [ncol] | hi images [ncol] | "non-finite seen" | the smallest list that holds one | bits of max |x| | -
__global__ void k_sq8_init(uint32_t *stats, int ncol) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * ncol + 4) stats[i] = (i < ncol || i == 2 * ncol + 1) ? 0xFFFFFFFFu : 0u;
}

// blockIdx.x = list, blockIdx.y = slice of its tiles, a wave per tile.  A lane reads the tile-major arena as the scan does: lane
// (g, r) of block c holds columns 16c + g + {0, 4, 8, 12} of row r.  L2: per block c the lanes fold their four columns over the
// wave's tiles in registers, the 16 rows by shuffles, the four waves through LDS, and 16 lanes end with atomicMin / atomicMax on the
// order-preserving images -- exact and independent of the order of arrival.  IP: one running max |x| per lane, one atomicMax per wave.
template <bool L2>
__global__ __launch_bounds__(256) void k_sq8_range(const float4 *__restrict__ vecs, int nblk, int ncol, const int64_t *__restrict__ pt_off,
                                                   const int32_t *__restrict__ pt_size, uint32_t *stats) {
    __shared__ float s_lo[4][16], s_hi[4][16];
    const int size = pt_size[blockIdx.x];  // (-1: no such list)
    if (size <= 0) return;
    const int64_t tile0 = pt_off[blockIdx.x] >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int ntl = (size + 15) >> 4;
    bool bad = false;
    float amax = 0.0f;
    for (int c = 0; c < nblk; c++) {
        float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
            if (t * 16 + r >= size) continue;  // rows behind the list's end are no rows
            const float4 v4 = vecs[((tile0 + t) * nblk + c) * 64 + lane];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bad |= !(fabsf(v[i]) <= FLT_MAX);  // (NaN: not <=)
                if (L2) {
                    lo[i] = fminf(lo[i], v[i]);
                    hi[i] = fmaxf(hi[i], v[i]);
                } else {
                    amax = fmaxf(amax, fabsf(v[i]));
                }
            }
        }
        if (L2) {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    lo[i] = fminf(lo[i], __shfl_xor(lo[i], o));
                    hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], o));
                }
            if (r == 0) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    s_lo[wv][g + 4 * i] = lo[i];  // column 16c + g + 4i
                    s_hi[wv][g + 4 * i] = hi[i];
                }
            }
            __syncthreads();
            if (threadIdx.x < 16 && 16 * c + (int)threadIdx.x < ncol) {
                const int j = threadIdx.x, col = 16 * c + j;
                const uint32_t il = sq8_img(fminf(fminf(s_lo[0][j], s_lo[1][j]), fminf(s_lo[2][j], s_lo[3][j])));
                const uint32_t ih = sq8_img(fmaxf(fmaxf(s_hi[0][j], s_hi[1][j]), fmaxf(s_hi[2][j], s_hi[3][j])));
                // (a stale read only costs the atomic it could have spared: the words move one way)
                if (il < stats[col]) atomicMin(&stats[col], il);
                if (ih > stats[ncol + col]) atomicMax(&stats[ncol + col], ih);
            }
            __syncthreads();
        }
    }
    if (!L2) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        // (non-negative floats order like their bit patterns; +inf arrives with the flag below)
        if (lane == 0 && __float_as_uint(amax) > stats[2 * ncol + 2]) atomicMax(&stats[2 * ncol + 2], __float_as_uint(amax));
    }
    if (__ballot(bad) != 0 && lane == 0) {
        atomicOr(&stats[2 * ncol], 1u);
        atomicMin(&stats[2 * ncol + 1], (uint32_t)blockIdx.x);
    }
}

// ---- arena tiles -> code tiles ---------------------------------------------------------------------------------------------------
// blockIdx.x = list, blockIdx.y = slice of its tiles, a wave per tile.  Lane (r, g) of code block c8 encodes the 16 columns of arena
// block 4 c8 + g of row r -- four float4, one from each of the block's lane groups -- and stores its 16 bytes at
// (tile nblk8 + c8) 1024 + 16 lane: byte t = column 64 c8 + 16 g + t.  The integer dot product is exact, so which K slot of
// v_mfma_i32_16x16x64_i8 the hardware gives to which of a lane's 16 bytes (and to which lane group) does not matter as long as the
// queries' codes use the same mapping: k_sq8_prep writes entry (c8, g), byte t, for the same column.  Rows of a last tile behind the
// list's size, columns from d on and blocks the arena does not have hold code 0.  nx[row] = the sum of the row's squared codes.
__global__ __launch_bounds__(256) void k_sq8_encode(const float4 *__restrict__ vecs, int nblk, int nblk8, int d, const int64_t *__restrict__ pt_off,
                                                    const int32_t *__restrict__ pt_size, const float *__restrict__ m, float scale,
                                                    uint4 *__restrict__ codes, int32_t *__restrict__ nx) {
    const int size = pt_size[blockIdx.x];
    if (size <= 0) return;
    const int64_t tile0 = pt_off[blockIdx.x] >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int ntl = (size + 15) >> 4;
    for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
        const int64_t tile = tile0 + t;
        const bool live = t * 16 + r < size;
        int n2 = 0;
        for (int c8 = 0; c8 < nblk8; c8++) {
            const int cb = 4 * c8 + g;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (live && cb < nblk) {
                const float4 *src = vecs + (tile * nblk + cb) * 64 + r;
                const float4 v0 = src[0], v1 = src[16], v2 = src[32], v3 = src[48];  // lane group gp: columns 16 cb + gp + {0, 4, 8, 12}
                const float x[16] = {v0.x, v1.x, v2.x, v3.x, v0.y, v1.y, v2.y, v3.y, v0.z, v1.z, v2.z, v3.z, v0.w, v1.w, v2.w, v3.w};
                int cd[16];
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int col = 16 * cb + j;
                    cd[j] = col < d ? sq8_code(x[j], m[col], scale) : 0;
                    n2 += cd[j] * cd[j];
                }
#pragma unroll
                for (int i = 0; i < 4; i++) w[i] = sq8_pack(cd[4 * i], cd[4 * i + 1], cd[4 * i + 2], cd[4 * i + 3]);
            }
            codes[(tile * nblk8 + c8) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        n2 += __shfl_xor(n2, 16);
        n2 += __shfl_xor(n2, 32);
        if (g == 0) nx[tile * 16 + r] = n2;
    }
}

// ---- query preparation ------------------------------------------------------------------------------------------------------------
// One wave per query, a sibling of k_funnel_prep: xq[(q nblk8 + c8) 4 + g] = the 16 codes of columns 64 c8 + 16 g .. + 15 (0 from d
// on), nq[q] = the sum of the squared codes.  L2 codes the query with the store's centres and scale; IP gives every query its own
// scale, max |q_j| over its finite coordinates / 127 (1 where that is 0) -- a positive factor of all of a query's keys, which the
// order of its candidates does not see, so it is not kept.
template <bool L2>
__global__ __launch_bounds__(64) void k_sq8_prep(const float *__restrict__ x, int d, int nblk8, const float *__restrict__ m, float scale,
                                                 uint4 *__restrict__ xq, int32_t *__restrict__ nq) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *s = x + q * d;
    float sc = scale;
    if (!L2) {
        float a = 0.0f;
        for (int j = lane; j < d; j += 64) {
            const float v = fabsf(s[j]);
            if (v <= FLT_MAX) a = fmaxf(a, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
        sc = __fdiv_rn(a, 127.0f);
        if (sc == 0.0f) sc = 1.0f;
    }
    int n2 = 0;
    for (int t = lane; t < nblk8 * 4; t += 64) {
        int cd[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int col = 16 * t + j;
            cd[j] = col < d ? sq8_code(s[col], L2 ? m[col] : 0.0f, sc) : 0;
            n2 += cd[j] * cd[j];
        }
        xq[q * nblk8 * 4 + t] = make_uint4(sq8_pack(cd[0], cd[1], cd[2], cd[3]), sq8_pack(cd[4], cd[5], cd[6], cd[7]),
                                           sq8_pack(cd[8], cd[9], cd[10], cd[11]), sq8_pack(cd[12], cd[13], cd[14], cd[15]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o);
    if (lane == 0) nq[q] = n2;
}

// ---- the code scan ----------------------------------------------------------------------------------------------------------------
// The tile form's body once more (see qk_scan_body.inc).  Its own kernel in its own translation unit: no instantiation of k_scan
// changes.
template <int DB, int MAXCH, bool L2>
__global__ __launch_bounds__(256) void k_scan_sq8(ScanParams P) {
    constexpr int MODE = 0;
#define QK_SCAN_FILT 0
#define QK_SCAN_SQ8
#include "qk_scan_body.inc"
#undef QK_SCAN_SQ8
#undef QK_SCAN_FILT
}

template <int DB, int MAXCH>
int launch_scan_sq8(dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_sq8<DB, MAXCH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_sq8<DB, MAXCH, true>), grid, block, lds, st, sp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_sq8<DB, MAXCH, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_sq8<DB, MAXCH, false>), grid, block, lds, st, sp);
    }
    return QK_OK;
}

}  // namespace

// the body of the entry points: parent == nullptr && pids == nullptr -> every list; deep: the candidates by counting (qk_sq8_deep.hip)
int qk_sq8_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe, int k,
               int fetch_k, int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing, bool deep) {
    const int d = s->d;
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (fetch_k < k) QK_FAIL(QK_ERR_INVALID, "%s: fetch_k=%d must be at least k=%d", who, fetch_k, k);
    if (Q < 0 || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (deep && k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d", who, k, QK_MAX_K);
    if (deep && fetch_k > QK_SQ8_MAX_FETCH) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_SQ8_MAX_FETCH=%d", who, fetch_k, QK_SQ8_MAX_FETCH);
    if (!deep && fetch_k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_MAX_K=%d", who, fetch_k, QK_MAX_K);
    if (d > QK_SQ8_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_SQ8_MAX_D=%d", who, d, QK_SQ8_MAX_D);
    if (!parent && !pids && s->nlist == 1)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a flat index without lists of its own takes the dense path, which has no int8 code form", who);
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
    const int C = fetch_k, nblk = s->nblk, nb8 = qk_sq8_nblk(d);
    // ---- the mirror and the call's buffer: what can refuse or fail for want of memory comes first -----------------------------------
    QK_TRY(qk_store_sync_table(s));
    QK_TRY(qk_store_sq8_mirror(ctx, s, metric));
    const size_t b_q = qk_al256((size_t)Q * nb8 * 64), b_n = qk_al256((size_t)Q * 4), b_c = deep ? qk_sq8_deep_bytes(Q, C) : qk_al256((size_t)Q * C * 8);
    QK_TRY(qk_fn_reserve(ctx, b_q + b_n + b_c));
    uint4 *xq = (uint4 *)ctx->fn_buf;
    int32_t *nq = (int32_t *)(ctx->fn_buf + b_q);
    int64_t *cand = (int64_t *)(ctx->fn_buf + b_q + b_n);
    Sq8DeepParams dd;
    if (deep) qk_sq8_deep_carve(ctx->fn_buf + b_q + b_n, Q, C, &dd);  // (the candidates first: cand as above)
    // ---- staging, full query preparation, coarse (the unfiltered qk_search's, on the float32 queries) -------------------------------
    const size_t b_oi = qk_al256((size_t)Q * k * 8), b_od = qk_al256((size_t)Q * k * 4);
    qk_scan_args sa;
    char *stage = nullptr;
    bool have_coarse = false;
    QK_TRY(qk_emit_front_end(ctx, parent, s, x, Q, pids, P, nprobe, metric, mem, b_oi + b_od, timing != nullptr, &sa, &stage, &have_coarse));
    int64_t *d_ids = host ? (int64_t *)stage : out_ids;
    float *d_dist = host ? (out_dist ? (float *)(stage + b_oi) : nullptr) : out_dist;
    const float4 *xq4_full = sa.xq4;
    const float *xn_full = sa.xn;
    QK_TRY(qk_launch_sq8_prep(st, s, sa.x, Q, metric, xq, nq));
    // ---- the candidates: the code scan with k = fetch_k; the merge leaves arena rows in the call's buffer ----------------------------
    sa.xq4 = (const float4 *)xq;
    sa.xn = (const float *)nq;
    sa.sq8_nblk = nb8;
    sa.sq8_codes = s->sq8_codes;
    sa.sq8_nx = s->sq8_nx;
    sa.k = deep ? 1 : C;  // (counting form: no pools; k sizes nothing that is used)
    if (deep) {
        sa.sq8_deep = &dd;
        QK_TRY(qk_launch_sq8_deep_init(st, dd, Q));
    }
    sa.out_ids = cand;
    sa.out_dist = nullptr;
    sa.record_events = timing != nullptr;
    QK_TRY(qk_scan_device(ctx, s, sa, timing, 4));
    if (deep) QK_TRY(qk_launch_sq8_resolve(s, sa, st));
    // ---- the exact finish: funnel search's ------------------------------------------------------------------------------------------
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
    QK_TRY(deep ? qk_launch_sq8_deep_finish(st, fp, Q) : qk_launch_funnel_finish(st, fp, Q));
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
        // the candidate search's figures (scan_bytes: code bytes), then the finish on top of total_ms
        rc = qk_finish_timing(ctx, s, timing, have_coarse, 4);
        float ms = 0.f;
        if (rc == QK_OK && tm && hipEventElapsedTime(&ms, ctx->ev[7], tail_end) == hipSuccess) timing->total_ms += ms;
        if (rc == QK_OK && deep) timing->scan_bytes *= 2;  // (the codes are streamed twice)
    }
    if (tail_end) (void)hipEventDestroy(tail_end);
    QK_TRY(rc);
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

int qk_launch_sq8_prep(hipStream_t st, const qk_store *s, const float *x, int64_t Q, int metric, uint4 *xq, int32_t *nq) {
    const int d = s->d, nb8 = qk_sq8_nblk(d);
    if (metric == QK_METRIC_L2)
        hipLaunchKernelGGL(k_sq8_prep<true>, dim3((unsigned)Q), dim3(64), 0, st, x, d, nb8, s->sq8_m, s->sq8_scale, xq, nq);
    else
        hipLaunchKernelGGL(k_sq8_prep<false>, dim3((unsigned)Q), dim3(64), 0, st, x, d, nb8, s->sq8_m, s->sq8_scale, xq, nq);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

int qk_launch_scan_sq8(int db, int maxch, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
#define QK_CASEQ(D, M) \
    if (db == D && maxch == M) return launch_scan_sq8<D, M>(grid, block, lds, st, sp);
    QK_CASEQ(1, 1) QK_CASEQ(1, 2) QK_CASEQ(1, 4) QK_CASEQ(1, 8) QK_CASEQ(2, 1) QK_CASEQ(2, 2) QK_CASEQ(2, 4) QK_CASEQ(2, 8)
    QK_CASEQ(4, 1) QK_CASEQ(4, 2) QK_CASEQ(4, 4) QK_CASEQ(4, 8) QK_CASEQ(8, 1) QK_CASEQ(8, 2) QK_CASEQ(8, 4) QK_CASEQ(8, 8)
#undef QK_CASEQ
    QK_FAIL(QK_ERR_UNSUPPORTED, "no int8 code scan kernel for DB=%d MAXCH=%d", db, maxch);
}

void qk_store_sq8_free(qk_store *s) {
    if (s->sq8_codes) hipFree(s->sq8_codes);
    if (s->sq8_nx) hipFree(s->sq8_nx);
    if (s->sq8_m) hipFree(s->sq8_m);
    if (s->sq8_stats) hipFree(s->sq8_stats);
    s->sq8_codes = nullptr;
    s->sq8_nx = nullptr;
    s->sq8_m = nullptr;
    s->sq8_stats = nullptr;
    s->sq8_cap_rows = 0;
    s->sq8_metric = -1;
}

int qk_store_sq8_mirror(qk_ctx *ctx, qk_store *s, int metric) {
    if (s->sq8_codes && s->sq8_metric == metric && s->sq8_version == s->version && s->sq8_cap_rows >= s->cap_rows) return QK_OK;
    const int d = s->d, nb8 = qk_sq8_nblk(d), ncol = nb8 * 64, nstat = 2 * ncol + 4;
    const bool l2 = metric == QK_METRIC_L2;
    if (s->sq8_cap_rows < s->cap_rows || !s->sq8_codes) {
        // (all four or none: a call without memory leaves the store as it was)
        const int64_t rows = (std::max<int64_t>(s->cap_rows, 16) + 15) & ~(int64_t)15;
        void *nc = nullptr, *nn = nullptr, *nm = nullptr, *ns = nullptr;
        if (hipMalloc(&nc, (size_t)rows * nb8 * 64) != hipSuccess || hipMalloc(&nn, (size_t)rows * 4) != hipSuccess ||
            hipMalloc(&nm, (size_t)ncol * 4) != hipSuccess || hipMalloc(&ns, (size_t)nstat * 4) != hipSuccess) {
            (void)hipGetLastError();
            if (nc) hipFree(nc);
            if (nn) hipFree(nn);
            if (nm) hipFree(nm);
            QK_FAIL(QK_ERR_OOM, "quantized search: no device memory for %lld bytes of int8 codes", (long long)rows * (nb8 * 64 + 4));
        }
        qk_store_sq8_free(s);  // (hipFree waits for the device: an earlier call may still read the old mirror)
        s->sq8_codes = nc;
        s->sq8_nx = (int32_t *)nn;
        s->sq8_m = (float *)nm;
        s->sq8_stats = (uint32_t *)ns;
        s->sq8_cap_rows = rows;
    }
    s->sq8_metric = -1;
    hipStream_t st = ctx->stream;
    const int64_t nl = (int64_t)s->parts.size();
    const bool rows_live = nl > 0 && s->vecs && s->ntotal > 0;
    const unsigned gy = nl >= 2048 ? 4 : nl >= 256 ? 16 : 64;  // (few lists: more workgroups per list)
    std::vector<uint32_t> h_stats(nstat, 0u);
    std::vector<float> h_m(ncol, 0.0f);
    float scale = 1.0f;
    if (rows_live) {
        hipLaunchKernelGGL(k_sq8_init, dim3((unsigned)((nstat + 255) / 256)), dim3(256), 0, st, s->sq8_stats, ncol);
        if (l2)
            hipLaunchKernelGGL(k_sq8_range<true>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, ncol,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, s->sq8_stats);
        else
            hipLaunchKernelGGL(k_sq8_range<false>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, ncol,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, s->sq8_stats);
        QK_HIP(hipGetLastError());
        QK_HIP(hipMemcpyAsync(h_stats.data(), s->sq8_stats, (size_t)nstat * 4, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
        if (h_stats[2 * ncol] != 0)
            QK_FAIL(QK_ERR_UNSUPPORTED, "quantized search: list %u holds a value that is not finite: no int8 codes for this store",
                    (unsigned)h_stats[2 * ncol + 1]);
        float num;
        if (l2) {
            float w = 0.0f;
            for (int j = 0; j < d; j++) {
                const float lo = sq8_from_img(h_stats[j]), hi = sq8_from_img(h_stats[ncol + j]);
                h_m[j] = 0.5f * lo + 0.5f * hi;
                w = std::max(w, hi - lo);
            }
            num = w / 254.0f;
        } else {
            float a;
            memcpy(&a, &h_stats[2 * ncol + 2], 4);
            num = a / 127.0f;
        }
        if (!std::isfinite(num)) QK_FAIL(QK_ERR_UNSUPPORTED, "quantized search: the range of the store's values has no finite int8 scale");
        scale = num == 0.0f ? 1.0f : num;
        QK_HIP(hipMemcpyAsync(s->sq8_m, h_m.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sq8_encode, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, nb8, d,
                           (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->sq8_m, scale, (uint4 *)s->sq8_codes, s->sq8_nx);
        QK_HIP(hipGetLastError());
    } else {
        QK_HIP(hipMemcpyAsync(s->sq8_m, h_m.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
    }
    QK_HIP(hipStreamSynchronize(st));  // (the one-off build: from here on every stream of the device may read the mirror)
    s->sq8_scale = scale;
    s->sq8_metric = metric;
    s->sq8_version = s->version;
    return QK_OK;
}

int qk_sq8_l2_centres(qk_ctx *ctx, qk_store *s, uint32_t *stats, int ncol, float *h_m, int64_t *bad_list) {
    hipStream_t st = ctx->stream;
    const int nstat = 2 * ncol + 4;
    const int64_t nl = (int64_t)s->parts.size();
    const unsigned gy = nl >= 2048 ? 4 : nl >= 256 ? 16 : 64;
    std::vector<uint32_t> h_stats(nstat, 0u);
    hipLaunchKernelGGL(k_sq8_init, dim3((unsigned)((nstat + 255) / 256)), dim3(256), 0, st, stats, ncol);
    hipLaunchKernelGGL(k_sq8_range<true>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, ncol,
                       (const int64_t *)s->d_off, (const int32_t *)s->d_size, stats);
    QK_HIP(hipGetLastError());
    QK_HIP(hipMemcpyAsync(h_stats.data(), stats, (size_t)nstat * 4, hipMemcpyDeviceToHost, st));
    QK_HIP(hipStreamSynchronize(st));
    *bad_list = h_stats[2 * ncol] != 0 ? (int64_t)h_stats[2 * ncol + 1] : -1;
    if (*bad_list >= 0) return QK_OK;
    for (int j = 0; j < ncol; j++) h_m[j] = j < s->d ? 0.5f * sq8_from_img(h_stats[j]) + 0.5f * sq8_from_img(h_stats[ncol + j]) : 0.0f;
    return QK_OK;
}

extern "C" {

int qk_sq8_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int metric,
                  int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_sq8_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_sq8_search: nprobe must be positive");
    return qk_sq8_run("qk_sq8_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, metric, out_ids, out_dist, mem, timing, false);
}

int qk_sq8_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int metric,
                int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_sq8_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_sq8_scan: bad partition id list");
    return qk_sq8_run("qk_sq8_scan", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, metric, out_ids, out_dist, mem, timing, false);
}

int qk_store_sq8_info(qk_store *s, int *valid, int64_t *bytes, float *scale) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_sq8_info: null store");
    // (a store with pending changes has no current mirror: the next call rebuilds it)
    const bool cur = s->sq8_codes && s->sq8_metric >= 0 && !s->table_dirty && s->sq8_version == s->version;
    if (valid) *valid = cur ? 1 : 0;
    if (bytes) *bytes = s->sq8_codes ? s->sq8_cap_rows * ((int64_t)qk_sq8_nblk(s->d) * 64 + 4) : 0;
    if (scale) *scale = cur ? s->sq8_scale : 0.0f;
    return QK_OK;
}

int qk_store_sq8_drop(qk_store *s) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_sq8_drop: null store");
    QK_HIP(hipSetDevice(s->ctx->device));
    QK_HIP(hipDeviceSynchronize());  // (searches of other contexts may be reading it)
    qk_store_sq8_free(s);
    return QK_OK;
}

}  // extern "C"
