// qk_scan_wide.hip -- the wide-row forms: the scan, the dense step (coarse / flat / nearest list) and the k-means assign for rows
// too wide for a 16-query tile in LDS.
//
// The generic kernels (k_scan, k_dense_ord / k_dense_argmin, k_assign) stage a whole 16-query tile in LDS -- 1 KiB per 16 columns --
// which stops them at d ~ 2500 (less next to large top-k pools).  These siblings keep only the pools in LDS and take the B operand
// of v_mfma_f32_16x16x4_f32 straight from global memory (the prepared queries in fragment order, qk_prep_queries: one float4 per
// lane and 16-column block, served from L2 / MALL), and walk the rows in groups of R row tiles: one B fragment feeds R independent
// accumulator chains, so the query bytes are 1 / R of the row bytes and the R chains cover the MFMA's dependent latency.
//   k_scan_wide<L2, MAXCH, EMIT>  sibling of k_scan in the same pipeline (items / segments of k_group_*, gtau, the pool records
//                                 k_merge reads; EMIT: every key to key_out for k_select_rows_large)
//   k_dense_wide<L2, ARGMIN>      every query against one list: k_dense_ord's key matrix, or k_dense_argmin's packed minimum
//   k_assign_wide<L2>             Lloyd assign (k_assign): rows of x against all centroids, argmin with ties to the lower index
// Every (query, row) chain still runs over the columns 0 .. d-1 in order -- block by block, elements x, y, z, w of each block --
// exactly as in the LDS-staged kernels: same bits.
#include "qk_internal.h"
#include "qk_device.h"
#include "qk_scan_types.h"

#include <algorithm>

constexpr int QK_WIDE_R = 4;   // row tiles per pass over the column blocks (accumulator chains in flight)
constexpr int QK_WIDE_DB = 4;  // 16-column blocks per load step

__device__ __forceinline__ float4 wide_ld_nt(const float4 *p) {
    const f32x4 t = __builtin_nontemporal_load((const f32x4 *)p);
    return make_float4(t[0], t[1], t[2], t[3]);
}

// acc[r] = the 16 x 16 products of row tile r (A operands at a + min(r, nr - 1) * tstride, this lane's float4 of block c at
// + c * 64) with the query tile whose block-c fragment bload(c) returns.  Tiles r >= nr repeat the last one (static loads, in bounds).
template <bool NT, class BLoad>
__device__ __forceinline__ void wide_tiles(f32x4 (&acc)[QK_WIDE_R], const float4 *a, int64_t tstride, int nr, int nblk, BLoad bload) {
    constexpr int R = QK_WIDE_R, DB = QK_WIDE_DB;
    const float4 *ar[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        ar[r] = a + (int64_t)min(r, nr - 1) * tstride;
        acc[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    auto ld = [&](const float4 *p) { return NT ? wide_ld_nt(p) : *p; };
    int c = 0;
    for (; c + DB <= nblk; c += DB) {
        float4 bq[DB], av[R][DB];
#pragma unroll
        for (int b = 0; b < DB; b++) bq[b] = bload(c + b);
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int b = 0; b < DB; b++) av[r][b] = ld(ar[r] + (c + b) * 64);
#pragma unroll
        for (int b = 0; b < DB; b++) {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][b].x, bq[b].x, acc[r], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][b].y, bq[b].y, acc[r], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][b].z, bq[b].z, acc[r], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][b].w, bq[b].w, acc[r], 0, 0, 0);
        }
    }
    for (; c < nblk; c++) {  // (the nblk % DB blocks left: d = 4100 has 257)
        const float4 bq = bload(c);
        float4 av[R];
#pragma unroll
        for (int r = 0; r < R; r++) av[r] = ld(ar[r] + c * 64);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r].x, bq.x, acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r].y, bq.y, acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r].z, bq.z, acc[r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r].w, bq.w, acc[r], 0, 0, 0);
    }
}

// ---- k_scan_wide ---------------------------------------------------------------------------------------------------------------
// One wave per workgroup, LDS = its 16 pools of C entries.  The wave's range of the tile sequence is cut like k_scan's (one wave
// per workgroup, no query sharing, no dynamic tail, no XCD weights); a segment's tiles go through wide_tiles R at a time, then
// each tile's keys take k_scan's candidate path (ballot, pool append, bisection select, gtau refresh / publish), and the segment
// ends with k_scan's compaction and record emission.
template <bool L2, int MAXCH, bool EMIT>
__global__ __launch_bounds__(64) void k_scan_wide(ScanParams P) {
#define QK_SCAN_FILT 0
#include "qk_scan_wide_body.inc"
#undef QK_SCAN_FILT
}
// the filtered sibling (its own kernel, so that no instantiation of k_scan_wide changes): see qk_scan_wide_body.inc
template <bool L2, int MAXCH>
__global__ __launch_bounds__(64) void k_scan_wide_filt(ScanParams P) {
    constexpr bool EMIT = false;
#define QK_SCAN_FILT 1
#include "qk_scan_wide_body.inc"
#undef QK_SCAN_FILT
}
// one filter per query (ScanParams::qmasks / qfilter): see qk_scan_wide_body.inc
template <bool L2, int MAXCH>
__global__ __launch_bounds__(64) void k_scan_wide_filtq(ScanParams P) {
    constexpr bool EMIT = false;
#define QK_SCAN_FILT 2
#include "qk_scan_wide_body.inc"
#undef QK_SCAN_FILT
}

// paged search (qk_after.hip): the filtered body plus the cursor test in the epilogue (see qk_scan_wide_body.inc)
template <bool L2, int MAXCH>
__global__ __launch_bounds__(64) void k_scan_wide_after(ScanParams P) {
    constexpr bool EMIT = false;
#define QK_SCAN_FILT 1
#define QK_SCAN_AFTER
#include "qk_scan_wide_body.inc"
#undef QK_SCAN_AFTER
#undef QK_SCAN_FILT
}

template <bool L2, int MAXCH>
static int launch_scan_wide_a(unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    QK_HIP(hipFuncSetAttribute((const void *)k_scan_wide_after<L2, MAXCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_scan_wide_after<L2, MAXCH>), dim3(grid), dim3(64), lds, st, sp);
    return QK_OK;
}

template <bool L2, int MAXCH>
static int launch_scan_wide_fq(unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    QK_HIP(hipFuncSetAttribute((const void *)k_scan_wide_filtq<L2, MAXCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_scan_wide_filtq<L2, MAXCH>), dim3(grid), dim3(64), lds, st, sp);
    return QK_OK;
}

template <bool L2, int MAXCH>
static int launch_scan_wide_f(unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    QK_HIP(hipFuncSetAttribute((const void *)k_scan_wide_filt<L2, MAXCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_scan_wide_filt<L2, MAXCH>), dim3(grid), dim3(64), lds, st, sp);
    return QK_OK;
}

template <bool L2, int MAXCH, bool EMIT>
static int launch_scan_wide_k(unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    QK_HIP(hipFuncSetAttribute((const void *)k_scan_wide<L2, MAXCH, EMIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_scan_wide<L2, MAXCH, EMIT>), dim3(grid), dim3(64), lds, st, sp);
    return QK_OK;
}
template <bool L2>
static int launch_scan_wide_m(int maxch, unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.mask) {
        if (sp.key_out) QK_FAIL(QK_ERR_UNSUPPORTED, "no filtered wide-row scan kernel for key emission");
        if (sp.qmasks) {  // one filter per query
            if (maxch == 1) return launch_scan_wide_fq<L2, 1>(grid, lds, st, sp);
            if (maxch == 2) return launch_scan_wide_fq<L2, 2>(grid, lds, st, sp);
            if (maxch == 4) return launch_scan_wide_fq<L2, 4>(grid, lds, st, sp);
            return launch_scan_wide_fq<L2, 8>(grid, lds, st, sp);
        }
        if (sp.after_key) {  // paged search
            if (maxch == 1) return launch_scan_wide_a<L2, 1>(grid, lds, st, sp);
            if (maxch == 2) return launch_scan_wide_a<L2, 2>(grid, lds, st, sp);
            if (maxch == 4) return launch_scan_wide_a<L2, 4>(grid, lds, st, sp);
            return launch_scan_wide_a<L2, 8>(grid, lds, st, sp);
        }
        if (maxch == 1) return launch_scan_wide_f<L2, 1>(grid, lds, st, sp);
        if (maxch == 2) return launch_scan_wide_f<L2, 2>(grid, lds, st, sp);
        if (maxch == 4) return launch_scan_wide_f<L2, 4>(grid, lds, st, sp);
        return launch_scan_wide_f<L2, 8>(grid, lds, st, sp);
    }
    if (sp.key_out) return launch_scan_wide_k<L2, 1, true>(grid, lds, st, sp);
    if (maxch == 1) return launch_scan_wide_k<L2, 1, false>(grid, lds, st, sp);
    if (maxch == 2) return launch_scan_wide_k<L2, 2, false>(grid, lds, st, sp);
    if (maxch == 4) return launch_scan_wide_k<L2, 4, false>(grid, lds, st, sp);
    return launch_scan_wide_k<L2, 8, false>(grid, lds, st, sp);
}
int qk_launch_scan_wide(int maxch, unsigned grid, size_t lds, hipStream_t st, const ScanParams &sp) {
    return sp.metric == QK_METRIC_L2 ? launch_scan_wide_m<true>(maxch, grid, lds, st, sp) : launch_scan_wide_m<false>(maxch, grid, lds, st, sp);
}

// ---- k_dense_wide --------------------------------------------------------------------------------------------------------------
// Workgroup = 16 queries (blockIdx.x) x a chunk of row tiles (blockIdx.y) cut four ways between its waves: k_dense_ord /
// k_dense_argmin with NQ = 1.  !ARGMIN: the key of every (query, row) goes to D[q][row] (0xFFFFFFFF past the list's end).
// ARGMIN: the minimum of (key << 32 | id) per query goes into best64[q] with atomicMin (the caller checked that ids fit 32 bits).
template <bool L2, bool ARGMIN>
__global__ __launch_bounds__(256) void k_dense_wide(QkDenseWideParams P) {
    __shared__ unsigned long long red[4][16];
    constexpr int R = QK_WIDE_R;
    constexpr bool l2 = L2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int nblk = P.nblk;
    const int64_t q = (int64_t)blockIdx.x * 16 + j;
    const int64_t qsafe = q < P.Q ? q : P.Q - 1;
    const float xnj = (l2 && q < P.Q) ? P.xn[q] : 0.0f;
    const float4 *qsrc = P.xq4 + qsafe * nblk * 4 + g;
    auto bload = [&](int c) { return qsrc[c * 4]; };
    unsigned long long best = ~0ull;
    const int ntile_all = (P.nrows + 15) >> 4;
    const int wg_t0 = blockIdx.y * P.tiles_per_wg;
    const int wg_t1 = min(ntile_all, wg_t0 + P.tiles_per_wg);
    const int tpw = (wg_t1 - wg_t0 + 3) >> 2;
    const int t0 = wg_t0 + wave * tpw, t1 = min(wg_t1, t0 + tpw);
    for (int tb = t0; tb < t1; tb += R) {
        const int nr = min(R, t1 - tb);
        const int64_t tile_abs = (P.row_off >> 4) + tb;
        f32x4 acc[R];
        // (every query block reads the whole list: plain loads, it stays in L2 / MALL)
        wide_tiles<false>(acc, P.vecs + tile_abs * nblk * 64 + lane, (int64_t)nblk * 64, nr, nblk, bload);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r >= nr) break;
            const int tile = tb + r;
            const int row0 = (tile << 4) + 4 * g;
            const float4 yn = l2 ? ((const float4 *)(P.norms + ((tile_abs + r) << 4)))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float yv[4] = {yn.x, yn.y, yn.z, yn.w};
            uint32_t kv[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) kv[reg] = l2 ? ord_from_l2(l2_expanded(xnj, yv[reg], acc[r][reg])) : ord_from_ip(acc[r][reg]);
            if (ARGMIN) {
                const longlong2 ia = ((const longlong2 *)(P.ids + ((int64_t)tile << 4)))[2 * g];
                const longlong2 ib = ((const longlong2 *)(P.ids + ((int64_t)tile << 4)))[2 * g + 1];
                const uint32_t iv[4] = {(uint32_t)ia.x, (uint32_t)ia.y, (uint32_t)ib.x, (uint32_t)ib.y};
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const unsigned long long c = ((unsigned long long)kv[reg] << 32) | iv[reg];
                    if (row0 + reg < P.nrows && c < best) best = c;
                }
            } else {
                uint4 o;
                o.x = row0 + 0 < P.nrows ? kv[0] : 0xFFFFFFFFu;
                o.y = row0 + 1 < P.nrows ? kv[1] : 0xFFFFFFFFu;
                o.z = row0 + 2 < P.nrows ? kv[2] : 0xFFFFFFFFu;
                o.w = row0 + 3 < P.nrows ? kv[3] : 0xFFFFFFFFu;
                if (q < P.Q) *(uint4 *)(P.D + q * P.ld + row0) = o;
            }
        }
    }
    if (!ARGMIN) return;
    unsigned long long o = __shfl_xor(best, 16);
    best = o < best ? o : best;
    o = __shfl_xor(best, 32);
    best = o < best ? o : best;
    if (g == 0) red[wave][j] = best;
    __syncthreads();
    if (tid < 16) {
        unsigned long long v = red[0][tid];
#pragma unroll
        for (int w = 1; w < 4; w++) v = red[w][tid] < v ? red[w][tid] : v;
        const int64_t qq = (int64_t)blockIdx.x * 16 + tid;
        if (qq < P.Q && (uint32_t)(v >> 32) != 0xFFFFFFFFu) atomicMin(&P.best64[qq], v);  // (all ones: a NaN value, no candidate)
    }
}

int qk_launch_dense_wide(hipStream_t st, const QkDenseWideParams &p, bool argmin, int metric, int num_cus) {
    const int64_t qgroups = (p.Q + 15) / 16;
    const int ntile = (p.nrows + 15) / 16;
    if (qgroups <= 0 || ntile <= 0) return QK_OK;
    // two workgroups per CU, whole groups of R tiles per wave
    const int64_t want_chunks = std::max<int64_t>(1, ((int64_t)2 * num_cus + qgroups - 1) / qgroups);
    int tiles_per_wg = (int)std::max<int64_t>(4 * QK_WIDE_R, (ntile + want_chunks - 1) / want_chunks);
    tiles_per_wg = qk_round_up(tiles_per_wg, 4 * QK_WIDE_R);
    QkDenseWideParams dp = p;
    dp.tiles_per_wg = tiles_per_wg;
    const dim3 grid((unsigned)qgroups, (unsigned)std::max(1, (ntile + tiles_per_wg - 1) / tiles_per_wg));
    const bool l2 = metric == QK_METRIC_L2;
    if (argmin) {
        if (l2) hipLaunchKernelGGL((k_dense_wide<true, true>), grid, dim3(256), 0, st, dp);
        else hipLaunchKernelGGL((k_dense_wide<false, true>), grid, dim3(256), 0, st, dp);
    } else {
        if (l2) hipLaunchKernelGGL((k_dense_wide<true, false>), grid, dim3(256), 0, st, dp);
        else hipLaunchKernelGGL((k_dense_wide<false, false>), grid, dim3(256), 0, st, dp);
    }
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// ---- k_assign_wide -------------------------------------------------------------------------------------------------------------
// Workgroup = 16 rows of x against every centroid tile (cut four ways between the waves): k_assign with NQ = 1.  The B fragment of
// block c is read from the row-major rows (columns 16c + g + {0, 4, 8, 12}, zero past d), the squared norm is k_assign's fmaf chain,
// and the (key, index) minimum keeps the lower index on a tie.
template <bool L2>
__global__ __launch_bounds__(256) void k_assign_wide(QkAssignWideParams P) {
    __shared__ float xn_s[16];
    __shared__ uint32_t red_ord[4][16];
    __shared__ int red_idx[4][16];
    constexpr int R = QK_WIDE_R;
    constexpr bool l2 = L2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int nblk = P.nblk, d = P.d;
    const int64_t row_base = (int64_t)blockIdx.x * 16;
    if (tid < 16) {
        const int64_t row = row_base + tid;
        float acc = 0.0f;
        if (row < P.n && l2) {
            const float *s = P.x + row * d;
            for (int c = 0; c < d; c++) acc = __fmaf_rn(s[c], s[c], acc);
        }
        xn_s[tid] = acc;
    }
    __syncthreads();
    const float xnj = xn_s[j];
    const int64_t row = row_base + j;
    const bool row_ok = row < P.n;
    const float *xs = P.x + (row_ok ? row : 0) * d;
    auto bload = [&](int c) {
        const int col = 16 * c + g;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row_ok) {
            v.x = col < d ? xs[col] : 0.0f;
            v.y = col + 4 < d ? xs[col + 4] : 0.0f;
            v.z = col + 8 < d ? xs[col + 8] : 0.0f;
            v.w = col + 12 < d ? xs[col + 12] : 0.0f;
        }
        return v;
    };
    uint32_t best_ord = 0xFFFFFFFFu;
    int best_idx = 0x7FFFFFFF;
    const int mt = (P.m + 15) >> 4;
    const int tpw = (mt + 3) >> 2;
    const int t0 = wave * tpw, t1 = min(mt, t0 + tpw);
    for (int tb = t0; tb < t1; tb += R) {
        const int nr = min(R, t1 - tb);
        f32x4 acc[R];
        wide_tiles<false>(acc, P.cvecs + (int64_t)tb * nblk * 64 + lane, (int64_t)nblk * 64, nr, nblk, bload);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r >= nr) break;
            const float4 yn = l2 ? ((const float4 *)(P.cnorms + ((int64_t)(tb + r) << 4)))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float yv[4] = {yn.x, yn.y, yn.z, yn.w};
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int idx = ((tb + r) << 4) + 4 * g + reg;
                const uint32_t o = l2 ? ord_bits_l2(l2_expanded(xnj, yv[reg], acc[r][reg])) : ord_bits_ip(acc[r][reg]);  // (k-means' keys)
                if (idx < P.m && o < best_ord) {
                    best_ord = o;
                    best_idx = idx;
                }
            }
        }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const uint32_t oo = __shfl_xor(best_ord, off);
        const int oi = __shfl_xor(best_idx, off);
        if (oo < best_ord || (oo == best_ord && oi < best_idx)) {
            best_ord = oo;
            best_idx = oi;
        }
    }
    if (g == 0) {
        red_ord[wave][j] = best_ord;
        red_idx[wave][j] = best_idx;
    }
    __syncthreads();
    if (tid < 16) {
        uint32_t bo = red_ord[0][tid];
        int bi = red_idx[0][tid];
        for (int w = 1; w < 4; w++) {
            const uint32_t oo = red_ord[w][tid];
            const int oi = red_idx[w][tid];
            if (oo < bo || (oo == bo && oi < bi)) {
                bo = oo;
                bi = oi;
            }
        }
        const int64_t rr = row_base + tid;
        if (rr < P.n) {
            P.assign[rr] = bi == 0x7FFFFFFF ? -1 : bi;
            if (P.val) P.val[rr] = l2 ? __uint_as_float(bo) : ip_from_ord(bo);
        }
    }
}

int qk_launch_assign_wide(hipStream_t st, const QkAssignWideParams &p, int metric) {
    if (p.n <= 0) return QK_OK;
    const dim3 grid((unsigned)((p.n + 15) / 16));
    if (metric == QK_METRIC_L2) hipLaunchKernelGGL((k_assign_wide<true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_assign_wide<false>), grid, dim3(256), 0, st, p);
    QK_HIP(hipGetLastError());
    return QK_OK;
}
