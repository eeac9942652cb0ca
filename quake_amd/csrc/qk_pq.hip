// qk_pq.hip -- product-quantized search (include/quake_hip.h, "product-quantized search"): product quantization with
// oversampling and rescoring.  The d columns are cut into M sub-spaces of dsub = d / M columns, each with a codebook of 256 float32
// codewords; a row is mirrored as M bytes, the index of the nearest codeword per sub-space.  Per query a table T[m][c] of the
// query's distance to every codeword is quantized to uint16 entries u[m][c] whose row sums stay under 8192; the fetch_k rows of
// its probed lists with the smallest key h = sum_m u[m][code_m] -- ties by arena row -- are re-scored on the float32 rows, the k
// best under (exact key, id) returned.
// The mirror: code row r is arena row r.  A row's codes are 16-byte words of 16 sub-quantizers (byte b of word w is sub-quantizer
// 16 w + b; bytes from M on are 0); the 16 words of a tile's rows lie side by side (256 B), the words of a tile one after the other:
//     uint4 index (tile nw + w) 16 + r,   nw = ceil(M / 16)
// One enqueue on the context's stream, no host wait inside -- except the one-off build of the mirror:
//   k_pq_norms         n[m][c] = dot(w, w) of every codeword, when codebooks are set
//   k_pq_encode        arena tiles -> code bytes: a k-means assign in miniature on v_mfma_f32_16x16x4_f32, the sub-space's codebook
//                      in LDS, the non-finite check in the same pass
//   k_pq_lut           T for 16 queries x 16 codewords per MFMA -> float32 [Q][M][256] in the call's workspace
//   (coarse: the shipped one)
//   k_pq_select        one workgroup per query, no global atomics: the prologue (lo / hi / R / delta, the uint16 table into LDS, the
//                      query's lists ordered by arena offset), pass A (keys by byte-indexed LDS gathers into a histogram of 8192
//                      bins), the cut key by a prefix sum, pass B (the rows under the cut and the first ties, compacted in walk order)
//   (k_funnel_finish / k_sq8_deep_finish: the exact finish, unchanged)
//   k_pq_gather        training only: a sample's sub-vectors [n][dsub] from the arena, for the library's own k-means
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int PQ_U = 4;           // rows per lane and step: their code loads are in flight together
constexpr int PQ_CW_STRIDE = 272; // floats between two columns of the staged codebook: the four k-slices of a B operand fall into
                                  // different 16-bank groups
constexpr int PQ_BINS = QK_PQ_KEY_BINS;

// the float of arena row (tile, r), column col: block col / 16, lane group col % 4, element (col % 16) / 4 of that lane's float4
__device__ __forceinline__ float pq_arena_at(const float *__restrict__ vecs, int64_t tile, int nblk, int r, int col) {
    return vecs[(((tile * nblk + (col >> 4)) * 64) + (col & 3) * 16 + r) * 4 + ((col & 15) >> 2)];
}

// ---- codeword norms ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pq_norms(const float *__restrict__ cb, int dsub, float *__restrict__ cbn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (m, c): the grid is M blocks of 256
    const float *w = cb + i * dsub;
    float acc = 0.0f;
    for (int j = 0; j < dsub; j++) acc = fmaf(w[j], w[j], acc);
    cbn[i] = acc;
}

// (e is NaN, e, c): does (e, c) come before (be, bc)?
__device__ __forceinline__ bool pq_before(float e, int c, float be, int bc) {
    const bool en = e != e, bn = be != be;
    if (en != bn) return bn;
    if (!en && e != be) return e < be;
    return c < bc;
}

// ---- arena tiles -> code bytes ------------------------------------------------------------------------------------------------------
// blockIdx.x = list, blockIdx.y = slice of its tiles, blockIdx.z = sub-quantizer m; a wave per tile.  The codebook of m is staged once
// per workgroup as B operands: s_w[(4 j + g) PQ_CW_STRIDE + c] = w[m][c][4 j + g], 0 from column dsub on; s_n[c] = n[m][c].  Lane
// (g, r) gathers the A operand of step j -- row r, column m dsub + 4 j + g -- from the arena's 16-column blocks, one float per
// step (a sub-space need not begin or end on a float4 of the arena), zero-padded behind dsub.  16 codeword tiles: acc[reg] of lane
// (g, j) = dot(row 4 g + reg, codeword 16 ct + j); e = fmaf(-2, dot, n); a running (e, c) minimum per reg -- c ascends with ct, so
// within a lane a later codeword replaces only if it comes strictly before --, then four shuffles reduce the 16 lanes of a group under
// (e is NaN, e, c).  Lane (g, j < 4) stores the byte of row 4 g + j.  Rows behind the list's size keep the 0 of the cleared mirror.
// A value of a live row that is not finite: atomicMin of the list number into *bad.
__global__ __launch_bounds__(256) void k_pq_encode(const float *__restrict__ vecs, int nblk, int M, int dsub, const int64_t *__restrict__ pt_off,
                                                   const int32_t *__restrict__ pt_size, const float *__restrict__ cb, const float *__restrict__ cbn,
                                                   uint8_t *__restrict__ codes, int32_t *__restrict__ bad) {
    extern __shared__ float pe_lds[];
    const int size = pt_size[blockIdx.x];
    if (size <= 0) return;
    const int m = blockIdx.z, nst = (dsub + 3) >> 2, nw = (M + 15) >> 4;
    float *s_w = pe_lds, *s_n = pe_lds + (size_t)nst * 4 * PQ_CW_STRIDE;
    for (int i = threadIdx.x; i < nst * 4 * 256; i += 256) {
        const int c = i & 255, col = i >> 8;
        s_w[col * PQ_CW_STRIDE + c] = col < dsub ? cb[((int64_t)m * 256 + c) * dsub + col] : 0.0f;
    }
    s_n[threadIdx.x] = cbn[m * 256 + threadIdx.x];
    __syncthreads();
    const int64_t tile0 = pt_off[blockIdx.x] >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int ntl = (size + 15) >> 4;
    bool finite = true;
    for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
        const int64_t tile = tile0 + t;
        const bool live = t * 16 + r < size;
        float a[QK_PQ_MAX_DSUB / 4];
#pragma unroll
        for (int j = 0; j < QK_PQ_MAX_DSUB / 4; j++) {
            a[j] = 0.0f;
            if (j < nst && live && 4 * j + g < dsub) {
                a[j] = pq_arena_at(vecs, tile, nblk, r, m * dsub + 4 * j + g);
                finite = finite && fabsf(a[j]) <= 3.402823466e38f;  // (false for NaN and +-inf)
            }
        }
        float be[4];
        int bc[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            be[reg] = __uint_as_float(0x7FC00000u);  // (NaN, c = 0: what a sub-space of NaN keys ends with)
            bc[reg] = 0;
        }
        for (int ct = 0; ct < 16; ct++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float *bw = s_w + g * PQ_CW_STRIDE + 16 * ct + r;
#pragma unroll
            for (int j = 0; j < QK_PQ_MAX_DSUB / 4; j++)
                if (j < nst) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bw[j * 4 * PQ_CW_STRIDE], acc, 0, 0, 0);
            const int c = 16 * ct + r;
            const float nc = s_n[c];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const float e = fmaf(-2.0f, acc[reg], nc);
                if (e < be[reg] || (be[reg] != be[reg] && e == e)) {
                    be[reg] = e;
                    bc[reg] = c;
                }
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float oe = __shfl_xor(be[reg], o);
                const int oc = __shfl_xor(bc[reg], o);
                if (pq_before(oe, oc, be[reg], bc[reg])) {
                    be[reg] = oe;
                    bc[reg] = oc;
                }
            }
        const int row = 4 * g + r;  // (for r < 4)
        const int code = r == 0 ? bc[0] : r == 1 ? bc[1] : r == 2 ? bc[2] : bc[3];
        if (r < 4 && t * 16 + row < size) codes[((tile * nw + (m >> 4)) * 16 + row) * 16 + (m & 15)] = (uint8_t)code;
    }
    if (__ballot(!finite) != 0ull && lane == 0) atomicMin(bad, (int32_t)blockIdx.x);
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------------
// blockIdx.x = tile of 16 queries, blockIdx.y = sub-quantizer m, wave w takes codeword tiles 4 w .. 4 w + 3.  Both operands come from
// global memory: A = the queries' sub-vectors (lane (g, r): query 16 qt + r, column m dsub + 4 j + g), B = the codewords (lane (g, c):
// codeword 16 ct + c, column 4 j + g), zero-padded behind dsub -- a codebook is read once per 16 queries.  acc[reg] of lane (g, j) =
// dot(query 4 g + reg, codeword 16 ct + j): T = fmaf(-2, dot, n) (L2), -dot (IP)
template <bool L2>
__global__ __launch_bounds__(256) void k_pq_lut(const float *__restrict__ x, int64_t Q, int d, int M, int dsub, const float *__restrict__ cb,
                                                const float *__restrict__ cbn, float *__restrict__ T) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int m = blockIdx.y, nst = (dsub + 3) >> 2;
    const int64_t q0 = (int64_t)blockIdx.x * 16, qa = q0 + r;
    float a[QK_PQ_MAX_DSUB / 4];
#pragma unroll
    for (int j = 0; j < QK_PQ_MAX_DSUB / 4; j++) a[j] = (j < nst && qa < Q && 4 * j + g < dsub) ? x[qa * d + m * dsub + 4 * j + g] : 0.0f;
    for (int ct = 4 * wv; ct < 4 * wv + 4; ct++) {
        const int cB = 16 * ct + r;
        const float *w = cb + ((int64_t)m * 256 + cB) * dsub;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < QK_PQ_MAX_DSUB / 4; j++)
            if (j < nst) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], 4 * j + g < dsub ? w[4 * j + g] : 0.0f, acc, 0, 0, 0);
        const float nc = L2 ? cbn[m * 256 + cB] : 0.0f;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int64_t q = q0 + 4 * g + reg;
            if (q < Q) T[(q * M + m) * 256 + cB] = L2 ? fmaf(-2.0f, acc[reg], nc) : -acc[reg];
        }
    }
}

// ---- the selection ------------------------------------------------------------------------------------------------------------------
struct PqSelectParams {
    const uint4 *codes;
    const int64_t *pt_off;
    const int32_t *pt_size;
    int npids;
    const int64_t *pids;  // [Q][P], or nullptr: list pi is list number pi
    int P, M, nw;
    const float *T;       // [Q][M][256]
    int C;                // fetch_k
    int64_t *cand;        // [Q][C] arena rows in ascending order, -1 behind
    uint2 *stat;          // [Q] {probed rows, lists walked}, or nullptr
};

// dynamic LDS of k_pq_select: the table (16 nw rows of 256 uint16: rows from M on are 0, so the padding bytes of a code word add
// nothing) | histogram | lo, hi [128 each] | list table (offset 8, size 4 bytes per list)
inline size_t pq_lds_bytes(int M, int P) { return (size_t)qk_pq_nw(M) * 16 * 512 + (size_t)PQ_BINS * 4 + 2 * QK_PQ_MAX_M * 4 + (size_t)P * 12; }

// exclusive prefix sum of v over the workgroup's 256 threads in thread order; total = the sum.  s_w [4]
__device__ __forceinline__ uint32_t pq_scan_excl(uint32_t v, uint32_t *s_w, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();  // (the last call's readers of s_w are done)
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t t = s_w[w];
        if (w < wave) base += t;
        tot += t;
    }
    total = tot;
    return base + x - v;
}

// the keys of rows i0 + 256 u, u < PQ_U, of the list at arena row `off` (rows behind its size: the last row's key, unused): per code
// word one 16-byte load per row -- the PQ_U loads of a word are independent, they are in flight together --, then 16 byte-indexed
// uint16 reads of the table per row
__device__ __forceinline__ void pq_keys(const uint4 *__restrict__ codes, int nw, const uint16_t *s_u, int64_t off, int size, int i0, uint32_t *h) {
    const uint4 *src[PQ_U];
#pragma unroll
    for (int u = 0; u < PQ_U; u++) {
        const int64_t row = off + min(i0 + 256 * u, size - 1);
        src[u] = codes + (row >> 4) * nw * 16 + (row & 15);
        h[u] = 0u;
    }
    for (int w = 0; w < nw; w++) {
        uint4 v[PQ_U];
#pragma unroll
        for (int u = 0; u < PQ_U; u++) v[u] = src[u][w * 16];
        const uint16_t *tw = s_u + w * 16 * 256;
#pragma unroll
        for (int u = 0; u < PQ_U; u++) {
            const uint32_t dw[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int b = 0; b < 16; b++) h[u] += tw[b * 256 + ((dw[b >> 2] >> (8 * (b & 3))) & 255u)];
        }
    }
}

// blockIdx.x = query, 256 threads.
//   0. the table: wave w reduces lo / hi of T[m][.] for m = w, w + 4, .. (four entries per lane, shuffles, no barrier) and notes
//      whether every entry is finite; every thread sums R over m ascending; the waves quantize their rows into s_u.
//   1. - 4. k_bin_select's steps word for word with the key above: the lists rank-sorted by (offset, entry), pass A into the
//      histogram, the cut by a prefix sum, pass B with ordered ballot compaction: taken rows land in cand[q] in ascending arena rows.
__global__ __launch_bounds__(256) void k_pq_select(PqSelectParams B) {
    extern __shared__ uint4 ps_lds[];
    __shared__ uint32_t s_w[4], s_cut[2], s_bad;
    __shared__ uint2 s_cnt[2][4 * PQ_U];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int P = B.P, M = B.M, nw = B.nw, C = B.C;
    uint16_t *s_u = (uint16_t *)ps_lds;
    uint32_t *s_hist = (uint32_t *)(s_u + (size_t)nw * 16 * 256);
    float *s_lo = (float *)(s_hist + PQ_BINS);
    float *s_hi = s_lo + QK_PQ_MAX_M;
    int64_t *s_off = (int64_t *)(s_hi + QK_PQ_MAX_M);
    int32_t *s_size = (int32_t *)(s_off + P);
    // ---- 0. the table
    const float *Tq = B.T + q * M * 256;
    if (tid == 0) s_bad = 0u;
    for (int i = tid; i < PQ_BINS; i += 256) s_hist[i] = 0u;
    for (int i = M * 256 + tid; i < nw * 16 * 256; i += 256) s_u[i] = 0;
    __syncthreads();
    {
        bool ok = true;
        for (int m = wave; m < M; m += 4) {
            float lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float t = Tq[m * 256 + lane + 64 * i];
                ok = ok && fabsf(t) <= 3.402823466e38f;
                lo = fminf(lo, t);
                hi = fmaxf(hi, t);
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                lo = fminf(lo, __shfl_xor(lo, o));
                hi = fmaxf(hi, __shfl_xor(hi, o));
            }
            if (lane == 0) {
                s_lo[m] = lo;
                s_hi[m] = hi;
            }
        }
        if (__ballot(!ok) != 0ull && lane == 0) s_bad = 1u;  // (every writer writes 1)
    }
    __syncthreads();
    {
        float R = 0.0f;
        for (int m = 0; m < M; m++) R += s_hi[m] - s_lo[m];
        const bool zero = s_bad != 0u || !(R > 0.0f) || !(R <= 3.402823466e38f);
        const float delta = R / 8000.0f;
        for (int m = wave; m < M; m += 4) {
            const float lo = s_lo[m];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int c = lane + 64 * i;
                const float t = Tq[m * 256 + c];
                s_u[m * 256 + c] = zero ? (uint16_t)0 : (uint16_t)rintf((t - lo) / delta);
            }
        }
    }
    // ---- 1. the lists in arena order
    constexpr int LPT = QK_PQ_MAX_NPROBE / 256;
    constexpr int64_t LAST = 0x7FFFFFFFFFFFFFFFll;
    int64_t off[LPT];
    int32_t sz[LPT];
#pragma unroll
    for (int j = 0; j < LPT; j++) {
        const int pi = tid + 256 * j;
        off[j] = LAST;
        sz[j] = 0;
        if (pi < P) {
            const int64_t p = B.pids ? B.pids[q * P + pi] : pi;
            if (p >= 0 && p < B.npids) {
                const int32_t s = B.pt_size[p];
                if (s > 0) {
                    off[j] = B.pt_off[p];
                    sz[j] = s;
                }
            }
            s_off[pi] = off[j];
        }
    }
    __syncthreads();
    int rank[LPT];
#pragma unroll
    for (int j = 0; j < LPT; j++) {
        const int pi = tid + 256 * j;
        rank[j] = 0;
        if (pi < P)
            for (int jj = 0; jj < P; jj++) {
                const int64_t o = s_off[jj];
                rank[j] += (o < off[j] || (o == off[j] && jj < pi)) ? 1 : 0;
            }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LPT; j++)
        if (tid + 256 * j < P) {
            s_off[rank[j]] = off[j];
            s_size[rank[j]] = sz[j];
        }
    __syncthreads();
    uint32_t mine = 0, live = 0;
#pragma unroll
    for (int j = 0; j < LPT; j++) {
        const int e = LPT * tid + j;
        if (e < P) {
            mine += (uint32_t)s_size[e];
            live += s_size[e] > 0 ? 1u : 0u;
        }
    }
    uint32_t total, nlists;
    (void)pq_scan_excl(mine, s_w, total);
    (void)pq_scan_excl(live, s_w, nlists);
    // ---- 2. pass A
    for (int li = 0; li < (int)nlists; li++) {
        const int size = s_size[li];
        const int64_t loff = s_off[li];
        for (int i0 = tid; i0 < size; i0 += 256 * PQ_U) {
            uint32_t h[PQ_U];
            pq_keys(B.codes, nw, s_u, loff, size, i0, h);
#pragma unroll
            for (int u = 0; u < PQ_U; u++)
                if (i0 + 256 * u < size) atomicAdd(&s_hist[min(h[u], (uint32_t)PQ_BINS - 1u)], 1u);  // (h < 8192 by construction)
        }
    }
    // ---- 3. the cut
    if (tid == 0) {
        s_cut[0] = (uint32_t)PQ_BINS;  // (no key reaches it: every row lies under the cut)
        s_cut[1] = total;
    }
    __syncthreads();
    {
        constexpr int chunk = PQ_BINS / 256;
        const int b0 = tid * chunk;
        uint32_t sum = 0;
        for (int b = b0; b < b0 + chunk; b++) sum += s_hist[b];
        uint32_t tot;
        const uint32_t ex = pq_scan_excl(sum, s_w, tot);
        if (ex < (uint32_t)C && (uint32_t)C <= ex + sum) {  // (exactly one thread, where the probed rows are at least fetch_k)
            uint32_t c = ex;
            int b = b0;
            while (b < b0 + chunk - 1 && c + s_hist[b] < (uint32_t)C) c += s_hist[b++];
            s_cut[0] = (uint32_t)b;
            s_cut[1] = c;
        }
    }
    __syncthreads();
    const uint32_t cut = s_cut[0];
    const uint32_t target = min(total, (uint32_t)C);
    const uint32_t need = target - min(s_cut[1], target);  // (no cut: 0)
    // ---- 4. pass B
    int64_t *cand = B.cand + q * C;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run_t = 0, run_e = 0;  // rows taken / ties seen so far: the same in every thread
    int par = 0;
    for (int li = 0; li < (int)nlists && run_t < target; li++) {
        const int size = s_size[li];
        const int64_t loff = s_off[li];
        for (int s0 = 0; s0 < size && run_t < target; s0 += 256 * PQ_U) {
            const int i0 = s0 + tid;
            uint32_t h[PQ_U];
            pq_keys(B.codes, nw, s_u, loff, size, i0, h);
            unsigned long long bl[PQ_U], bt[PQ_U];
#pragma unroll
            for (int u = 0; u < PQ_U; u++) {
                const bool valid = i0 + 256 * u < size;
                const uint32_t hh = min(h[u], (uint32_t)PQ_BINS - 1u);
                bl[u] = __ballot(valid && hh < cut);
                bt[u] = __ballot(valid && hh == cut);
                if (lane == 0) s_cnt[par][4 * u + wave] = make_uint2((uint32_t)__popcll(bl[u]), (uint32_t)__popcll(bt[u]));
            }
            __syncthreads();
            uint32_t base_t[PQ_U], base_e[PQ_U];
#pragma unroll
            for (int e = 0; e < 4 * PQ_U; e++) {
                const uint2 c = s_cnt[par][e];
                if ((e & 3) == wave) {
                    base_t[e >> 2] = run_t;
                    base_e[e >> 2] = run_e;
                }
                run_t += c.x + min(c.y, need - min(run_e, need));
                run_e += c.y;
            }
            par ^= 1;
#pragma unroll
            for (int u = 0; u < PQ_U; u++) {
                const uint32_t left = need - min(base_e[u], need);  // ties this wave's ballot may still take
                const uint32_t lb = (uint32_t)__popcll(bl[u] & below), tb = (uint32_t)__popcll(bt[u] & below);
                const bool less = (bl[u] >> lane) & 1ull, tie = (bt[u] >> lane) & 1ull;
                const uint32_t slot = base_t[u] + lb + min(tb, left);
                if ((less || (tie && tb < left)) && slot < (uint32_t)C) cand[slot] = loff + i0 + 256 * u;
            }
        }
    }
    for (uint32_t i = target + tid; i < (uint32_t)C; i += 256) cand[i] = -1;
    if (B.stat && tid == 0) B.stat[q] = make_uint2(total, nlists);
}

// ---- training: the sample's sub-vectors ----------------------------------------------------------------------------------------------
// out[i][j] = column m dsub + j of arena row rows[i]
__global__ __launch_bounds__(256) void k_pq_gather(const float *__restrict__ vecs, int nblk, const int64_t *__restrict__ rows, int64_t n, int m, int dsub,
                                                   float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * dsub) return;
    const int64_t row = rows[i / dsub];
    out[i] = pq_arena_at(vecs, row >> 4, nblk, (int)(row & 15), m * dsub + (int)(i % dsub));
}

// M against d: the definition's limits
int pq_check_m(const char *who, int d, int M) {
    if (M < 1) QK_FAIL(QK_ERR_INVALID, "%s: M=%d must be at least 1", who, M);
    if (M > QK_PQ_MAX_M) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: M=%d exceeds QK_PQ_MAX_M=%d", who, M, QK_PQ_MAX_M);
    if (d % M != 0) QK_FAIL(QK_ERR_INVALID, "%s: M=%d does not divide d=%d", who, M, d);
    if (d / M > QK_PQ_MAX_DSUB) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d / M = %d exceeds QK_PQ_MAX_DSUB=%d", who, d / M, QK_PQ_MAX_DSUB);
    return QK_OK;
}

// device codebooks [M][256][d / M] become the store's: the norms are computed, the codes are invalid.  Takes ownership of cb
int pq_adopt(qk_store *s, int M, float *cb) {
    float *cbn = nullptr;
    int32_t *bad = nullptr;
    if (hipMalloc((void **)&cbn, (size_t)M * 256 * 4) != hipSuccess || hipMalloc((void **)&bad, 4) != hipSuccess) {
        (void)hipGetLastError();
        if (cbn) hipFree(cbn);
        hipFree(cb);
        QK_FAIL(QK_ERR_OOM, "product-quantized search: no device memory for the codebooks");
    }
    hipStream_t st = s->ctx->stream;
    hipLaunchKernelGGL(k_pq_norms, dim3((unsigned)M), dim3(256), 0, st, (const float *)cb, s->d / M, cbn);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {  // (the norms may be anything: the store keeps what it had)
        hipFree(cbn);
        hipFree(bad);
        hipFree(cb);
        QK_HIP(e);
    }
    qk_store_pq_free(s, true);  // (hipFree waits for the device: an earlier call may still read the old codebooks)
    s->pq_M = M;
    s->pq_cb = cb;
    s->pq_cbn = cbn;
    s->pq_bad = bad;
    return QK_OK;
}

// the body of both entry points: parent == nullptr && pids == nullptr -> every list
int qk_pq_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe, int k,
              int fetch_k, int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    const int d = s->d;
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (fetch_k < k) QK_FAIL(QK_ERR_INVALID, "%s: fetch_k=%d must be at least k=%d", who, fetch_k, k);
    if (Q < 0 || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d", who, k, QK_MAX_K);
    if (fetch_k > QK_PQ_MAX_FETCH) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_PQ_MAX_FETCH=%d", who, fetch_k, QK_PQ_MAX_FETCH);
    if (d > QK_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_MAX_D=%d", who, d, QK_MAX_D);
    if (!parent && !pids && s->nlist == 1)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a flat index without lists of its own takes the dense path, which has no PQ code form", who);
    if (s->pq_M == 0) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: the store has no codebooks: train or set codebooks first", who);
    // lists per query: the coarse step's min(nprobe, parent rows), the pids row, or every list of the store
    const int64_t Pq = parent ? std::max<int64_t>(std::min<int64_t>(nprobe, parent->ntotal), 1) : pids ? P : (int64_t)s->parts.size();
    if (Pq > QK_PQ_MAX_NPROBE) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: %lld lists per query exceed QK_PQ_MAX_NPROBE=%d", who, (long long)Pq, QK_PQ_MAX_NPROBE);
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
    const int C = fetch_k, nblk = s->nblk, M = s->pq_M, dsub = d / M, nw = qk_pq_nw(M);
    // ---- the mirror and the call's buffer: what can refuse or fail for want of memory comes first -----------------------------------
    QK_TRY(qk_store_sync_table(s));
    const int64_t rows_ub = Pq * std::max<int64_t>(s->max_size, 0);  // (walk positions and bin counts are 32-bit)
    if (rows_ub >= ((int64_t)1 << 32)) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a query could probe %lld rows, 2^32 or more", who, (long long)rows_ub);
    QK_TRY(qk_store_pq_mirror(ctx, s));
    const size_t b_t = qk_al256((size_t)Q * M * 256 * 4), b_c = qk_al256((size_t)Q * C * 8), b_s = qk_al256((size_t)Q * 8);
    QK_TRY(qk_fn_reserve(ctx, b_t + b_c + b_s));
    float *T = (float *)ctx->fn_buf;
    int64_t *cand = (int64_t *)(ctx->fn_buf + b_t);
    uint2 *stat = (uint2 *)(ctx->fn_buf + b_t + b_c);
    // ---- staging, full query preparation, coarse (the unfiltered qk_search's, on the float32 queries) -------------------------------
    const size_t b_oi = qk_al256((size_t)Q * k * 8), b_od = qk_al256((size_t)Q * k * 4);
    qk_scan_args sa;
    char *stage = nullptr;
    bool have_coarse = false;
    QK_TRY(qk_emit_front_end(ctx, parent, s, x, Q, pids, P, nprobe, metric, mem, b_oi + b_od, timing != nullptr, &sa, &stage, &have_coarse));
    int64_t *d_ids = host ? (int64_t *)stage : out_ids;
    float *d_dist = host ? (out_dist ? (float *)(stage + b_oi) : nullptr) : out_dist;
    const bool tm = ctx->timing && timing;
    if (tm) QK_HIP(hipEventRecord(ctx->ev[4], st));
    const dim3 lg((unsigned)((Q + 15) / 16), (unsigned)M);
    if (l2)
        hipLaunchKernelGGL(k_pq_lut<true>, lg, dim3(256), 0, st, sa.x, Q, d, M, dsub, (const float *)s->pq_cb, (const float *)s->pq_cbn, T);
    else
        hipLaunchKernelGGL(k_pq_lut<false>, lg, dim3(256), 0, st, sa.x, Q, d, M, dsub, (const float *)s->pq_cb, (const float *)s->pq_cbn, T);
    QK_HIP(hipGetLastError());
    // ---- the candidates ---------------------------------------------------------------------------------------------------------------
    PqSelectParams pp;
    pp.codes = (const uint4 *)s->pq_codes;
    pp.pt_off = (const int64_t *)s->d_off;
    pp.pt_size = (const int32_t *)s->d_size;
    pp.npids = (int)s->parts.size();
    pp.pids = sa.all_lists ? nullptr : sa.pids;
    pp.P = sa.all_lists ? pp.npids : sa.P;
    pp.M = M;
    pp.nw = nw;
    pp.T = T;
    pp.C = C;
    pp.cand = cand;
    pp.stat = timing ? stat : nullptr;
    if (pp.P < 1 || pp.P > QK_PQ_MAX_NPROBE) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: %d lists per query exceed QK_PQ_MAX_NPROBE=%d", who, pp.P, QK_PQ_MAX_NPROBE);
    const size_t lds = pq_lds_bytes(M, pp.P);
    QK_HIP(hipFuncSetAttribute((const void *)k_pq_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (tm) QK_HIP(hipEventRecord(ctx->ev[5], st));
    hipLaunchKernelGGL(k_pq_select, dim3((unsigned)Q), dim3(256), lds, st, pp);
    QK_HIP(hipGetLastError());
    ctx->last_scan_kernel = "k_pq_select (PQ codes)";
    if (tm) {
        QK_HIP(hipEventRecord(ctx->ev[6], st));
        QK_HIP(hipEventRecord(ctx->ev[7], st));  // (no merge)
    }
    // ---- the exact finish: funnel search's, or its sibling for more candidates than that one pools ---------------------------------
    FunnelFinishParams fp;
    fp.cand = cand;
    fp.xq4 = sa.xq4;
    fp.xn = sa.xn;
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
    QK_TRY(qk_launch_sq8_deep_finish(st, fp, Q));
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
        std::vector<uint2> h_stat((size_t)Q);
        hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(h_stat.data(), stat, (size_t)Q * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            qk_set_error("%s: reading the walk's figures -> %s", who, hipGetErrorString(e));
            rc = QK_ERR_HIP;
        } else {
            int64_t rows = 0, lists = 0;
            for (const uint2 &v : h_stat) rows += v.x, lists += v.y;
            timing->n_items = Q;
            timing->partitions_scanned = lists;
            timing->scan_bytes = rows * (int64_t)nw * 16;
            rc = qk_read_phase_ms(ctx, timing, have_coarse, 4);
            float ms = 0.f;
            if (rc == QK_OK && tm && hipEventElapsedTime(&ms, ctx->ev[7], tail_end) == hipSuccess) timing->total_ms += ms;
        }
    }
    if (tail_end) (void)hipEventDestroy(tail_end);
    QK_TRY(rc);
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

}  // namespace

void qk_store_pq_free(qk_store *s, bool codebooks) {
    if (s->pq_codes) hipFree(s->pq_codes);
    s->pq_codes = nullptr;
    s->pq_cap_rows = 0;
    s->pq_valid = false;
    if (!codebooks) return;
    if (s->pq_cb) hipFree(s->pq_cb);
    if (s->pq_cbn) hipFree(s->pq_cbn);
    if (s->pq_bad) hipFree(s->pq_bad);
    s->pq_cb = s->pq_cbn = nullptr;
    s->pq_bad = nullptr;
    s->pq_M = 0;
}

int qk_store_pq_mirror(qk_ctx *ctx, qk_store *s) {
    if (s->pq_codes && s->pq_valid && s->pq_version == s->version && s->pq_cap_rows >= s->cap_rows) return QK_OK;
    const int d = s->d, M = s->pq_M, dsub = d / M, nw = qk_pq_nw(M);
    if (s->pq_cap_rows < s->cap_rows || !s->pq_codes) {
        const int64_t rows = (std::max<int64_t>(s->cap_rows, 16) + 15) & ~(int64_t)15;
        void *nc = nullptr;
        if (hipMalloc(&nc, (size_t)rows * nw * 16) != hipSuccess) {
            (void)hipGetLastError();
            QK_FAIL(QK_ERR_OOM, "product-quantized search: no device memory for %lld bytes of PQ codes", (long long)rows * nw * 16);
        }
        qk_store_pq_free(s, false);  // (hipFree waits for the device: an earlier call may still read the old mirror)
        s->pq_codes = nc;
        s->pq_cap_rows = rows;
    }
    s->pq_valid = false;
    hipStream_t st = ctx->stream;
    const int64_t nl = (int64_t)s->parts.size();
    int32_t h_bad = 0x7FFFFFFF;
    QK_HIP(hipMemcpyAsync(s->pq_bad, &h_bad, 4, hipMemcpyHostToDevice, st));
    QK_HIP(hipMemsetAsync(s->pq_codes, 0, (size_t)s->pq_cap_rows * nw * 16, st));  // (the padding bytes, the rows behind a list's size)
    if (nl > 0 && s->vecs && s->ntotal > 0) {
        const unsigned gy = nl >= 2048 ? 4 : nl >= 256 ? 16 : 64;  // (few lists: more workgroups per list)
        const int nst = (dsub + 3) / 4;
        const size_t lds = ((size_t)nst * 4 * PQ_CW_STRIDE + 256) * 4;
        QK_HIP(hipFuncSetAttribute((const void *)k_pq_encode, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_pq_encode, dim3((unsigned)nl, gy, (unsigned)M), dim3(256), lds, st, (const float *)s->vecs, s->nblk, M, dsub,
                           (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->pq_cb, (const float *)s->pq_cbn,
                           (uint8_t *)s->pq_codes, s->pq_bad);
        QK_HIP(hipGetLastError());
    }
    QK_HIP(hipMemcpyAsync(&h_bad, s->pq_bad, 4, hipMemcpyDeviceToHost, st));
    QK_HIP(hipStreamSynchronize(st));  // (the one-off build: from here on every stream of the device may read the mirror)
    if (h_bad != 0x7FFFFFFF)
        QK_FAIL(QK_ERR_UNSUPPORTED, "product-quantized search: list %d holds a value that is not finite: no PQ codes for this store", h_bad);
    s->pq_valid = true;
    s->pq_version = s->version;
    return QK_OK;
}

extern "C" {

int qk_pq_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int metric,
                 int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_pq_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_pq_search: nprobe must be positive");
    return qk_pq_run("qk_pq_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, metric, out_ids, out_dist, mem, timing);
}

int qk_pq_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int metric,
               int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_pq_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_pq_scan: bad partition id list");
    return qk_pq_run("qk_pq_scan", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, metric, out_ids, out_dist, mem, timing);
}

int qk_store_pq_set_codebooks(qk_store *s, int M, const float *codebooks) {
    if (!s || !codebooks) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_set_codebooks: null argument");
    QK_TRY(pq_check_m("qk_store_pq_set_codebooks", s->d, M));
    const size_t n = (size_t)256 * s->d;  // (M * 256 * dsub)
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(codebooks[i]))
            QK_FAIL(QK_ERR_INVALID, "qk_store_pq_set_codebooks: codeword %lld of sub-quantizer %lld holds a value that is not finite",
                    (long long)(i / (s->d / M) % 256), (long long)(i / (s->d / M) / 256));
    QK_HIP(hipSetDevice(s->ctx->device));
    float *cb = nullptr;
    if (hipMalloc((void **)&cb, n * 4) != hipSuccess) {
        (void)hipGetLastError();
        QK_FAIL(QK_ERR_OOM, "qk_store_pq_set_codebooks: no device memory for the codebooks");
    }
    if (hipMemcpy(cb, codebooks, n * 4, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(cb);
        QK_FAIL(QK_ERR_HIP, "qk_store_pq_set_codebooks: copying the codebooks failed");
    }
    return pq_adopt(s, M, cb);
}

int qk_store_pq_codebooks(qk_store *s, float *out) {
    if (!s || !out) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_codebooks: null argument");
    if (s->pq_M == 0) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_store_pq_codebooks: the store has no codebooks: train or set codebooks first");
    QK_HIP(hipSetDevice(s->ctx->device));
    QK_HIP(hipMemcpy(out, s->pq_cb, (size_t)256 * s->d * 4, hipMemcpyDeviceToHost));
    return QK_OK;
}

int qk_store_pq_train(qk_ctx *ctx, qk_store *s, int M, int64_t max_rows, int niter, uint64_t seed) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_train: null argument");
    QK_TRY(pq_check_m("qk_store_pq_train", s->d, M));
    if (niter < 1 || max_rows < 256) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_train: niter=%d must be at least 1, max_rows=%lld at least 256", niter, (long long)max_rows);
    QK_HIP(hipSetDevice(ctx->device));
    QK_TRY(qk_store_sync_table(s));
    // the live rows in arena order, by list; the sample: the first n entries of the seeded permutation of their positions
    std::vector<int64_t> first, start;  // per non-empty list: its first arena row, its first position
    int64_t live = 0;
    for (const qk_part &p : s->parts)
        if (p.present && p.size > 0) {
            first.push_back(p.row_off);
            start.push_back(live);
            live += p.size;
        }
    if (live < 256) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_store_pq_train: %lld live rows are fewer than 256 codewords: supply codebooks", (long long)live);
    const int64_t n = std::min<int64_t>(live, max_rows);
    std::vector<int64_t> rows((size_t)n);
    QK_TRY(qk_rand_perm(live, n, seed, rows.data()));
    for (int64_t &v : rows) {
        const size_t li = (size_t)(std::upper_bound(start.begin(), start.end(), v) - start.begin()) - 1;
        v = first[li] + (v - start[li]);
    }
    const int dsub = s->d / M;
    int64_t *d_rows = nullptr, *d_assign = nullptr;
    float *d_x = nullptr, *cb = nullptr;
    auto drop = [&]() {
        if (d_rows) hipFree(d_rows);
        if (d_assign) hipFree(d_assign);
        if (d_x) hipFree(d_x);
    };
    if (hipMalloc((void **)&d_rows, (size_t)n * 8) != hipSuccess || hipMalloc((void **)&d_assign, (size_t)n * 8) != hipSuccess ||
        hipMalloc((void **)&d_x, (size_t)n * dsub * 4) != hipSuccess || hipMalloc((void **)&cb, (size_t)256 * s->d * 4) != hipSuccess) {
        (void)hipGetLastError();
        drop();
        QK_FAIL(QK_ERR_OOM, "qk_store_pq_train: no device memory for a sample of %lld rows", (long long)n);
    }
    hipStream_t st = ctx->stream;
    int rc = hipMemcpyAsync(d_rows, rows.data(), (size_t)n * 8, hipMemcpyHostToDevice, st) == hipSuccess ? QK_OK : QK_ERR_HIP;
    for (int m = 0; m < M && rc == QK_OK; m++) {
        hipLaunchKernelGGL(k_pq_gather, dim3((unsigned)((n * dsub + 255) / 256)), dim3(256), 0, st, (const float *)s->vecs, s->nblk,
                           (const int64_t *)d_rows, n, m, dsub, d_x);
        rc = qk_kmeans(ctx, d_x, n, dsub, 256, QK_METRIC_L2, niter, seed + (uint64_t)m, cb + (size_t)m * 256 * dsub, d_assign, QK_MEM_DEVICE);
    }
    if (rc == QK_OK && hipStreamSynchronize(st) != hipSuccess) rc = QK_ERR_HIP;
    std::vector<float> h((size_t)256 * s->d);
    if (rc == QK_OK && hipMemcpy(h.data(), cb, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = QK_ERR_HIP;
    drop();
    if (rc != QK_OK) {
        hipFree(cb);
        if (rc == QK_ERR_HIP) qk_set_error("qk_store_pq_train: a device call failed");
        return rc;
    }
    for (float v : h)
        if (!std::isfinite(v)) {
            hipFree(cb);
            QK_FAIL(QK_ERR_INVALID, "qk_store_pq_train: the sample gave a codeword that is not finite");
        }
    return pq_adopt(s, M, cb);
}

int qk_store_pq_info(qk_store *s, int *M, int *dsub, int *has_codebooks, int *valid, int64_t *bytes) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_info: null store");
    // (a store with pending changes has no current mirror: the next call rebuilds it)
    const bool cur = s->pq_codes && s->pq_valid && !s->table_dirty && s->pq_version == s->version;
    if (M) *M = s->pq_M;
    if (dsub) *dsub = s->pq_M ? s->d / s->pq_M : 0;
    if (has_codebooks) *has_codebooks = s->pq_M ? 1 : 0;
    if (valid) *valid = cur ? 1 : 0;
    if (bytes) *bytes = s->pq_codes ? s->pq_cap_rows * (int64_t)qk_pq_nw(s->pq_M) * 16 : 0;
    return QK_OK;
}

int qk_store_pq_drop(qk_store *s, int drop_codebooks) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_pq_drop: null store");
    QK_HIP(hipSetDevice(s->ctx->device));
    QK_HIP(hipDeviceSynchronize());  // (searches of other contexts may be reading it)
    qk_store_pq_free(s, drop_codebooks != 0);
    return QK_OK;
}

}  // extern "C"
