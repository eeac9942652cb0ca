// qk_bin_asym.hip -- binary search, asymmetric (include/quake_hip.h, "binary search, asymmetric"): the stored row
// stays one sign bit per coordinate -- binary search's mirror, byte for byte --, the query keeps four bits per coordinate, and two
// float32 factors per row (its centred squared norm r2 and w = r2 / l1) turn the popcounts into an estimate of the inner product
// itself.  The probed rows are ranked by that float32 estimate; everything behind the candidates is binary search's.
//   k_bin_factors      arena tiles -> (r2, w) per arena row; the one-off build, with the sign mirror's validity rule
//   k_bin_prep_asym    one wave per query: lo / hi by shuffles, the four bit planes by ballots, (lo, delta, sumU)
//   k_bin_select_asym  one workgroup per query, no global atomics, no scratch: the query's lists ordered by arena offset as
//                      k_bin_select orders them, three walks of a radix selection over the 32-bit images of the float keys (digits
//                      of 11 / 11 / 10 bits, one LDS histogram), a fourth walk that compacts the rows under the cut image and the
//                      first ties at it in walk order.  Every walk recomputes the keys from the codes: any number of probed rows
// Every float operation of the definition is a separately rounded IEEE operation: the __f*_rn intrinsics, no fma, no packed fp32.
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace {

constexpr int BA_U = 4;              // rows per lane and step: 1024 rows of a walk between two barriers of the compaction
constexpr int BA_BINS = 2048;        // the widest digit: 11 bits

// dynamic LDS of k_bin_select_asym: four planes | list table (offset 8, size 4 bytes per list) | histogram
inline size_t ba_lds_bytes(int d, int P) { return (size_t)qk_bin_nbw(d) * 64 + (size_t)P * 12 + (size_t)BA_BINS * 4; }

// order-preserving image of a float key in the unsigned integers (qk_sq8.hip's sq8_img); a NaN key is the last image
__device__ __forceinline__ uint32_t ba_img(float f) {
    const uint32_t b = __float_as_uint(f);
    return f != f ? 0xFFFFFFFFu : b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// ---- arena tiles -> row factors ------------------------------------------------------------------------------------------------------
__global__ void k_bin_fac_init(uint32_t *flag) {
    if (threadIdx.x == 0) {
        flag[0] = 0u;           // "a factor is not finite"
        flag[1] = 0xFFFFFFFFu;  // the smallest list that holds such a row
    }
}

// blockIdx.x = list, blockIdx.y = slice of its tiles, a wave per tile: k_bin_encode's grid and walk.  Lane (r, g) holds columns
// 16 c + g + {0, 4, 8, 12} of row r in block c -- the columns j = g (mod 4) in ascending order as c and the element rise: it runs
// chain g of the definition over all blocks.  Two shuffles close the row: lanes g and g ^ 1 add their chains (a_0 + a_1, a_2 + a_3;
// float addition commutes bit for bit), then g and g ^ 2 those sums.  Lane group 0 stores float2 (r2, w) at the arena row.
template <bool L2>
__global__ __launch_bounds__(256) void k_bin_factors(const float4 *__restrict__ vecs, int nblk, int d, const int64_t *__restrict__ pt_off,
                                                     const int32_t *__restrict__ pt_size, const float *__restrict__ m, float2 *__restrict__ fac,
                                                     uint32_t *flag) {
    const int size = pt_size[blockIdx.x];
    if (size <= 0) return;
    const int64_t tile0 = pt_off[blockIdx.x] >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int ntl = (size + 15) >> 4;
    bool bad = false;
    for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
        const int64_t tile = tile0 + t;
        const bool live = t * 16 + r < size;
        float a = 0.0f, l = 0.0f;
        if (live)
            for (int c = 0; c < nblk; c++) {
                const float4 v4 = vecs[(tile * nblk + c) * 64 + lane];
                const float x[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int col = 16 * c + 4 * e + g;
                    if (col < d) {
                        const float v = __fsub_rn(x[e], L2 ? m[col] : 0.0f);
                        a = __fadd_rn(a, __fmul_rn(v, v));
                        l = __fadd_rn(l, fabsf(v));
                    }
                }
            }
        a = __fadd_rn(a, __shfl_xor(a, 16));
        l = __fadd_rn(l, __shfl_xor(l, 16));
        const float r2 = __fadd_rn(a, __shfl_xor(a, 32)), l1 = __fadd_rn(l, __shfl_xor(l, 32));
        const float w = l1 == 0.0f ? 0.0f : __fdiv_rn(r2, l1);
        if (live && g == 0) {
            fac[tile * 16 + r] = make_float2(r2, w);
            bad |= !(fabsf(r2) <= FLT_MAX) || !(fabsf(w) <= FLT_MAX);  // (NaN: not <=)
        }
    }
    if (__ballot(bad) != 0 && lane == 0) {
        atomicOr(&flag[0], 1u);
        atomicMin(&flag[1], (uint32_t)blockIdx.x);
    }
}

// ---- query preparation ------------------------------------------------------------------------------------------------------------
// q'_j = q_j - m_j, a value that is not finite or is -0 replaced by +0 (so min and max are one bit pattern whatever their order)
template <bool L2>
__device__ __forceinline__ float ba_centred(const float *__restrict__ s, const float *__restrict__ m, int j) {
    const float v = __fsub_rn(s[j], L2 ? m[j] : 0.0f);
    return fabsf(v) <= FLT_MAX && v != 0.0f ? v : 0.0f;
}

// One wave per query.  lo / hi: every lane folds columns lane + 64 i, six shuffles each.  A 128-column word of plane b is two ballots
// of bit b of u, lane l deciding columns 128 w + l and 128 w + 64 + l as k_bin_prep does: planes [q][b][w].  qf [q] = (lo, delta,
// sumU as bits, 0).
template <bool L2>
__global__ __launch_bounds__(64) void k_bin_prep_asym(const float *__restrict__ x, int d, int nbw, const float *__restrict__ m,
                                                      uint4 *__restrict__ planes, float4 *__restrict__ qf) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *s = x + q * d;
    float lo = INFINITY, hi = -INFINITY;
    for (int j = lane; j < d; j += 64) {
        const float v = ba_centred<L2>(s, m, j);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    float delta = __fdiv_rn(__fsub_rn(hi, lo), 15.0f);
    if (delta == 0.0f) delta = 1.0f;
    int sum = 0;
    for (int w = 0; w < nbw; w++) {
        int u[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = 128 * w + 64 * h + lane;
            // (a NaN -- infinite over infinite, where hi - lo overflows -- is 0: fmaxf returns the other operand)
            u[h] = j < d ? (int)fminf(fmaxf(rintf(__fdiv_rn(__fsub_rn(ba_centred<L2>(s, m, j), lo), delta)), 0.0f), 15.0f) : 0;
            sum += u[h];
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const unsigned long long m0 = __ballot((u[0] >> b) & 1), m1 = __ballot((u[1] >> b) & 1);
            if (lane == 0) planes[(q * 4 + b) * nbw + w] = make_uint4((uint32_t)m0, (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)(m1 >> 32));
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) qf[q] = make_float4(lo, delta, __int_as_float(sum), 0.0f);
}

// ---- the selection ------------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of v over the workgroup's 256 threads in thread order; total = the sum.  s_w [4]  (k_bin_select's)
__device__ __forceinline__ uint32_t ba_scan_excl(uint32_t v, uint32_t *s_w, uint32_t &total) {
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

// the key images of rows i0 + 256 u, u < BA_U, of the list at arena row `off` (rows behind its size: the last row's, unused).  Per
// 128-column block one 16-byte load per row; per dword four v_and_b32 against the planes' words, broadcast from LDS, and five
// v_bcnt_u32_b32 whose built-in add keeps one accumulator per plane and one for the row's own bits: the shifts by 2^b happen once
// per row.  The loads of the BA_U rows -- a block's words and the float2 factors -- are independent: they are in flight together.
//   S = sum_b 2^b popcount(plane_b & code), t = 2 S - sumU, p = 2 popcount(code) - d   (exact integers below 2^24)
//   e = delta * t + lo * p;   L2: key = r2 - 2 (w e);   IP: key = -(w e)
template <bool L2>
__device__ __forceinline__ void ba_keys(const uint4 *__restrict__ codes, const float2 *__restrict__ fac, int nbw, int d, const uint4 *s_pl, float lo,
                                        float delta, int sumU, int64_t off, int size, int i0, uint32_t *img) {
    const uint4 *src[BA_U];
    float2 f[BA_U];
    uint32_t acc[BA_U][4], pop[BA_U];
#pragma unroll
    for (int u = 0; u < BA_U; u++) {
        const int64_t row = off + min(i0 + 256 * u, size - 1);
        src[u] = codes + (row >> 4) * nbw * 16 + (row & 15);
        f[u] = fac[row];
        pop[u] = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) acc[u][b] = 0u;
    }
    for (int w = 0; w < nbw; w++) {
        uint4 v[BA_U];
#pragma unroll
        for (int u = 0; u < BA_U; u++) v[u] = src[u][w * 16];
#pragma unroll
        for (int u = 0; u < BA_U; u++)
            pop[u] = __builtin_popcount(v[u].x) + __builtin_popcount(v[u].y) + __builtin_popcount(v[u].z) + __builtin_popcount(v[u].w) + pop[u];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint4 qv = s_pl[b * nbw + w];
#pragma unroll
            for (int u = 0; u < BA_U; u++) {
                acc[u][b] = __builtin_popcount(v[u].x & qv.x) + acc[u][b];
                acc[u][b] = __builtin_popcount(v[u].y & qv.y) + acc[u][b];
                acc[u][b] = __builtin_popcount(v[u].z & qv.z) + acc[u][b];
                acc[u][b] = __builtin_popcount(v[u].w & qv.w) + acc[u][b];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < BA_U; u++) {
        const int S = (int)(acc[u][0] + 2u * acc[u][1] + 4u * acc[u][2] + 8u * acc[u][3]);
        const int t = 2 * S - sumU, p = 2 * (int)pop[u] - d;
        const float e = __fadd_rn(__fmul_rn(delta, (float)t), __fmul_rn(lo, (float)p));
        const float we = __fmul_rn(f[u].y, e);
        img[u] = ba_img(L2 ? __fsub_rn(f[u].x, __fmul_rn(2.0f, we)) : -we);
    }
}

// blockIdx.x = query, 256 threads.  Dynamic LDS (ba_lds_bytes): [4][nbw] uint4 planes | [P] int64 list offsets | [P] int32 sizes |
// [2048] uint32 histogram.
//   1. the lists: k_bin_select's step 1 -- -1, absent and empty lists leave, the rest are ranked by (offset, entry) and written back
//      in that order: every walk below is in arena order, which is the tie rule of the definition.  A sum of the sizes gives the
//      probed rows.  Not more probed rows than fetch_k: no cut, step 3 takes every row.
//   2. the cut image K: three rounds over the digits img >> 21, (img >> 10) & 2047, img & 1023.  A round clears the histogram,
//      walks the probed rows and counts the digit of those whose higher digits equal the prefix found so far; thread t then sums
//      bins 8 t .. 8 t + 7, a prefix sum finds the thread and that thread the digit D with fewer than rem = fetch_k - c0 rows under
//      it and at least rem up to it.  c0 grows by the rows under D, the prefix by D.  After round 3 the prefix is K, c0 the rows whose
//      image is below K, need = fetch_k - c0 of the rows at K are taken.
//   3. the compaction, k_bin_select's pass B with the test on images: BA_U x 256 rows per step.  A row is taken if img < K, or
//      img == K and fewer than need ties came before it in the walk.  Every wave publishes (rows under K, ties) of each of its BA_U
//      ballots, one barrier (the buffers alternate), then every thread runs through the 4 BA_U pairs in walk order -- the same
//      running totals in every thread -- and knows the slot of its rows: taken rows land in cand[q] in ascending arena rows.
struct BinAsymSelectParams {
    const uint4 *codes;
    const float2 *fac;
    const int64_t *pt_off;
    const int32_t *pt_size;
    int npids;
    const int64_t *pids;  // [Q][P], or nullptr: list pi is list number pi
    int P, nbw, d;
    const uint4 *planes;  // [Q][4][nbw]
    const float4 *qf;     // [Q] (lo, delta, sumU as bits, -)
    int C;                // fetch_k
    int64_t *cand;        // [Q][C] arena rows in ascending order, -1 behind
    uint2 *stat;          // [Q] {probed rows, lists walked}, or nullptr
};

template <bool L2>
__global__ __launch_bounds__(256) void k_bin_select_asym(BinAsymSelectParams B) {
    extern __shared__ uint4 ba_lds[];
    __shared__ uint32_t s_w[4], s_cut[2];
    __shared__ uint2 s_cnt[2][4 * BA_U];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int P = B.P, nbw = B.nbw, d = B.d, C = B.C;
    uint4 *s_pl = ba_lds;
    int64_t *s_off = (int64_t *)(s_pl + 4 * nbw);
    int32_t *s_size = (int32_t *)(s_off + P);
    uint32_t *s_hist = (uint32_t *)(s_size + P);
    // ---- 1. the query, the lists in arena order
    for (int i = tid; i < 4 * nbw; i += 256) s_pl[i] = B.planes[q * 4 * nbw + i];
    const float4 qf = B.qf[q];
    const float lo = qf.x, delta = qf.y;
    const int sumU = __float_as_int(qf.z);
    constexpr int LPT = QK_BIN_MAX_NPROBE / 256;
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
    (void)ba_scan_excl(mine, s_w, total);
    (void)ba_scan_excl(live, s_w, nlists);
    const bool all = total <= (uint32_t)C;  // no cut
    // ---- 2. the cut image
    uint32_t K = 0u, c0 = 0u;
    for (int rd = 0; rd < 3 && !all; rd++) {
        const int shift = rd == 0 ? 21 : rd == 1 ? 10 : 0, bits = rd == 2 ? 10 : 11;
        for (int i = tid; i < BA_BINS; i += 256) s_hist[i] = 0u;
        __syncthreads();
        for (int li = 0; li < (int)nlists; li++) {
            const int size = s_size[li];
            const int64_t loff = s_off[li];
            for (int i0 = tid; i0 < size; i0 += 256 * BA_U) {
                uint32_t img[BA_U];
                ba_keys<L2>(B.codes, B.fac, nbw, d, s_pl, lo, delta, sumU, loff, size, i0, img);
#pragma unroll
                for (int u = 0; u < BA_U; u++)
                    if (i0 + 256 * u < size && (rd == 0 || (img[u] >> (shift + bits)) == K))
                        atomicAdd(&s_hist[(img[u] >> shift) & ((1u << bits) - 1u)], 1u);
            }
        }
        __syncthreads();
        {
            constexpr int CH = BA_BINS / 256;
            const uint32_t rem = (uint32_t)C - c0;
            uint32_t sum = 0;
#pragma unroll
            for (int b = 0; b < CH; b++) sum += s_hist[CH * tid + b];
            uint32_t tot;
            const uint32_t ex = ba_scan_excl(sum, s_w, tot);
            if (ex < rem && rem <= ex + sum) {  // (exactly one thread: the rows that match the prefix are at least rem)
                uint32_t c = ex;
                int b = CH * tid;
                while (c + s_hist[b] < rem) c += s_hist[b++];
                s_cut[0] = (uint32_t)b;
                s_cut[1] = c0 + c;
            }
        }
        __syncthreads();
        K = (K << bits) | s_cut[0];
        c0 = s_cut[1];
    }
    const uint32_t target = min(total, (uint32_t)C);
    const uint32_t need = all ? 0u : target - c0;
    // ---- 3. the compaction
    int64_t *cand = B.cand + q * C;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run_t = 0, run_e = 0;  // rows taken / ties seen so far: the same in every thread
    int par = 0;
    for (int li = 0; li < (int)nlists && run_t < target; li++) {
        const int size = s_size[li];
        const int64_t loff = s_off[li];
        for (int s0 = 0; s0 < size && run_t < target; s0 += 256 * BA_U) {
            const int i0 = s0 + tid;
            uint32_t img[BA_U];
            if (all) {
#pragma unroll
                for (int u = 0; u < BA_U; u++) img[u] = 0u;
            } else {
                ba_keys<L2>(B.codes, B.fac, nbw, d, s_pl, lo, delta, sumU, loff, size, i0, img);
            }
            unsigned long long bl[BA_U], bt[BA_U];
#pragma unroll
            for (int u = 0; u < BA_U; u++) {
                const bool valid = i0 + 256 * u < size;
                bl[u] = __ballot(valid && (all || img[u] < K));
                bt[u] = __ballot(valid && !all && img[u] == K);
                if (lane == 0) s_cnt[par][4 * u + wave] = make_uint2((uint32_t)__popcll(bl[u]), (uint32_t)__popcll(bt[u]));
            }
            __syncthreads();
            uint32_t base_t[BA_U], base_e[BA_U];
#pragma unroll
            for (int e = 0; e < 4 * BA_U; e++) {
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
            for (int u = 0; u < BA_U; u++) {
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

}  // namespace

void qk_store_bin_fac_free(qk_store *s) {
    if (s->bin_fac) hipFree(s->bin_fac);
    if (s->bin_fac_flag) hipFree(s->bin_fac_flag);
    s->bin_fac = nullptr;
    s->bin_fac_flag = nullptr;
    s->bin_fac_cap_rows = 0;
    s->bin_fac_metric = -1;
}

int qk_store_bin_factors(qk_ctx *ctx, qk_store *s, int metric) {
    if (s->bin_fac && s->bin_fac_metric == metric && s->bin_fac_version == s->version && s->bin_fac_cap_rows >= s->cap_rows) return QK_OK;
    if (!s->bin_codes || s->bin_metric != metric || s->bin_version != s->version)
        QK_FAIL(QK_ERR_INVALID, "binary search, asymmetric: the row factors need the sign mirror's centres");
    if (s->bin_fac_cap_rows < s->cap_rows || !s->bin_fac) {
        // (both or none: a call without memory leaves the store as it was)
        const int64_t rows = (std::max<int64_t>(s->cap_rows, 16) + 15) & ~(int64_t)15;
        void *nf = nullptr, *ng = nullptr;
        if (hipMalloc(&nf, (size_t)rows * 8) != hipSuccess || hipMalloc(&ng, 8) != hipSuccess) {
            (void)hipGetLastError();
            if (nf) hipFree(nf);
            QK_FAIL(QK_ERR_OOM, "binary search, asymmetric: no device memory for %lld bytes of row factors", (long long)rows * 8);
        }
        qk_store_bin_fac_free(s);  // (hipFree waits for the device: an earlier call may still read the old factors)
        s->bin_fac = nf;
        s->bin_fac_flag = (uint32_t *)ng;
        s->bin_fac_cap_rows = rows;
    }
    s->bin_fac_metric = -1;
    hipStream_t st = ctx->stream;
    const int64_t nl = (int64_t)s->parts.size();
    if (nl > 0 && s->vecs && s->ntotal > 0) {
        const unsigned gy = nl >= 2048 ? 4 : nl >= 256 ? 16 : 64;  // (k_bin_encode's grid)
        uint32_t h_flag[2] = {0u, 0u};
        hipLaunchKernelGGL(k_bin_fac_init, dim3(1), dim3(64), 0, st, s->bin_fac_flag);
        if (metric == QK_METRIC_L2)
            hipLaunchKernelGGL(k_bin_factors<true>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, s->d,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->bin_m, (float2 *)s->bin_fac, s->bin_fac_flag);
        else
            hipLaunchKernelGGL(k_bin_factors<false>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, s->d,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->bin_m, (float2 *)s->bin_fac, s->bin_fac_flag);
        QK_HIP(hipGetLastError());
        QK_HIP(hipMemcpyAsync(h_flag, s->bin_fac_flag, 8, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));  // (the one-off build: from here on every stream of the device may read the factors)
        if (h_flag[0] != 0u)
            QK_FAIL(QK_ERR_UNSUPPORTED, "binary search, asymmetric: list %lld holds a row whose norm factors are not finite: no row factors for this store",
                    (long long)h_flag[1]);
    }
    s->bin_fac_metric = metric;
    s->bin_fac_version = s->version;
    return QK_OK;
}

size_t qk_bin_asym_query_bytes(int64_t Q, int d) { return qk_al256((size_t)Q * qk_bin_nbw(d) * 64) + qk_al256((size_t)Q * 16); }

int qk_launch_bin_prep_asym(hipStream_t st, const qk_store *s, const float *x, int64_t Q, int metric, void *planes, void *qf) {
    const int d = s->d, nbw = qk_bin_nbw(d);
    if (metric == QK_METRIC_L2)
        hipLaunchKernelGGL(k_bin_prep_asym<true>, dim3((unsigned)Q), dim3(64), 0, st, x, d, nbw, (const float *)s->bin_m, (uint4 *)planes, (float4 *)qf);
    else
        hipLaunchKernelGGL(k_bin_prep_asym<false>, dim3((unsigned)Q), dim3(64), 0, st, x, d, nbw, (const float *)s->bin_m, (uint4 *)planes, (float4 *)qf);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

int qk_launch_bin_select_asym(hipStream_t st, const qk_store *s, const qk_scan_args &sa, int metric, const void *planes, const void *qf,
                              int fetch_k, int64_t *cand, uint2 *stat, int64_t Q) {
    BinAsymSelectParams bp;
    bp.codes = (const uint4 *)s->bin_codes;
    bp.fac = (const float2 *)s->bin_fac;
    bp.pt_off = (const int64_t *)s->d_off;
    bp.pt_size = (const int32_t *)s->d_size;
    bp.npids = (int)s->parts.size();
    bp.pids = sa.all_lists ? nullptr : sa.pids;
    bp.P = sa.all_lists ? bp.npids : sa.P;
    bp.nbw = qk_bin_nbw(s->d);
    bp.d = s->d;
    bp.planes = (const uint4 *)planes;
    bp.qf = (const float4 *)qf;
    bp.C = fetch_k;
    bp.cand = cand;
    bp.stat = stat;
    if (bp.P < 1 || bp.P > QK_BIN_MAX_NPROBE || fetch_k < 1 || fetch_k > QK_BIN_MAX_FETCH || s->d > QK_MAX_D)
        QK_FAIL(QK_ERR_UNSUPPORTED, "k_bin_select_asym: %d lists per query (at most QK_BIN_MAX_NPROBE=%d), fetch_k=%d, d=%d are outside its range", bp.P,
                QK_BIN_MAX_NPROBE, fetch_k, s->d);
    const size_t lds = ba_lds_bytes(s->d, bp.P);
    if (metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_bin_select_asym<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_bin_select_asym<true>, dim3((unsigned)Q), dim3(256), lds, st, bp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_bin_select_asym<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_bin_select_asym<false>, dim3((unsigned)Q), dim3(256), lds, st, bp);
    }
    QK_HIP(hipGetLastError());
    return QK_OK;
}

extern "C" {

int qk_store_bin_asym_info(qk_store *s, int *valid, int64_t *bytes) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_bin_asym_info: null store");
    // (a store with pending changes has no current factors: the next asymmetric call rebuilds them)
    if (valid) *valid = s->bin_fac && s->bin_fac_metric >= 0 && !s->table_dirty && s->bin_fac_version == s->version ? 1 : 0;
    if (bytes) *bytes = s->bin_fac ? s->bin_fac_cap_rows * 8 : 0;
    return QK_OK;
}

}  // extern "C"
