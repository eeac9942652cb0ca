// qk_bin.hip -- binary search (include/quake_hip.h, "binary search"): binary quantization with oversampling and
// rescoring.  Every coordinate of the store is mirrored as one sign bit b_j = (x_j > m_j); per query the fetch_k rows of its probed
// lists with the smallest Hamming distance to the query's bits -- ties by arena row -- are re-scored on the float32 rows, the k best
// under (exact key, id) returned.
// The mirror: code row r is arena row r.  A 128-column block of a row is one 16-byte word (bit j % 128 of it is column j, dwords
// little-endian); the 16 words of a tile's rows lie side by side (256 B), the blocks of a tile one after the other:
//     uint4 index (tile nbw + w) 16 + r,   nbw = ceil(d / 128)
// so at nbw = 1 the mirror is one contiguous stream of 16 B per arena row.  One enqueue on the context's stream, no host wait inside --
// except the one-off build of the mirror:
//   (k_sq8_range<true>  L2 only: quantized search's column centres, qk_sq8.hip)
//   k_bin_encode       arena tiles -> code tiles
//   k_bin_prep         the queries' bit words
//   (coarse: the shipped one)
//   k_bin_select       one workgroup per query, no global atomics: the query's lists ordered by arena offset, pass A (keys by
//                      popcount, a histogram of d + 1 bins and -- where the probed rows fit -- the keys themselves in LDS), the cut key
//                      by a prefix sum, pass B (the rows under the cut and the first ties at it, compacted in walk order)
//   (k_sq8_prep, k_sq8_rerank: the rescored form only -- "binary search, rescored"; qk_sq8.hip, qk_cascade.hip)
//   (k_funnel_finish / k_sq8_deep_finish: the exact finish of funnel search and of deep quantized search, unchanged.  Neither reads
//    anything from the order of its candidates: both pool (exact key, id) by order of arrival and select under (key, id))
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"

#include <algorithm>
#include <cstring>
#include <vector>

// 1: pass A keeps the keys of a query's probed rows in LDS as uint16 where they fit and pass B reads them back; 0: pass B always
// recomputes them from the codes.  Measured (profiles/bin_probe.jsonl, labels "key_cache" / "product"): at 10M x 128
// the cache costs 0.06 - 1.3 ms of select time -- its LDS takes the occupancy the 16-byte re-read needs less --, at 10M x 768 it
// saves 0.03 - 0.1 ms of calls that take 0.5 - 8.8 ms.  The product build is 0
#ifndef QK_BIN_KEY_CACHE
#define QK_BIN_KEY_CACHE 0
#endif

namespace {

constexpr int BIN_LDS = 160 * 1024;   // LDS of a gfx950 workgroup
constexpr int BIN_LDS_STATIC = 1024;  // what k_bin_select keeps outside its dynamic region, rounded up
constexpr int BIN_U = 4;              // rows per lane and step: 1024 rows of the walk between two barriers of pass B

inline size_t bin_hist_bytes(int d) { return (size_t)((d + 1 + 3) & ~3) * 4; }
// dynamic LDS of k_bin_select: query words | list table (offset 8, size 4, first walk position 4 bytes per list) | histogram | keys
inline size_t bin_lds_bytes(int d, int P, int64_t cache_rows) {
    return (size_t)qk_bin_nbw(d) * 16 + (size_t)P * 16 + bin_hist_bytes(d) + (size_t)cache_rows * 2;
}
// THE CAPACITY OF THE LDS KEY CACHE: the most probed rows of one query whose uint16 keys fit behind the query, a full list table
// (QK_BIN_MAX_NPROBE entries) and the histogram -- a function of d alone: 73072 rows at d = 64, 72944 at d = 128, 56312 at d = 8192
inline int64_t bin_cache_rows(int d) {
    return (int64_t)((BIN_LDS - BIN_LDS_STATIC - bin_lds_bytes(d, QK_BIN_MAX_NPROBE, 0)) / 2) & ~(int64_t)7;
}

// ---- arena tiles -> code tiles ------------------------------------------------------------------------------------------------------
// blockIdx.x = list, blockIdx.y = slice of its tiles, a wave per tile.  Lane (g, r) reads the arena as the scan does -- block c: row
// r, columns 16 c + g + {0, 4, 8, 12} -- compares its four values and shifts the results to their places in the row's word: arena
// block c = 8 w + cc fills bits 16 (cc & 1) + 4 e + g of dword cc >> 1.  The four lane groups of a row hold disjoint bits: two
// shuffles per dword OR them, lane group 0 stores the 16 words of the tile (256 B).  Rows of a last tile behind the list's size,
// columns from d on and blocks the arena does not have hold 0.
template <bool L2>
__global__ __launch_bounds__(256) void k_bin_encode(const float4 *__restrict__ vecs, int nblk, int nbw, int d, const int64_t *__restrict__ pt_off,
                                                    const int32_t *__restrict__ pt_size, const float *__restrict__ m, uint4 *__restrict__ codes) {
    const int size = pt_size[blockIdx.x];
    if (size <= 0) return;
    const int64_t tile0 = pt_off[blockIdx.x] >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int ntl = (size + 15) >> 4;
    for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
        const int64_t tile = tile0 + t;
        const bool live = t * 16 + r < size;
        for (int w = 0; w < nbw; w++) {
            uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int cc = 0; cc < 8; cc++) {
                const int c = 8 * w + cc;
                if (!live || c >= nblk) continue;
                const float4 v4 = vecs[(tile * nblk + c) * 64 + lane];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int col = 16 * c + 4 * e + g;
                    const bool bit = col < d && v[e] > (L2 ? m[col] : 0.0f);  // (ordered: NaN gives 0)
                    b[cc >> 1] |= (bit ? 1u : 0u) << (16 * (cc & 1) + 4 * e + g);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                b[i] |= __shfl_xor(b[i], 16);
                b[i] |= __shfl_xor(b[i], 32);
            }
            if (g == 0) codes[(tile * nbw + w) * 16 + r] = make_uint4(b[0], b[1], b[2], b[3]);
        }
    }
}

// ---- query preparation ------------------------------------------------------------------------------------------------------------
// One wave per query: a 128-column word is two ballots of 64 comparisons, lane l deciding columns 128 w + l and 128 w + 64 + l.
template <bool L2>
__global__ __launch_bounds__(64) void k_bin_prep(const float *__restrict__ x, int d, int nbw, const float *__restrict__ m, uint4 *__restrict__ xq) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float *s = x + q * d;
    for (int w = 0; w < nbw; w++) {
        const int c0 = 128 * w + lane, c1 = c0 + 64;
        const bool b0 = c0 < d && s[c0] > (L2 ? m[c0] : 0.0f);
        const bool b1 = c1 < d && s[c1] > (L2 ? m[c1] : 0.0f);
        const unsigned long long m0 = __ballot(b0), m1 = __ballot(b1);
        if (lane == 0) xq[q * nbw + w] = make_uint4((uint32_t)m0, (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)(m1 >> 32));
    }
}

// ---- the selection ------------------------------------------------------------------------------------------------------------------
struct BinSelectParams {
    const uint4 *codes;
    const int64_t *pt_off;
    const int32_t *pt_size;
    int npids;
    const int64_t *pids;  // [Q][P], or nullptr: list pi is list number pi
    int P, nbw, nbins;    // nbins = d + 1
    const uint4 *xq;      // [Q][nbw]
    int C;                // fetch_k
    int64_t *cand;        // [Q][C] arena rows in ascending order, -1 behind
    int cache_rows;       // uint16 keys the dynamic LDS has room for (a multiple of 8; 0: none)
    uint2 *stat;          // [Q] {probed rows, lists walked}, or nullptr
};

// exclusive prefix sum of v over the workgroup's 256 threads in thread order; total = the sum.  s_w [4]
__device__ __forceinline__ uint32_t wg_scan_excl(uint32_t v, uint32_t *s_w, uint32_t &total) {
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

// the Hamming keys of rows i0 + 256 u, u < BIN_U, of the list at arena row `off` (rows behind its size: the last row's key, unused):
// per 128-column block one 16-byte load per row against the query's word, broadcast from LDS; v_xor_b32 and v_bcnt_u32_b32 with
// its built-in add per dword.  The BIN_U loads of a block are independent: they are in flight together
__device__ __forceinline__ void bin_keys(const uint4 *__restrict__ codes, int nbw, const uint4 *s_q, int64_t off, int size, int i0, uint32_t *h) {
    const uint4 *src[BIN_U];
#pragma unroll
    for (int u = 0; u < BIN_U; u++) {
        const int64_t row = off + min(i0 + 256 * u, size - 1);
        src[u] = codes + (row >> 4) * nbw * 16 + (row & 15);
        h[u] = 0u;
    }
    for (int w = 0; w < nbw; w++) {
        const uint4 qv = s_q[w];
#pragma unroll
        for (int u = 0; u < BIN_U; u++) {
            const uint4 v = src[u][w * 16];
            h[u] = __builtin_popcount(v.x ^ qv.x) + h[u];
            h[u] = __builtin_popcount(v.y ^ qv.y) + h[u];
            h[u] = __builtin_popcount(v.z ^ qv.z) + h[u];
            h[u] = __builtin_popcount(v.w ^ qv.w) + h[u];
        }
    }
}

// blockIdx.x = query, 256 threads.  Dynamic LDS (bin_lds_bytes): [nbw] uint4 query | [P] int64 list offsets | [P] int32 sizes |
// [P] uint32 first walk position | [d + 1, rounded up to 4] uint32 histogram | [cache_rows] uint16 keys.
//   1. the lists: thread t holds entries t + 256 j of the pids row (-1, absent and empty lists: offset "last", size 0), ranks them by
//      (offset, entry) against all P in LDS and writes them back in that order: the walk below is in arena order, which is the
//      tie rule of the definition for free.  A prefix sum of the sizes gives every list's first walk position and the total.
//   2. pass A: every probed row's key -> histogram (LDS atomics), and -> s_key[walk position] where the total fits cache_rows.
//   3. the cut: thread t sums its share of the bins, a prefix sum finds the thread, that thread the key b with c0 rows under it
//      (c0 < fetch_k <= c0 + rows at b).  Fewer probed rows than fetch_k: no cut, every row is taken.
//   4. pass B: the same walk, BIN_U x 256 rows per step.  A row is taken if h < b, or h == b and fewer than need = fetch_k - c0 ties
//      came before it in the walk.  Every wave publishes (rows under b, ties) of each of its BIN_U ballots, one barrier (the
//      buffers alternate), then every thread runs through the 4 BIN_U pairs in walk order -- the same running totals in every
//      thread -- and knows the slot of its rows: taken rows land in cand[q] in walk order, ascending arena rows.
__global__ __launch_bounds__(256) void k_bin_select(BinSelectParams B) {
    extern __shared__ uint4 bs_lds[];
    __shared__ uint32_t s_w[4], s_cut[2];
    __shared__ uint2 s_cnt[2][4 * BIN_U];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int P = B.P, nbw = B.nbw, nbins = B.nbins, C = B.C;
    uint4 *s_q = bs_lds;
    int64_t *s_off = (int64_t *)(s_q + nbw);
    int32_t *s_size = (int32_t *)(s_off + P);
    uint32_t *s_start = (uint32_t *)(s_size + P);
    uint32_t *s_hist = s_start + P;
    uint16_t *s_key = (uint16_t *)(s_hist + ((nbins + 3) & ~3));
    // ---- 1. the query, the histogram, the lists in arena order
    for (int i = tid; i < nbw; i += 256) s_q[i] = B.xq[q * nbw + i];
    for (int i = tid; i < nbins; i += 256) s_hist[i] = 0u;
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
    uint32_t pos = wg_scan_excl(mine, s_w, total);
    (void)wg_scan_excl(live, s_w, nlists);
#pragma unroll
    for (int j = 0; j < LPT; j++) {
        const int e = LPT * tid + j;
        if (e < P) {
            s_start[e] = pos;
            pos += (uint32_t)s_size[e];
        }
    }
    __syncthreads();
    const bool cached = QK_BIN_KEY_CACHE && total <= (uint32_t)B.cache_rows;
    // ---- 2. pass A
    for (int li = 0; li < (int)nlists; li++) {
        const int size = s_size[li];
        const int64_t loff = s_off[li];
        const uint32_t fb = s_start[li];
        for (int i0 = tid; i0 < size; i0 += 256 * BIN_U) {
            uint32_t h[BIN_U];
            bin_keys(B.codes, nbw, s_q, loff, size, i0, h);
#pragma unroll
            for (int u = 0; u < BIN_U; u++) {
                const int i = i0 + 256 * u;
                if (i < size) {
                    atomicAdd(&s_hist[min(h[u], (uint32_t)nbins - 1u)], 1u);  // (h <= d: the padding bits are 0 on both sides)
                    if (cached) s_key[fb + i] = (uint16_t)h[u];
                }
            }
        }
    }
    // ---- 3. the cut
    if (tid == 0) {
        s_cut[0] = (uint32_t)nbins;  // (no key reaches it: every row lies under the cut)
        s_cut[1] = total;
    }
    __syncthreads();
    {
        const int chunk = (nbins + 255) / 256, b0 = tid * chunk, b1 = min(b0 + chunk, nbins);
        uint32_t sum = 0;
        for (int b = b0; b < b1; b++) sum += s_hist[b];
        uint32_t tot;
        const uint32_t ex = wg_scan_excl(sum, s_w, tot);
        if (ex < (uint32_t)C && (uint32_t)C <= ex + sum) {  // (exactly one thread, where the probed rows are at least fetch_k)
            uint32_t c = ex;
            int b = b0;
            while (c + s_hist[b] < (uint32_t)C) c += s_hist[b++];
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
        const uint32_t fb = s_start[li];
        for (int s0 = 0; s0 < size && run_t < target; s0 += 256 * BIN_U) {
            const int i0 = s0 + tid;
            uint32_t h[BIN_U];
            if (cached) {
#pragma unroll
                for (int u = 0; u < BIN_U; u++) h[u] = i0 + 256 * u < size ? (uint32_t)s_key[fb + i0 + 256 * u] : 0u;
            } else {
                bin_keys(B.codes, nbw, s_q, loff, size, i0, h);
            }
            unsigned long long bl[BIN_U], bt[BIN_U];
#pragma unroll
            for (int u = 0; u < BIN_U; u++) {
                const bool valid = i0 + 256 * u < size;
                bl[u] = __ballot(valid && h[u] < cut);
                bt[u] = __ballot(valid && h[u] == cut);
                if (lane == 0) s_cnt[par][4 * u + wave] = make_uint2((uint32_t)__popcll(bl[u]), (uint32_t)__popcll(bt[u]));
            }
            __syncthreads();
            uint32_t base_t[BIN_U], base_e[BIN_U];
#pragma unroll
            for (int e = 0; e < 4 * BIN_U; e++) {
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
            for (int u = 0; u < BIN_U; u++) {
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

// the body of the entry points: parent == nullptr && pids == nullptr -> every list.  rescore_k >= 0: the rescored form ("binary search,
// rescored") -- k_sq8_rerank (qk_cascade.hip) between the selection and the finish, which then sees rescore_k candidates.
// asym: the candidates by k_bin_prep_asym / k_bin_select_asym over the same sign mirror and the row factors ("binary search,
// asymmetric"; qk_bin_asym.hip); everything else is the same call
int qk_bin_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe, int k,
               int fetch_k, int rescore_k, bool asym, int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    const int d = s->d;
    const bool rescored = rescore_k >= 0;
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
    if (fetch_k < k) QK_FAIL(QK_ERR_INVALID, "%s: fetch_k=%d must be at least k=%d", who, fetch_k, k);
    if (rescored && rescore_k < k) QK_FAIL(QK_ERR_INVALID, "%s: rescore_k=%d must be at least k=%d", who, rescore_k, k);
    if (rescored && rescore_k > fetch_k) QK_FAIL(QK_ERR_INVALID, "%s: rescore_k=%d must be at most fetch_k=%d", who, rescore_k, fetch_k);
    if (Q < 0 || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (mem != QK_MEM_HOST && mem != QK_MEM_DEVICE) QK_FAIL(QK_ERR_INVALID, "%s: mem must be QK_MEM_HOST or QK_MEM_DEVICE", who);
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d", who, k, QK_MAX_K);
    if (rescored && rescore_k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: rescore_k=%d exceeds QK_MAX_K=%d", who, rescore_k, QK_MAX_K);
    if (fetch_k > QK_BIN_MAX_FETCH) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: fetch_k=%d exceeds QK_BIN_MAX_FETCH=%d", who, fetch_k, QK_BIN_MAX_FETCH);
    if (rescored && d > QK_SQ8_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_SQ8_MAX_D=%d", who, d, QK_SQ8_MAX_D);
    if (d > QK_MAX_D) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: d=%d exceeds QK_MAX_D=%d", who, d, QK_MAX_D);
    if (!parent && !pids && s->nlist == 1)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a flat index without lists of its own takes the dense path, which has no sign code form", who);
    // lists per query: the coarse step's min(nprobe, parent rows), the pids row, or every list of the store
    const int64_t Pq = parent ? std::max<int64_t>(std::min<int64_t>(nprobe, parent->ntotal), 1) : pids ? P : (int64_t)s->parts.size();
    if (Pq > QK_BIN_MAX_NPROBE) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: %lld lists per query exceed QK_BIN_MAX_NPROBE=%d", who, (long long)Pq, QK_BIN_MAX_NPROBE);
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
    const int C = fetch_k, R = rescored ? rescore_k : fetch_k, nblk = s->nblk, nbw = qk_bin_nbw(d), nb8 = qk_sq8_nblk(d);
    // ---- the mirror and the call's buffer: what can refuse or fail for want of memory comes first -----------------------------------
    QK_TRY(qk_store_sync_table(s));
    const int64_t rows_ub = Pq * std::max<int64_t>(s->max_size, 0);  // (walk positions and bin counts are 32-bit)
    if (rows_ub >= ((int64_t)1 << 32)) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: a query could probe %lld rows, 2^32 or more", who, (long long)rows_ub);
    // (the int8 codes first: a store with a non-finite row is refused in quantized search's words, for both metrics)
    if (rescored) QK_TRY(qk_store_sq8_mirror(ctx, s, metric));
    QK_TRY(qk_store_bin_mirror(ctx, s, metric));
    if (asym) QK_TRY(qk_store_bin_factors(ctx, s, metric));
    const size_t b_q = asym ? qk_bin_asym_query_bytes(Q, d) : qk_al256((size_t)Q * nbw * 16), b_c = qk_al256((size_t)Q * C * 8), b_s = qk_al256((size_t)Q * 8);
    const size_t b_q8 = rescored ? qk_al256((size_t)Q * nb8 * 64) : 0, b_n8 = rescored ? qk_al256((size_t)Q * 4) : 0,
                 b_c2 = rescored ? qk_al256((size_t)Q * R * 8) : 0;
    QK_TRY(qk_fn_reserve(ctx, b_q + b_c + b_s + b_q8 + b_n8 + b_c2));
    uint4 *xq = (uint4 *)ctx->fn_buf;
    int64_t *cand = (int64_t *)(ctx->fn_buf + b_q);
    uint2 *stat = (uint2 *)(ctx->fn_buf + b_q + b_c);
    uint4 *xq8 = (uint4 *)(ctx->fn_buf + b_q + b_c + b_s);
    int32_t *nq8 = (int32_t *)(ctx->fn_buf + b_q + b_c + b_s + b_q8);
    int64_t *cand2 = (int64_t *)(ctx->fn_buf + b_q + b_c + b_s + b_q8 + b_n8);
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
    char *qf = !asym ? nullptr : (char *)xq + qk_al256((size_t)Q * nbw * 64);  // (asym: the queries' (lo, delta, sumU) behind their four planes)
    if (asym)
        QK_TRY(qk_launch_bin_prep_asym(st, s, sa.x, Q, metric, xq, qf));
    else if (l2)
        hipLaunchKernelGGL(k_bin_prep<true>, dim3((unsigned)Q), dim3(64), 0, st, sa.x, d, nbw, (const float *)s->bin_m, xq);
    else
        hipLaunchKernelGGL(k_bin_prep<false>, dim3((unsigned)Q), dim3(64), 0, st, sa.x, d, nbw, (const float *)s->bin_m, xq);
    QK_HIP(hipGetLastError());
    if (rescored) QK_TRY(qk_launch_sq8_prep(st, s, sa.x, Q, metric, xq8, nq8));
    // ---- the candidates ---------------------------------------------------------------------------------------------------------------
    if (asym) {
        if (tm) QK_HIP(hipEventRecord(ctx->ev[5], st));
        QK_TRY(qk_launch_bin_select_asym(st, s, sa, metric, xq, qf, C, cand, timing ? stat : nullptr, Q));
        ctx->last_scan_kernel = rescored ? "k_bin_select_asym (sign codes) + k_sq8_rerank (int8 codes)" : "k_bin_select_asym (sign codes)";
    } else {
        BinSelectParams bp;
        bp.codes = (const uint4 *)s->bin_codes;
        bp.pt_off = (const int64_t *)s->d_off;
        bp.pt_size = (const int32_t *)s->d_size;
        bp.npids = (int)s->parts.size();
        bp.pids = sa.all_lists ? nullptr : sa.pids;
        bp.P = sa.all_lists ? bp.npids : sa.P;
        bp.nbw = nbw;
        bp.nbins = d + 1;
        bp.xq = xq;
        bp.C = C;
        bp.cand = cand;
        bp.cache_rows = QK_BIN_KEY_CACHE ? (int)std::min<int64_t>(bin_cache_rows(d), (rows_ub + 7) & ~(int64_t)7) : 0;
        bp.stat = timing ? stat : nullptr;
        if (bp.P < 1 || bp.P > QK_BIN_MAX_NPROBE) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: %d lists per query exceed QK_BIN_MAX_NPROBE=%d", who, bp.P, QK_BIN_MAX_NPROBE);
        const size_t lds = bin_lds_bytes(d, bp.P, bp.cache_rows);
        QK_HIP(hipFuncSetAttribute((const void *)k_bin_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (tm) QK_HIP(hipEventRecord(ctx->ev[5], st));
        hipLaunchKernelGGL(k_bin_select, dim3((unsigned)Q), dim3(256), lds, st, bp);
        QK_HIP(hipGetLastError());
        ctx->last_scan_kernel = rescored ? "k_bin_select (sign codes) + k_sq8_rerank (int8 codes)" : "k_bin_select (sign codes)";
    }
    if (tm) {
        QK_HIP(hipEventRecord(ctx->ev[6], st));
        QK_HIP(hipEventRecord(ctx->ev[7], st));  // (no merge)
    }
    // ---- rescored: the R best of the C candidates on the int8 codes, behind the phase events like the finish -----------------------
    if (rescored) {
        Sq8RerankParams rp;
        rp.cand = cand;
        rp.cand2 = cand2;
        rp.codes = (const uint4 *)s->sq8_codes;
        rp.nx = s->sq8_nx;
        rp.xq = xq8;
        rp.nq = nq8;
        rp.nb8 = nb8;
        rp.C = C;
        rp.R = R;
        rp.metric = metric;
        QK_TRY(qk_launch_sq8_rerank(st, rp, Q));
    }
    // ---- the exact finish: funnel search's, or its sibling for more candidates than that one pools ---------------------------------
    FunnelFinishParams fp;
    fp.cand = rescored ? cand2 : cand;
    fp.xq4 = sa.xq4;
    fp.xn = sa.xn;
    fp.vecs = (const float4 *)s->vecs;
    fp.norms = s->norms;
    fp.ids = s->ids;
    fp.nblk = nblk;
    fp.C = R;
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
            timing->scan_bytes = rows * ((int64_t)nbw * 16 + (asym ? 8 : 0));
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

void qk_store_bin_free(qk_store *s) {
    if (s->bin_codes) hipFree(s->bin_codes);
    if (s->bin_m) hipFree(s->bin_m);
    if (s->bin_stats) hipFree(s->bin_stats);
    s->bin_codes = nullptr;
    s->bin_m = nullptr;
    s->bin_stats = nullptr;
    s->bin_cap_rows = 0;
    s->bin_metric = -1;
    qk_store_bin_fac_free(s);  // (the row factors of the asymmetric form live and die with the centres they were built from)
}

int qk_store_bin_mirror(qk_ctx *ctx, qk_store *s, int metric) {
    if (s->bin_codes && s->bin_metric == metric && s->bin_version == s->version && s->bin_cap_rows >= s->cap_rows) return QK_OK;
    const int d = s->d, nbw = qk_bin_nbw(d), ncol = nbw * 128, nstat = 2 * ncol + 4;
    const bool l2 = metric == QK_METRIC_L2;
    if (s->bin_cap_rows < s->cap_rows || !s->bin_codes) {
        // (all three or none: a call without memory leaves the store as it was)
        const int64_t rows = (std::max<int64_t>(s->cap_rows, 16) + 15) & ~(int64_t)15;
        void *nc = nullptr, *nm = nullptr, *ns = nullptr;
        if (hipMalloc(&nc, (size_t)rows * nbw * 16) != hipSuccess || hipMalloc(&nm, (size_t)ncol * 4) != hipSuccess ||
            hipMalloc(&ns, (size_t)nstat * 4) != hipSuccess) {
            (void)hipGetLastError();
            if (nc) hipFree(nc);
            if (nm) hipFree(nm);
            QK_FAIL(QK_ERR_OOM, "binary search: no device memory for %lld bytes of sign codes", (long long)rows * nbw * 16);
        }
        qk_store_bin_free(s);  // (hipFree waits for the device: an earlier call may still read the old mirror)
        s->bin_codes = nc;
        s->bin_m = (float *)nm;
        s->bin_stats = (uint32_t *)ns;
        s->bin_cap_rows = rows;
    }
    s->bin_metric = -1;
    hipStream_t st = ctx->stream;
    const int64_t nl = (int64_t)s->parts.size();
    const bool rows_live = nl > 0 && s->vecs && s->ntotal > 0;
    const unsigned gy = nl >= 2048 ? 4 : nl >= 256 ? 16 : 64;  // (few lists: more workgroups per list)
    std::vector<float> h_m(ncol, 0.0f);
    if (rows_live && l2) {
        int64_t bad = -1;
        QK_TRY(qk_sq8_l2_centres(ctx, s, s->bin_stats, ncol, h_m.data(), &bad));
        if (bad >= 0)
            QK_FAIL(QK_ERR_UNSUPPORTED, "binary search: list %lld holds a value that is not finite: no L2 sign codes for this store", (long long)bad);
    }
    QK_HIP(hipMemcpyAsync(s->bin_m, h_m.data(), (size_t)ncol * 4, hipMemcpyHostToDevice, st));
    if (rows_live) {
        if (l2)
            hipLaunchKernelGGL(k_bin_encode<true>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, nbw, d,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->bin_m, (uint4 *)s->bin_codes);
        else
            hipLaunchKernelGGL(k_bin_encode<false>, dim3((unsigned)nl, gy), dim3(256), 0, st, (const float4 *)s->vecs, s->nblk, nbw, d,
                               (const int64_t *)s->d_off, (const int32_t *)s->d_size, (const float *)s->bin_m, (uint4 *)s->bin_codes);
        QK_HIP(hipGetLastError());
    }
    QK_HIP(hipStreamSynchronize(st));  // (the one-off build, and h_m: from here on every stream of the device may read the mirror)
    s->bin_metric = metric;
    s->bin_version = s->version;
    return QK_OK;
}

extern "C" {

int qk_bin_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int metric,
                  int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_search: nprobe must be positive");
    return qk_bin_run("qk_bin_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, -1, false, metric, out_ids, out_dist, mem, timing);
}

int qk_bin_search_rescored(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int rescore_k,
                           int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_rescored: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_rescored: nprobe must be positive");
    if (rescore_k < 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_rescored: rescore_k=%d must be at least k=%d", rescore_k, k);
    return qk_bin_run("qk_bin_search_rescored", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, rescore_k, false, metric, out_ids, out_dist, mem, timing);
}

int qk_bin_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int metric,
                int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan: bad partition id list");
    return qk_bin_run("qk_bin_scan", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, -1, false, metric, out_ids, out_dist, mem, timing);
}

int qk_bin_scan_rescored(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int rescore_k,
                         int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_rescored: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_rescored: bad partition id list");
    if (rescore_k < 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_rescored: rescore_k=%d must be at least k=%d", rescore_k, k);
    return qk_bin_run("qk_bin_scan_rescored", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, rescore_k, false, metric, out_ids, out_dist, mem, timing);
}

int qk_bin_search_asym(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int rescore_k,
                       int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_asym: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_asym: nprobe must be positive");
    if (rescore_k < 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_search_asym: rescore_k=%d must be 0 (no int8 stage) or at least k=%d", rescore_k, k);
    return qk_bin_run("qk_bin_search_asym", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, rescore_k > 0 ? rescore_k : -1, true, metric, out_ids,
                      out_dist, mem, timing);
}

int qk_bin_scan_asym(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int rescore_k,
                     int metric, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_asym: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_asym: bad partition id list");
    if (rescore_k < 0) QK_FAIL(QK_ERR_INVALID, "qk_bin_scan_asym: rescore_k=%d must be 0 (no int8 stage) or at least k=%d", rescore_k, k);
    return qk_bin_run("qk_bin_scan_asym", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, rescore_k > 0 ? rescore_k : -1, true, metric, out_ids, out_dist,
                      mem, timing);
}

int qk_store_bin_info(qk_store *s, int *valid, int64_t *bytes, int64_t *cache_rows) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_bin_info: null store");
    // (a store with pending changes has no current mirror: the next call rebuilds it)
    const bool cur = s->bin_codes && s->bin_metric >= 0 && !s->table_dirty && s->bin_version == s->version;
    if (valid) *valid = cur ? 1 : 0;
    if (bytes) *bytes = s->bin_codes ? s->bin_cap_rows * (int64_t)qk_bin_nbw(s->d) * 16 : 0;
    if (cache_rows) *cache_rows = QK_BIN_KEY_CACHE ? bin_cache_rows(s->d) : 0;  // (0: this build has no key cache)
    return QK_OK;
}

int qk_store_bin_drop(qk_store *s) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_bin_drop: null store");
    QK_HIP(hipSetDevice(s->ctx->device));
    QK_HIP(hipDeviceSynchronize());  // (searches of other contexts may be reading it)
    qk_store_bin_free(s);
    return QK_OK;
}

}  // extern "C"
