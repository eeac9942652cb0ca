// qk_sq8_deep.hip -- deep quantized search (include/quake_hip.h, "deep quantized search"): the candidates of quantized
// search -- the fetch_k rows of a query's probed lists with the smallest (integer key, arena row) -- selected by COUNTING instead of
// in LDS pools, for fetch_k up to QK_SQ8_MAX_FETCH.  The keys are exact integers, so a histogram of them is exact whatever the order
// of arrival.  One enqueue on the context's stream, no host wait, no data-dependent memory:
//   (mirror, k_sq8_prep, coarse, grouping: the shipped ones, qk_sq8.hip / qk_scan.hip)
//   k_sq8_bound        one workgroup per query: a strided sample of its probed lists' code tiles, scored with v_dot4_i32_i8 against the
//                      query's codes in LDS; U_q = the fetch_k-th smallest sample key (a subset's order statistic bounds the full
//                      set's), the bin origin = the sample's smallest key, the bin shift
//   k_scan_sq8_deep<PASS 0>  the sq8 scan's body without pools: a key <= U_q adds one to hist[q][bin]
//   k_sq8_cut          one wave per query: prefix sum over the bins -> the cut bin b, c0 = keys in the bins under b (< fetch_k)
//   k_scan_sq8_deep<PASS 1>  the same stream again: bins under b append their row to the query's candidates (exactly c0 slots), bin b
//                      appends (key, row) to the query's contested slice of QK_SQ8_DEEP_CAP entries
//   k_sq8_resolve      one workgroup per query: the fetch_k - c0 smallest contested entries under (key, row) by byte-wise selection --
//                      over the contested slice, or, where bin b holds more rows than the slice, over the query's probed rows
//                      themselves, keys recomputed: the same exact answer from a fixed number of walks
//   k_sq8_deep_finish  funnel search's exact finish for more candidates than its LDS pool holds: the gathered MFMA of k_funnel_finish,
//                      all exact keys in LDS, the k best under (exact key, id) by byte-wise selection (fetch_k <= QK_MAX_K: the shipped
//                      k_funnel_finish itself)
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"
#include "qk_scan_opts.h"

#include <algorithm>
#include <cstring>

namespace {

typedef int qk_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ qk_i32x4 qk_as_i4(const float4 v) { return __builtin_bit_cast(qk_i32x4, v); }

constexpr uint32_t DEEP_TOP = 0xFFFFFFFEu;  // above every key: L2 keys lie under 2^31, IP keys within 2^31 +- 127^2 QK_SQ8_MAX_D
constexpr int DEEP_SAMPLE = 16384;          // most sample keys a query's bound is taken from (64 KiB of LDS)

// what a workgroup needs to score a query's probed rows by itself
struct Sq8Walk {
    const uint4 *codes;
    const int32_t *nx;
    const int64_t *pt_off;
    const int32_t *pt_size;
    int npids;
    const int64_t *pids;                 // [Q][P], or nullptr
    const unsigned long long *packed;    // [Q] (P = 1), or nullptr; both null: list pi is list number pi
    int P, nb8, l2;
    const uint4 *xq;                     // [Q][nb8][4] the queries' codes
    const int32_t *nq;                   // [Q]
};

__device__ __forceinline__ int walk_pid(const Sq8Walk &w, int64_t q, int pi) {
    int64_t p;
    if (w.packed) {
        const unsigned long long v = w.packed[q];
        p = v == ~0ull ? -1 : (int64_t)(v & 0xFFFFFFFFull);
    } else {
        p = w.pids ? w.pids[q * w.P + pi] : pi;
    }
    if (p < 0 || p >= w.npids) return -1;
    return w.pt_size[p] > 0 ? (int)p : -1;
}

// Every `stride`-th tile of every probed list of query q, a wave per tile: lane (r, g) holds the 16 codes of row r, columns
// 64 c8 + 16 g .. + 15, as in the scan; four v_dot4_i32_i8 per block against the query's codes in LDS (one query: an MFMA would spend
// 15 of its 16 columns on nothing), the four column groups folded by two shuffles.  f(valid, key, row) is called by every lane;
// valid in lanes g == 0 whose row lies inside the list.  The key is k_scan_sq8's, bit for bit: both are exact integers.
template <class F>
__device__ __forceinline__ void sq8_walk(const Sq8Walk &w, int64_t q, int stride, const uint4 *s_xq, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int nqv = w.nq[q];
    for (int pi = 0; pi < w.P; pi++) {
        const int p = walk_pid(w, q, pi);
        if (p < 0) continue;
        const int size = w.pt_size[p];
        const int64_t off = w.pt_off[p];
        const int ntl = (size + 15) >> 4;
        for (int64_t t = (int64_t)wave * stride; t < ntl; t += 4 * (int64_t)stride) {
            const int64_t tile = (off >> 4) + t;
            const uint4 *src = w.codes + tile * w.nb8 * 64 + lane;
            int dot = 0;
            for (int c8 = 0; c8 < w.nb8; c8++) {
                const uint4 a = src[(int64_t)c8 * 64], b = s_xq[c8 * 4 + g];
                dot = __builtin_amdgcn_sdot4((int)a.x, (int)b.x, dot, false);
                dot = __builtin_amdgcn_sdot4((int)a.y, (int)b.y, dot, false);
                dot = __builtin_amdgcn_sdot4((int)a.z, (int)b.z, dot, false);
                dot = __builtin_amdgcn_sdot4((int)a.w, (int)b.w, dot, false);
            }
            dot += __shfl_xor(dot, 16);
            dot += __shfl_xor(dot, 32);
            const int row_in = (int)t * 16 + r;
            const bool valid = g == 0 && row_in < size;
            const int64_t row = off + row_in;
            const int nxv = (valid && w.l2) ? w.nx[row] : 0;
            const uint32_t key = w.l2 ? (uint32_t)(nqv + nxv - 2 * dot) : (uint32_t)(-dot) ^ 0x80000000u;
            f(valid, key, row);
        }
    }
}

// The m-th smallest (1-based) of a workgroup's elements under (hi, lo), byte by byte from the top: 4 rounds over hi, lo_bytes over the
// low bytes of lo (the bytes above them are 0 in every element).  each(g) calls g(hi, lo) for this thread's elements, the same set in
// every round; at least m elements exist.  256 threads; s_hist [256], s_pick [2].  Every round counts the digits of the elements that
// match the prefix found so far and descends into the digit that holds the m-th: exact, 4 + lo_bytes passes over the elements.
template <class Each>
__device__ __forceinline__ void wg_select(Each each, uint32_t m, int lo_bytes, uint32_t *s_hist, uint32_t *s_pick, uint32_t &thi, uint64_t &tlo) {
    const int tid = threadIdx.x;
    uint32_t phi = 0;
    uint64_t plo = 0;
    for (int rd = 0; rd < 4 + lo_bytes; rd++) {
        const bool hi_rd = rd < 4;
        const int sh = hi_rd ? 24 - 8 * rd : 8 * (lo_bytes - 1 - (rd - 4));
        __syncthreads();
        s_hist[tid] = 0;
        __syncthreads();
        each([&](uint32_t hi, uint64_t lo) {
            bool match;
            uint32_t dig;
            if (hi_rd) {
                match = ((uint64_t)(hi ^ phi) >> (sh + 8)) == 0;
                dig = (hi >> sh) & 255u;
            } else {
                match = hi == phi && (sh + 8 >= 64 || ((lo ^ plo) >> (sh + 8)) == 0);
                dig = (uint32_t)(lo >> sh) & 255u;
            }
            if (match) atomicAdd(&s_hist[dig], 1u);
        });
        __syncthreads();
        if (tid < 64) {
            const uint32_t c0 = s_hist[4 * tid], c1 = s_hist[4 * tid + 1], c2 = s_hist[4 * tid + 2], c3 = s_hist[4 * tid + 3];
            const uint32_t c = c0 + c1 + c2 + c3;
            uint32_t x = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o);
                if (tid >= o) x += y;
            }
            const uint32_t ex = x - c;
            if (ex < m && m <= x) {  // exactly one lane: the matching elements are at least m
                uint32_t rr = m - ex, dig = 4 * tid;
                if (rr > c0) {
                    rr -= c0, dig++;
                    if (rr > c1) {
                        rr -= c1, dig++;
                        if (rr > c2) rr -= c2, dig++;
                    }
                }
                s_pick[0] = dig;
                s_pick[1] = rr;
            }
        }
        __syncthreads();
        const uint32_t dig = s_pick[0];
        m = s_pick[1];
        if (hi_rd) phi |= dig << sh;
        else plo |= (uint64_t)dig << sh;
    }
    thi = phi;
    tlo = plo;
}

__device__ __forceinline__ uint32_t deep_bin(uint32_t key, uint32_t lo, uint32_t sh) { return key < lo ? 0u : 1u + ((key - lo) >> sh); }

// ---- per-query state before anything else: "no cut, nothing contested" -- what a call without a scan launch resolves ------------------
__global__ void k_sq8_deep_init(uint4 *stt, int64_t Q) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) stt[i] = make_uint4(0u, 0u, (uint32_t)QK_SQ8_DEEP_BINS, 0u);
}

// ---- the bound ----------------------------------------------------------------------------------------------------------------------
// blockIdx.x = query, 256 threads.  Dynamic LDS: the query's codes [nb8 * 4] uint4 | sample keys [DEEP_SAMPLE].  The stride aims at
// max(4 fetch_k, 1024) sample rows, spread over every probed list (lists are not shuffled: their heads are no sample); a sample that
// outgrows the buffer is cut where it is full -- any subset gives a true bound.  Also clears the query's histogram.
__global__ __launch_bounds__(256) void k_sq8_bound(Sq8Walk w, int C, uint4 *qst, uint32_t *hist) {
    extern __shared__ uint4 bd_lds[];
    __shared__ uint32_t s_hist[256], s_pick[2], s_n, s_min;
    __shared__ unsigned long long s_rows;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    uint4 *s_xq = bd_lds;
    uint32_t *s_keys = (uint32_t *)(bd_lds + w.nb8 * 4);
    for (int i = tid; i < QK_SQ8_DEEP_BINS; i += 256) hist[q * QK_SQ8_DEEP_BINS + i] = 0u;
    for (int i = tid; i < w.nb8 * 4; i += 256) s_xq[i] = w.xq[q * w.nb8 * 4 + i];
    if (tid == 0) {
        s_n = 0u;
        s_min = 0xFFFFFFFFu;
        s_rows = 0ull;
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int pi = tid; pi < w.P; pi += 256) {
        const int p = walk_pid(w, q, pi);
        if (p >= 0) mine += (unsigned long long)w.pt_size[p];
    }
    if (mine) atomicAdd(&s_rows, mine);
    __syncthreads();
    const unsigned long long target = (unsigned long long)min(DEEP_SAMPLE, max(4 * C, 1024));
    // (from the probed ROWS, not tiles: short lists, whose last tiles are mostly padding, still give about `target` sample rows)
    const int stride = (int)min(1ull << 20, max(1ull, s_rows / target));
    sq8_walk(w, q, stride, s_xq, [&](bool valid, uint32_t key, int64_t) {
        if (!valid) return;
        const uint32_t slot = atomicAdd(&s_n, 1u);
        if (slot < (uint32_t)DEEP_SAMPLE) {
            s_keys[slot] = key;
            atomicMin(&s_min, key);
        }
    });
    __syncthreads();
    const int n = (int)min(s_n, (uint32_t)DEEP_SAMPLE);
    uint32_t U = DEEP_TOP;
    if (n >= C) {
        uint64_t unused;
        wg_select([&](auto g) { for (int i = tid; i < n; i += 256) g(s_keys[i], 0ull); }, (uint32_t)C, 0, s_hist, s_pick, U, unused);
    }
    if (tid == 0) {
        const uint32_t lo = n > 0 ? s_min : 0u;
        uint32_t sh = 0;
        while (((U - lo) >> sh) > (uint32_t)(QK_SQ8_DEEP_BINS - 2)) sh++;
        qst[q] = make_uint4(U, lo, sh, 0u);
    }
}

// ---- the cut ------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = query, one wave; lane l owns bins 16 l .. 16 l + 15.  stt[q] = {c0, keys in the cut bin, cut bin, -}; a query with fewer
// than fetch_k counted keys (U_q at the top of the range: every probed row was counted) has no cut: bin number QK_SQ8_DEEP_BINS.
__global__ __launch_bounds__(64) void k_sq8_cut(const uint32_t *__restrict__ hist, int C, uint4 *qst, uint4 *stt, uint32_t *cur) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t *h = hist + q * QK_SQ8_DEEP_BINS + 16 * lane;
    uint32_t c[16], sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        c[i] = h[i];
        sum += c[i];
    }
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    const uint32_t total = __shfl(x, 63);
    if (lane < 2) cur[2 * q + lane] = 0u;
    if (total < (uint32_t)C) {
        if (lane == 0) {
            stt[q] = make_uint4(total, 0u, (uint32_t)QK_SQ8_DEEP_BINS, 0u);
            qst[q].w = (uint32_t)QK_SQ8_DEEP_BINS;
        }
        return;
    }
    uint32_t ex = x - sum;
    if (ex < (uint32_t)C && (uint32_t)C <= x) {
        int b = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (ex + c[i] < (uint32_t)C && b == i) {
                ex += c[i];
                b = i + 1;
            }
        }
        uint32_t nb = 0;
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (i == b) nb = c[i];
        stt[q] = make_uint4(ex, nb, (uint32_t)(16 * lane + b), 0u);
        qst[q].w = (uint32_t)(16 * lane + b);
    }
}

// ---- the two passes -----------------------------------------------------------------------------------------------------------------
template <int DB, bool L2, int PASS>
__global__ __launch_bounds__(256) void k_scan_sq8_deep(ScanParams P) {
    constexpr int MODE = 0;
    constexpr int MAXCH = 1;
#define QK_SCAN_FILT 0
#define QK_SCAN_SQ8
#define QK_SCAN_SQ8_DEEP
#include "qk_scan_body.inc"
#undef QK_SCAN_SQ8_DEEP
#undef QK_SCAN_SQ8
#undef QK_SCAN_FILT
}

template <int DB, int PASS>
int launch_pass(dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_sq8_deep<DB, true, PASS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_sq8_deep<DB, true, PASS>), grid, block, lds, st, sp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_sq8_deep<DB, false, PASS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_sq8_deep<DB, false, PASS>), grid, block, lds, st, sp);
    }
    QK_HIP(hipGetLastError());
    return QK_OK;
}
template <int PASS>
int launch_pass_db(int db, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (db == 1) return launch_pass<1, PASS>(grid, block, lds, st, sp);
    if (db == 2) return launch_pass<2, PASS>(grid, block, lds, st, sp);
    if (db == 4) return launch_pass<4, PASS>(grid, block, lds, st, sp);
    if (db == 8) return launch_pass<8, PASS>(grid, block, lds, st, sp);
    QK_FAIL(QK_ERR_UNSUPPORTED, "no counting int8 code scan kernel for DB=%d", db);
}

// ---- the resolve ----------------------------------------------------------------------------------------------------------------------
// blockIdx.x = query, 256 threads; dynamic LDS: the query's codes (the walk's).  m = fetch_k - c0 of the nb keys of the cut bin are
// still to be chosen: the m smallest under (key, row).  nb <= QK_SQ8_DEEP_CAP: they all lie in the contested slice.  More: the slice
// holds an arbitrary part of them, so the elements are the query's probed rows themselves -- every row whose key falls into the cut
// bin, keys recomputed by sq8_walk.  Either way wg_select finds the m-th smallest (key, row) in 4 + 5 counting passes and one more
// pass appends the elements at or under it: (key, row) pairs are distinct, so exactly m.  Terminates after a fixed number of passes
// whatever the data; a store of identical rows ends with the m smallest arena rows.
__global__ __launch_bounds__(256) void k_sq8_resolve(Sq8Walk w, Sq8DeepParams dp) {
    extern __shared__ uint4 rs_lds[];
    __shared__ uint32_t s_hist[256], s_pick[2], s_out;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int C = dp.C;
    const uint4 stt = dp.stt[q];
    const uint32_t c0 = min(stt.x, (uint32_t)C), nb = stt.y, cut = stt.z;
    const uint32_t m = cut >= (uint32_t)QK_SQ8_DEEP_BINS ? 0u : min((uint32_t)C - c0, nb);
    int64_t *cand = dp.cand + q * C;
    if (tid == 0) s_out = 0u;
    if (m > 0) {
        const uint32_t *ckey = dp.ckey + q * QK_SQ8_DEEP_CAP;
        const int64_t *crow = dp.crow + q * QK_SQ8_DEEP_CAP;
        auto take = [&](uint32_t thi, uint64_t tlo, uint32_t hi, uint64_t lo) {
            if (hi < thi || (hi == thi && lo <= tlo)) {
                const uint32_t slot = atomicAdd(&s_out, 1u);
                if (slot < m) cand[c0 + slot] = (int64_t)lo;
            }
        };
        uint32_t thi = 0xFFFFFFFFu;
        uint64_t tlo = ~0ull;
        if (nb <= (uint32_t)QK_SQ8_DEEP_CAP) {
            auto each = [&](auto g) { for (uint32_t i = tid; i < nb; i += 256) g(ckey[i], (uint64_t)crow[i]); };
            if (m < nb) wg_select(each, m, 5, s_hist, s_pick, thi, tlo);
            __syncthreads();
            each([&](uint32_t hi, uint64_t lo) { take(thi, tlo, hi, lo); });
        } else {
            const uint4 qs = dp.qst[q];
            for (int i = tid; i < w.nb8 * 4; i += 256) rs_lds[i] = w.xq[q * w.nb8 * 4 + i];
            __syncthreads();
            auto each = [&](auto g) {
                sq8_walk(w, q, 1, rs_lds, [&](bool valid, uint32_t key, int64_t row) {
                    if (valid && key <= qs.x && deep_bin(key, qs.y, qs.z) == cut) g(key, (uint64_t)row);
                });
            };
            if (m < nb) wg_select(each, m, 5, s_hist, s_pick, thi, tlo);
            __syncthreads();
            each([&](uint32_t hi, uint64_t lo) { take(thi, tlo, hi, lo); });
        }
    }
    // behind the candidates: -1, as the pool form's merge pads
    for (uint32_t i = c0 + m + tid; i < (uint32_t)C; i += 256) cand[i] = -1;
}

// ---- the exact finish for fetch_k > QK_MAX_K ----------------------------------------------------------------------------------------
// k_funnel_finish's gather (qk_funnel.hip: the canonical chain x, y, z, w of every block in ascending order, so the key is the one
// the scan computes for the pair) with a pool of C entries, then the k best under (exact key, id) by wg_select -- ids are compared as
// signed integers: their sign bit is flipped -- and k_funnel_finish's ordered write of the row through compact_pool.
// Dynamic LDS: [nblk * 4] float4 query | [C] int64 ids | [512] int64 | [C] uint32 keys | [512] uint32.
constexpr int DF_U = 4;
__global__ __launch_bounds__(256) void k_sq8_deep_finish(FunnelFinishParams F) {
    extern __shared__ float4 df_lds4[];
    __shared__ uint32_t s_hist[256], s_pick[2];
    __shared__ int s_cnt, s_sel;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nblk = F.nblk, C = F.C, k = F.k;
    const int64_t q = blockIdx.x;
    const bool l2 = F.metric == QK_METRIC_L2;
    float4 *qs = df_lds4;
    int64_t *big_id = (int64_t *)(df_lds4 + (size_t)nblk * 4);
    int64_t *pool_id = big_id + C;
    uint32_t *big_ord = (uint32_t *)(pool_id + 512);
    uint32_t *pool_ord = big_ord + C;
    for (int t = tid; t < nblk * 4; t += 256) qs[t] = F.xq4[q * nblk * 4 + t];
    if (tid == 0) {
        s_cnt = 0;
        s_sel = 0;
    }
    const float xnq = l2 ? F.xn[q] : 0.f;
    __syncthreads();
    for (int b0 = wave * 16; b0 < C; b0 += 64) {
        const int ci = b0 + r;
        const int64_t row = ci < C ? F.cand[q * C + ci] : -1;
        if (__ballot(row >= 0) == 0) continue;  // (padding only: nothing to gather; uniform)
        const int64_t rs = row >= 0 ? row : 0;
        const float4 *base = F.vecs + ((rs >> 4) * nblk) * 64 + 16 * g + (rs & 15);
        float4 a0[DF_U], a1[DF_U];
#define DF_LOAD(A, C0)                                                                       \
    _Pragma("unroll") for (int u_ = 0; u_ < DF_U; u_++) A[u_] = base[(int64_t)min((C0) + u_, nblk - 1) * 64];
#define DF_STEP(A, C0)                                                                       \
    _Pragma("unroll") for (int u_ = 0; u_ < DF_U; u_++) if ((C0) + u_ < nblk) {              \
        const float4 bq_ = qs[((C0) + u_) * 4 + g];                                          \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].x, bq_.x, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].y, bq_.y, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].z, bq_.z, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u_].w, bq_.w, acc, 0, 0, 0);            \
    }
        DF_LOAD(a0, 0)
        const float nrm_r = F.norms[rs];
        const int64_t id_r = F.ids[rs];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < nblk; c0 += 2 * DF_U) {
            DF_LOAD(a1, c0 + DF_U)
            DF_STEP(a0, c0)
            DF_LOAD(a0, c0 + 2 * DF_U)
            DF_STEP(a1, c0 + DF_U)
        }
#undef DF_LOAD
#undef DF_STEP
        const int src = 4 * g + (r & 3);
        const float nrm = __shfl(nrm_r, src, 64);
        const int64_t id = __shfl(id_r, src, 64);
        const int64_t row_o = __shfl(row, src, 64);
        const float v = (r & 3) == 0 ? acc[0] : (r & 3) == 1 ? acc[1] : (r & 3) == 2 ? acc[2] : acc[3];
        const uint32_t o = l2 ? ord_from_l2(l2_expanded(xnq, nrm, v)) : ord_from_ip(v);
        if (r < 4 && row_o >= 0 && o != 0xFFFFFFFFu) {
            const int slot = atomicAdd(&s_cnt, 1);  // (at most C; the order of arrival does not reach the result)
            big_ord[slot] = o;
            big_id[slot] = id;
        }
    }
    __syncthreads();
    const int n = s_cnt;
    constexpr uint64_t SIGN = 0x8000000000000000ull;
    uint32_t thi = 0xFFFFFFFFu;
    uint64_t tlo = ~0ull;
    auto each = [&](auto f) { for (int i = tid; i < n; i += 256) f(big_ord[i], (uint64_t)big_id[i] ^ SIGN); };
    if (n > k) wg_select(each, (uint32_t)k, 8, s_hist, s_pick, thi, tlo);
    __syncthreads();
    each([&](uint32_t hi, uint64_t lo) {
        if (hi < thi || (hi == thi && lo <= tlo)) {
            const int slot = atomicAdd(&s_sel, 1);
            if (slot < 512) {  // (exactly min(n, k) <= QK_MAX_K where ids are distinct)
                pool_ord[slot] = hi;
                pool_id[slot] = (int64_t)(lo ^ SIGN);
            }
        }
    });
    __syncthreads();
    if (wave != 0) return;
    const int cnt = compact_pool<8>(pool_ord, pool_id, min(s_sel, 512), k, lane);
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

Sq8Walk make_walk(qk_store *s, const qk_scan_args &a) {
    Sq8Walk w;
    w.codes = (const uint4 *)a.sq8_codes;
    w.nx = a.sq8_nx;
    w.pt_off = (const int64_t *)s->d_off;
    w.pt_size = (const int32_t *)s->d_size;
    w.npids = (int)s->parts.size();
    w.pids = a.all_lists ? nullptr : a.pids;
    w.packed = a.all_lists ? nullptr : a.pids_packed;
    w.P = a.all_lists ? w.npids : a.P;
    w.nb8 = a.sq8_nblk;
    w.l2 = a.metric == QK_METRIC_L2 ? 1 : 0;
    w.xq = (const uint4 *)a.xq4;
    w.nq = (const int32_t *)a.xn;
    return w;
}

}  // namespace

size_t qk_sq8_deep_bytes(int64_t Q, int fetch_k) {
    return qk_al256((size_t)Q * fetch_k * 8) + qk_al256((size_t)Q * QK_SQ8_DEEP_CAP * 8) + qk_al256((size_t)Q * QK_SQ8_DEEP_CAP * 4) +
           qk_al256((size_t)Q * QK_SQ8_DEEP_BINS * 4) + 2 * qk_al256((size_t)Q * 16) + qk_al256((size_t)Q * 8);
}

void qk_sq8_deep_carve(char *buf, int64_t Q, int fetch_k, Sq8DeepParams *dp) {
    dp->C = fetch_k;
    dp->cand = (int64_t *)buf;
    buf += qk_al256((size_t)Q * fetch_k * 8);
    dp->crow = (int64_t *)buf;
    buf += qk_al256((size_t)Q * QK_SQ8_DEEP_CAP * 8);
    dp->ckey = (uint32_t *)buf;
    buf += qk_al256((size_t)Q * QK_SQ8_DEEP_CAP * 4);
    dp->hist = (uint32_t *)buf;
    buf += qk_al256((size_t)Q * QK_SQ8_DEEP_BINS * 4);
    dp->qst = (uint4 *)buf;
    buf += qk_al256((size_t)Q * 16);
    dp->stt = (uint4 *)buf;
    buf += qk_al256((size_t)Q * 16);
    dp->cur = (uint32_t *)buf;
}

int qk_launch_sq8_deep_init(hipStream_t st, const Sq8DeepParams &dp, int64_t Q) {
    hipLaunchKernelGGL(k_sq8_deep_init, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, dp.stt, Q);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

int qk_launch_scan_sq8_deep(qk_store *s, const qk_scan_args &a, int db, dim3 grid, dim3 block, size_t lds, hipStream_t st, ScanParams &sp) {
    const Sq8DeepParams &dp = *a.sq8_deep;
    const Sq8Walk w = make_walk(s, a);
    const int64_t Q = a.Q;
    sp.dp = dp;
    sp.dyn_counter = nullptr;  // (both passes walk the static cut: a dynamic tail's counter, drained by pass A, would leave pass B without it)
    const size_t lds_b = (size_t)w.nb8 * 64 + (size_t)DEEP_SAMPLE * 4;
    QK_HIP(hipFuncSetAttribute((const void *)k_sq8_bound, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL(k_sq8_bound, dim3((unsigned)Q), dim3(256), lds_b, st, w, dp.C, dp.qst, dp.hist);
    QK_HIP(hipGetLastError());
    QK_TRY(launch_pass_db<0>(db, grid, block, lds, st, sp));
    hipLaunchKernelGGL(k_sq8_cut, dim3((unsigned)Q), dim3(64), 0, st, (const uint32_t *)dp.hist, dp.C, dp.qst, dp.stt, dp.cur);
    QK_HIP(hipGetLastError());
    return launch_pass_db<1>(db, grid, block, lds, st, sp);
}

int qk_launch_sq8_resolve(qk_store *s, const qk_scan_args &a, hipStream_t st) {
    const Sq8Walk w = make_walk(s, a);
    hipLaunchKernelGGL(k_sq8_resolve, dim3((unsigned)a.Q), dim3(256), (size_t)w.nb8 * 64, st, w, *a.sq8_deep);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

int qk_launch_sq8_deep_finish(hipStream_t st, const FunnelFinishParams &fp, int64_t Q) {
    if (fp.C <= QK_MAX_K) return qk_launch_funnel_finish(st, fp, Q);
    const size_t lds = (size_t)fp.nblk * 64 + (size_t)(fp.C + 512) * 12;
    QK_HIP(hipFuncSetAttribute((const void *)k_sq8_deep_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_sq8_deep_finish, dim3((unsigned)Q), dim3(256), lds, st, fp);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

extern "C" {

int qk_sq8_search_deep(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k, int metric,
                       int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_sq8_search_deep: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_sq8_search_deep: nprobe must be positive");
    return qk_sq8_run("qk_sq8_search_deep", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, fetch_k, metric, out_ids, out_dist, mem, timing, true);
}

int qk_sq8_scan_deep(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k, int metric,
                     int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_sq8_scan_deep: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_sq8_scan_deep: bad partition id list");
    return qk_sq8_run("qk_sq8_scan_deep", ctx, nullptr, s, x, Q, pids, P, 0, k, fetch_k, metric, out_ids, out_dist, mem, timing, true);
}

}  // extern "C"
