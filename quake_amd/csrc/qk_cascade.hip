// qk_cascade.hip -- the middle stage of rescored binary search (include/quake_hip.h, "binary search, rescored"): the
// shortlist that k_bin_select ranked by Hamming distance is re-ranked on the store's int8 codes, and only the rescore_k best of it
// reach the exact finish, whose gather of float32 rows is what such a call pays for.
//   k_sq8_rerank       one workgroup per query, no global atomics: the query's code tile in LDS, the candidates' integer keys by a
//                      gather of their code rows (16 candidates per wave and step, v_dot4_i32_i8), the keys in LDS by candidate
//                      position, the rescore_k-th key by byte-wise selection, an ordered ballot compaction into cand2
// Every number in this file is an integer: no float chain, no per-source build flags.
#include "qk_internal.h"

#include "qk_device.h"
#include "qk_scan_types.h"

namespace {

constexpr int RR_U = 4;  // code blocks per load group: two groups of 4 x 16 B per lane in flight
constexpr int RR_V = 4;  // positions per thread and compaction step: 1024 candidates between two barriers

// blockIdx.x = query, 256 threads.  Dynamic LDS: [nb8 * 4] uint4 query codes | [C] uint32 keys.
//   1. the query's codes (k_sq8_prep's tile, entry (c, g) = the 16 codes of columns 64 c + 16 g ..) and n, the number of candidates:
//      cand[q] holds ascending arena rows and -1 behind them.
//   2. keys: a wave takes candidates b0 .. b0 + 15; lane (r, g) gathers, for every code block c, the 16 bytes of candidate r at
//      (tile_r nb8 + c) 64 + 16 g + (row_r & 15) -- k_sq8_encode's layout, so the piece lies against entry (c, g) of the query.
//      The addresses of all blocks are known from the row alone: RR_U loads are issued before the first is used and the next
//      group is issued before this one is consumed (k_funnel_finish's pipeline).  Four v_dot4_i32_i8 per block, two shuffles fold
//      the lane groups, lane group 0 adds nx and nq (L2) and stores the scan's uint32 image of the key at the candidate's position.
//      Candidates are in arena order, so the 16 of a step share tiles and lines where the shortlist is dense.
//   3. the cut: n > R -> the R-th smallest key by four rounds of 256 bins over the LDS keys, each descending into the digit that
//      holds it; `need` = how many keys equal to the cut are still to be taken.
//   4. compaction, k_bin_select's pass B over positions: every key under the cut and the first `need` at it, in position order --
//      which is arena order, the tie rule of the definition -- land in cand2[q]; -1 behind them.
template <bool L2>
__global__ __launch_bounds__(256) void k_sq8_rerank(Sq8RerankParams P) {
    extern __shared__ uint4 rr_lds[];
    __shared__ uint32_t s_hist[256], s_pick[2];
    __shared__ uint2 s_cnt[2][4 * RR_V];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nb8 = P.nb8, C = P.C, R = P.R;
    const int64_t q = blockIdx.x;
    uint4 *s_q = rr_lds;
    uint32_t *s_key = (uint32_t *)(rr_lds + (size_t)nb8 * 4);
    const int64_t *cand = P.cand + q * C;
    int64_t *cand2 = P.cand2 + q * R;
    // ---- 1. the query, the number of candidates
    for (int t = tid; t < nb8 * 4; t += 256) s_q[t] = P.xq[q * nb8 * 4 + t];
    if (tid == 0) s_n = 0;
    __syncthreads();
    {
        int c = 0;
        for (int i = tid; i < C; i += 256) c += cand[i] >= 0 ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0 && c > 0) atomicAdd(&s_n, c);
    }
    __syncthreads();
    const int n = s_n;
    const int nqv = L2 ? P.nq[q] : 0;
    // ---- 2. the keys
    for (int b0 = wave * 16; b0 < n; b0 += 64) {
        const int64_t row = cand[min(b0 + r, n - 1)];
        const int64_t rs = row >= 0 ? row : 0;  // (never taken while -1 stands behind the candidates only)
        const uint4 *base = P.codes + ((rs >> 4) * nb8) * 64 + 16 * g + (rs & 15);
        uint4 a0[RR_U], a1[RR_U];
#define RR_LOAD(A, C0) \
    _Pragma("unroll") for (int u_ = 0; u_ < RR_U; u_++) A[u_] = base[(int64_t)min((C0) + u_, nb8 - 1) * 64];
#define RR_STEP(A, C0)                                                          \
    _Pragma("unroll") for (int u_ = 0; u_ < RR_U; u_++) if ((C0) + u_ < nb8) {  \
        const uint4 bq_ = s_q[((C0) + u_) * 4 + g];                             \
        dot = __builtin_amdgcn_sdot4((int)A[u_].x, (int)bq_.x, dot, false);     \
        dot = __builtin_amdgcn_sdot4((int)A[u_].y, (int)bq_.y, dot, false);     \
        dot = __builtin_amdgcn_sdot4((int)A[u_].z, (int)bq_.z, dot, false);     \
        dot = __builtin_amdgcn_sdot4((int)A[u_].w, (int)bq_.w, dot, false);     \
    }
        RR_LOAD(a0, 0)
        const int nxv = L2 ? P.nx[rs] : 0;
        int dot = 0;
        for (int c0 = 0; c0 < nb8; c0 += 2 * RR_U) {
            RR_LOAD(a1, c0 + RR_U)
            RR_STEP(a0, c0)
            RR_LOAD(a0, c0 + 2 * RR_U)
            RR_STEP(a1, c0 + RR_U)
        }
#undef RR_LOAD
#undef RR_STEP
        dot += __shfl_xor(dot, 16);
        dot += __shfl_xor(dot, 32);
        // the exact integer key as the code scan forms it: nq + nx - 2 dot in [0, 2^31), or -dot moved into the unsigned range
        const uint32_t key = L2 ? (uint32_t)(nqv + nxv - 2 * dot) : (uint32_t)(-dot) ^ 0x80000000u;
        if (g == 0 && b0 + r < n) s_key[b0 + r] = key;
    }
    __syncthreads();
    const uint32_t target = (uint32_t)min(n, R);
    // ---- 3. the cut
    uint32_t cut = 0xFFFFFFFFu, need = 0;  // (no key reaches 0xFFFFFFFF: without a cut every candidate lies under it)
    if (n > R) {
        uint32_t prefix = 0, rem = (uint32_t)R;
        for (int rd = 0; rd < 4; rd++) {
            const int sh = 24 - 8 * rd;
            s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                const uint32_t key = s_key[i];
                if ((((uint64_t)(key ^ prefix)) >> (sh + 8)) == 0) atomicAdd(&s_hist[(key >> sh) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {  // lane l owns digits 4 l .. 4 l + 3
                const uint32_t c0 = s_hist[4 * tid], c1 = s_hist[4 * tid + 1], c2 = s_hist[4 * tid + 2], c3 = s_hist[4 * tid + 3];
                const uint32_t c = c0 + c1 + c2 + c3;
                uint32_t x = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(x, o);
                    if (tid >= o) x += y;
                }
                const uint32_t ex = x - c;
                if (ex < rem && rem <= x) {  // exactly one lane: the keys that match the prefix are at least rem
                    uint32_t rr = rem - ex, dig = 4 * tid;
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
            prefix |= s_pick[0] << sh;
            rem = s_pick[1];
        }
        cut = prefix;
        need = rem;  // (of the keys equal to the cut, the R-th smallest key is the rem-th: 1 <= rem)
    }
    // ---- 4. the compaction
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run_t = 0, run_e = 0;  // candidates taken / ties seen so far: the same in every thread
    int par = 0;
    for (int s0 = 0; s0 < n && run_t < target; s0 += 256 * RR_V) {
        unsigned long long bl[RR_V], bt[RR_V];
#pragma unroll
        for (int u = 0; u < RR_V; u++) {
            const int i = s0 + 256 * u + tid;
            const bool valid = i < n;
            const uint32_t key = valid ? s_key[i] : 0u;
            bl[u] = __ballot(valid && key < cut);
            bt[u] = __ballot(valid && key == cut);
            if (lane == 0) s_cnt[par][4 * u + wave] = make_uint2((uint32_t)__popcll(bl[u]), (uint32_t)__popcll(bt[u]));
        }
        __syncthreads();
        uint32_t base_t[RR_V], base_e[RR_V];
#pragma unroll
        for (int e = 0; e < 4 * RR_V; e++) {
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
        for (int u = 0; u < RR_V; u++) {
            const int i = s0 + 256 * u + tid;
            const uint32_t left = need - min(base_e[u], need);  // ties this wave's ballot may still take
            const uint32_t lb = (uint32_t)__popcll(bl[u] & below), tb = (uint32_t)__popcll(bt[u] & below);
            const bool less = (bl[u] >> lane) & 1ull, tie = (bt[u] >> lane) & 1ull;
            const uint32_t slot = base_t[u] + lb + min(tb, left);
            if ((less || (tie && tb < left)) && slot < target) cand2[slot] = cand[i];
        }
    }
    for (uint32_t i = target + tid; i < (uint32_t)R; i += 256) cand2[i] = -1;
}

}  // namespace

int qk_launch_sq8_rerank(hipStream_t st, const Sq8RerankParams &rp, int64_t Q) {
    if (rp.nb8 < 1 || rp.nb8 * 64 > QK_SQ8_MAX_D || rp.R < 1 || rp.R > rp.C || rp.C > QK_BIN_MAX_FETCH)
        QK_FAIL(QK_ERR_INVALID, "k_sq8_rerank: nb8=%d, fetch_k=%d, rescore_k=%d lie outside what the kernel's LDS is laid out for", rp.nb8, rp.C, rp.R);
    const size_t lds = (size_t)rp.nb8 * 64 + (size_t)rp.C * 4;  // (at most 2 + 16 KiB)
    if (rp.metric == QK_METRIC_L2)
        hipLaunchKernelGGL(k_sq8_rerank<true>, dim3((unsigned)Q), dim3(256), lds, st, rp);
    else
        hipLaunchKernelGGL(k_sq8_rerank<false>, dim3((unsigned)Q), dim3(256), lds, st, rp);
    QK_HIP(hipGetLastError());
    return QK_OK;
}
