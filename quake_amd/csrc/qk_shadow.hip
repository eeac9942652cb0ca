// qk_shadow.hip -- the fp16 shadow form of the single-probe scan (include/quake_hip.h, qk_ctx_set_shadow).
//
// At nprobe 1 the tile form streams every probed list once and sits at the HBM ceiling: the only lever left is bytes per row.
// The store keeps an fp16 mirror of its arena in the same tile indexing (k_shadow_convert); k_scan_shadow is the tile form's body
// compiled once more over it (qk_scan_body.inc, QK_SCAN_SHADOW): half the bytes per row, one v_mfma_f32_16x16x32_f16 per 32
// columns, no id loads.  Its keys are approximate, so it only SELECTS: every segment leaves the k' = 32 best approximate keys per
// query with their arena rows.  k_shadow_finish, one wave per query in the merge's place, recomputes the canonical fp32 key of
// every candidate that can belong to the answer, proves from the error bound E (qk_shadow_bound.h) that no dropped row can, and
// answers a query it cannot prove by an exact scan of its list.  Every reported id and distance comes from the canonical chain:
// the same bits as the other forms.  No workgroup waits for another one anywhere here: plain grids.
#include "qk_internal.h"
#include "qk_device.h"
#include "qk_scan_types.h"
#include "qk_scan_opts.h"
#include "qk_shadow_bound.h"

#include <algorithm>
#include <vector>

typedef _Float16 qk_h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ qk_h8 qk_as_h8(const float4 v) { return __builtin_bit_cast(qk_h8, v); }

// fp16 image of x (round to nearest even) and the distance from x to it -- to the farther of the image and zero where the image is
// subnormal: the bound must hold whether or not the matrix unit flushes such inputs
__device__ __forceinline__ uint32_t qk_h_bits(float x, float &err, float &himg) {
    const _Float16 h = (_Float16)x;
    const float hf = (float)h;
    float e = fabsf(x - hf);
    if (hf != 0.0f && fabsf(hf) < 6.103515625e-05f) e = fmaxf(e, fabsf(x));
    err = e;
    himg = hf;
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}

// a bound (integer key, smaller = better) moved by E towards "worse", rounded outwards; 0xFFFFFFFF (none) stays
__device__ __forceinline__ uint32_t qk_ord_widen(uint32_t ord, float E, bool l2) {
    if (ord == 0xFFFFFFFFu) return ord;
    // (round to nearest, then one step outwards)
    if (l2) return ord_from_l2(nextafterf(__uint_as_float(ord) + E, INFINITY));
    return ord_from_ip(nextafterf(ip_from_ord(ord) - E, -INFINITY));
}

// ---- the shadow: fp32 arena -> fp16 mirror ----------------------------------------------------------------------------------------
// Arena block c of a tile is 64 lanes x float4: lane (g, r) holds columns 16c + 4t + g (t = 0..3) of row r.  Shadow block b of the
// tile is 64 lanes x 16 B: the lane's float4 of arena blocks 2b and 2b + 1, element by element in fp16 -- eight halves, the lane's
// share of the K = 32 operand of v_mfma_f32_16x16x32_f16 (the queries are laid out with the same mapping, so the product sums the
// same 32 columns).  An odd block count is padded with a zero block.  Workgroup (p, y): the tiles of list p, a wave each.
__global__ __launch_bounds__(256) void k_shadow_convert(const float4 *__restrict__ vecs, int nblk, const int64_t *__restrict__ pt_off,
                                                        const int32_t *__restrict__ pt_size, uint4 *__restrict__ shadow,
                                                        uint32_t *__restrict__ stats) {
    const int size = pt_size[blockIdx.x];
    if (size <= 0) return;
    const int64_t row_off = pt_off[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nbs = (nblk + 1) >> 1;
    const int ntl = (size + 15) >> 4;
    float m_err = 0.0f, m_nrm = 0.0f;
    uint32_t bad = 0;
    for (int t = (int)blockIdx.y * 4 + wv; t < ntl; t += 4 * (int)gridDim.y) {
        const int64_t tile = (row_off >> 4) + t;
        float e2 = 0.0f, n2 = 0.0f;
        uint32_t tb = 0;
        for (int b = 0; b < nbs; b++) {
            const float4 a0 = vecs[(tile * nblk + 2 * b) * 64 + lane];
            const float4 a1 = 2 * b + 1 < nblk ? vecs[(tile * nblk + 2 * b + 1) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            uint32_t hb[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float e, hf;
                hb[i] = qk_h_bits(v[i], e, hf);
                e2 = __fmaf_rn(e, e, e2);
                n2 = __fmaf_rn(hf, hf, n2);
                tb |= fabsf(v[i]) <= 65504.0f ? 0u : 1u;  // (NaN: not <=)
            }
            shadow[(tile * nbs + b) * 64 + lane] = make_uint4(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16));
        }
        // the four lanes (g = 0..3) of a row hold its columns between them
        e2 += __shfl_xor(e2, 16);
        e2 += __shfl_xor(e2, 32);
        n2 += __shfl_xor(n2, 16);
        n2 += __shfl_xor(n2, 32);
        if (t * 16 + (lane & 15) < size) {  // rows behind the list's end are never candidates
            m_err = fmaxf(m_err, e2);
            m_nrm = fmaxf(m_nrm, n2);
            bad |= tb;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m_err = fmaxf(m_err, __shfl_xor(m_err, o));
        m_nrm = fmaxf(m_nrm, __shfl_xor(m_nrm, o));
    }
    const bool anybad = __ballot(bad != 0) != 0;
    if (lane == 0) {  // (non-negative floats order like their bit patterns)
        atomicMax(&stats[0], __float_as_uint(m_err));
        atomicMax(&stats[1], __float_as_uint(m_nrm));
        if (anybad) atomicOr(&stats[2], 1u);
    }
}

int qk_launch_shadow_convert(hipStream_t st, const float4 *vecs, int nblk, const int64_t *pt_off, const int32_t *pt_size, int npids, void *shadow,
                             uint32_t *stats) {
    if (npids <= 0) return QK_OK;
    // (few lists: more workgroups per list, so that a flat store is not converted by four waves)
    const int gy = npids >= 2048 ? 4 : npids >= 256 ? 16 : 256;
    hipLaunchKernelGGL(k_shadow_convert, dim3((unsigned)npids, (unsigned)gy), dim3(256), 0, st, vecs, nblk, pt_off, pt_size, (uint4 *)shadow, stats);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// ---- the queries: fp16 copy in B-operand order, and every query's error bound -----------------------------------------------------
// One wave per query.  xq4[(q * nblk + c) * 4 + g] holds columns 16c + g + {0, 4, 8, 12}; lane (c, g) converts that float4, the lanes of
// an even c write their 8 B and those of c + 1 behind them: xqh[(q * nbs + b) * 4 + g], which the scan stages like xq4.
__global__ __launch_bounds__(256) void k_shadow_prep(const float4 *__restrict__ xq4, const float *__restrict__ xn, int64_t Q, int d, int nblk,
                                                     int metric_l2, float rho, float xmax, uint4 *__restrict__ xqh, float *__restrict__ E) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int nbs = (nblk + 1) >> 1;
    float e2 = 0.0f;
    uint32_t bad = 0;
    for (int c0 = 0; c0 < 2 * nbs; c0 += 16) {  // 16 arena blocks (64 float4) per round; d <= 256: one round
        const int c = c0 + (lane >> 2), g = lane & 3;
        const float4 a = c < nblk ? xq4[(q * nblk + c) * 4 + g] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float v[4] = {a.x, a.y, a.z, a.w};
        uint32_t hb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float e, hf;
            hb[i] = qk_h_bits(v[i], e, hf);
            e2 = __fmaf_rn(e, e, e2);
            bad |= fabsf(v[i]) <= 65504.0f ? 0u : 1u;
        }
        const uint32_t lo = hb[0] | (hb[1] << 16), hi = hb[2] | (hb[3] << 16);
        const uint32_t plo = __shfl_down(lo, 4), phi = __shfl_down(hi, 4);  // lane (c + 1, g)
        if ((c & 1) == 0 && c < 2 * nbs) xqh[(q * nbs + (c >> 1)) * 4 + g] = make_uint4(lo, hi, plo, phi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o);
    const bool anybad = __ballot(bad != 0) != 0;
    if (lane == 0) {
        const float up = 1.0009765625f;
        float b = anybad ? -1.0f : qk_shadow_bound(metric_l2, d, sqrtf(xn[q]) * up, sqrtf(e2) * up, rho, xmax);
        E[q] = b >= 0.0f ? b : -1.0f;  // (NaN: no bound)
    }
}

int qk_launch_shadow_prep(hipStream_t st, const float4 *xq4, const float *xn, int64_t Q, int d, int nblk, int metric, float rho, float xmax,
                          float4 *xqh, float *E) {
    hipLaunchKernelGGL(k_shadow_prep, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, xq4, xn, Q, d, nblk, metric == QK_METRIC_L2 ? 1 : 0, rho, xmax,
                       (uint4 *)xqh, E);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// ---- the scan kernel -----------------------------------------------------------------------------------------------------------------
// The tile form's body over the shadow (see qk_scan_body.inc).  Its own kernel in its own translation unit: no instantiation of
// k_scan changes.  Pools of k' + 32 = 64 entries: one wave wide (MAXCH 1).
template <int DB, bool L2>
__global__ __launch_bounds__(256) void k_scan_shadow(ScanParams P) {
    constexpr int MODE = 0;
    constexpr int MAXCH = 1;
#define QK_SCAN_FILT 0
#define QK_SCAN_SHADOW
#include "qk_scan_body.inc"
#undef QK_SCAN_SHADOW
#undef QK_SCAN_FILT
}

template <int DB>
static int launch_scan_shadow(dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_shadow<DB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_shadow<DB, true>), grid, block, lds, st, sp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_shadow<DB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_shadow<DB, false>), grid, block, lds, st, sp);
    }
    return QK_OK;
}

int qk_launch_scan_shadow(int db, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.C > 64) QK_FAIL(QK_ERR_UNSUPPORTED, "shadow scan: pools of %d entries (one wave holds 64)", sp.C);
    if (db == 1) return launch_scan_shadow<1>(grid, block, lds, st, sp);
    if (db == 2) return launch_scan_shadow<2>(grid, block, lds, st, sp);
    if (db == 4) return launch_scan_shadow<4>(grid, block, lds, st, sp);
    if (db == 8) return launch_scan_shadow<8>(grid, block, lds, st, sp);
    QK_FAIL(QK_ERR_UNSUPPORTED, "no shadow scan kernel for DB=%d", db);
}

// ---- the exact finish ----------------------------------------------------------------------------------------------------------------
// One wave per query (P = 1: the query's pair is its number).  The records of the pair hold up to k' = 32 (approximate key, arena
// row) entries each, ascending; a record with k' entries may have dropped rows, all of them with approximate keys >= its last one.
//   1. a_k = the k-th smallest approximate key of all entries.  k entries lie at or under it, so the true k-th exact key t is at most
//      a_k + E, and a row of the answer that is among the entries has an approximate key <= t + E <= a_k + 2E: the candidates.
//   2. the canonical key of every candidate (the k-ordered fmaf chain of the seed and of the fp32 matrix path), tau = their k-th smallest
//   3. verified, if every full record's last key is > tau + E: a dropped row's exact key is then > tau, it is not in the answer and
//      cannot tie with it.  (Rows the start bound kept out: approximate key > seed + E, exact key > seed >= t.)
//   4. not verified, no record at all, or a query without a bound: the same wave scans the query's list with the exact chain.
//
// Who loads what, and when.  Loads that do not depend on each other are issued together:
//   a. the pair's slot line (one load: lane i holds record i), E, the query and its norm
//   b. headers, keys and rows of the records -- eight records a round, the wave covering two records of k' entries per step as
//      (lane >> 5, lane & 31), every load of the round issued before one is consumed.  Step 1 needs no pool: a_k comes from a
//      bisection on the key bits over the round's registers (sf_kth), the smallest last key of the full records from the same
//      read.  More than eight records: the k smallest keys so far are carried from round to round, and step 2 reads the records
//      a second time (from the cache).  Records behind the slot line are chained: a serial walk, one record a round.
//   c. the candidates of all records in one list (arena rows, ballot prefix), 64 a round, a lane each: the row pieces of
//      QK_SF_GROUP column blocks, the norm and the id are in flight before the fused chain starts; a further round trip per
//      further group of blocks
//   d. one compaction of (exact key, id) per round of 64, carrying the k survivors; the store
// What this bought and what it did not (the dependent trips were not what the kernel's time was made of): NOTES.md.
constexpr int QK_SF_POOL = 128;  // pool entries (two per lane); compacted to k when more than 64 are held
constexpr int QK_SF_ROUND = 8;   // records of the slot line per round: four steps of two
#ifndef QK_SF_GROUP
#define QK_SF_GROUP 8            // column blocks of a candidate's row in flight per lane (a side build may set 4: -DQK_SF_GROUP=4)
#endif
#ifndef QK_SF_WAVES
#define QK_SF_WAVES 1            // waves per SIMD the register budget is held to
#endif

// Step 1, one round: the k-th smallest of the keys in o[0..NR) (0xFFFFFFFF: no entry) and of the carry cr (lanes < k: the k smallest
// keys of the earlier rounds).  select_core's bisection: T = the largest value with fewer than k keys below it; 0xFFFFFFFF while
// fewer than k entries were seen.  more: another round follows -- the carry becomes the keys below T and T in the places left.
template <int NR>
__device__ __forceinline__ uint32_t sf_kth(const uint32_t (&o)[NR], uint32_t &cr, int k, int lane, uint32_t *carry, bool more) {
    uint32_t T = 0;
    for (int b = 31; b >= 0; b--) {
        const uint32_t tr = T | (1u << b);
        int c = __popcll(__ballot(cr < tr));
#pragma unroll
        for (int i = 0; i < NR; i++) c += __popcll(__ballot(o[i] < tr));
        if (c < k) T = tr;
    }
    if (more) {
        int base = 0;
#pragma unroll
        for (int i = 0; i <= NR; i++) {
            const uint32_t v = i < NR ? o[i % NR] : cr;
            const bool keep = v < T;
            const uint64_t m = __ballot(keep);
            if (keep) carry[base + __popcll(m & ((1ull << lane) - 1ull))] = v;  // (fewer than k keys lie below T)
            base += __popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        cr = lane < base ? carry[lane] : lane < k ? T : 0xFFFFFFFFu;
        __builtin_amdgcn_wave_barrier();
    }
    return T;
}

__global__ __launch_bounds__(64, QK_SF_WAVES) void k_shadow_finish(ShadowFinishParams F) {
    __shared__ int64_t pool_id[QK_SF_POOL];
    __shared__ uint32_t pool_ord[QK_SF_POOL];
    __shared__ int64_t cand_row[64 + 4 * 64];  // the candidates' arena rows: fewer than 64 left over + a round's four registers
    __shared__ uint32_t carry[QK_SHADOW_MAX_K];
    __shared__ float xs[QK_SHADOW_MAX_D];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int k = F.k;
    const bool l2 = F.metric == QK_METRIC_L2;
    constexpr int KP = QK_SHADOW_KP;
    // trip 1
    const int sv = lane < QK_SLOTS ? F.pair_slots[q * QK_SLOTS + lane] : -1;  // lane 0: the count; lane i: record i - 1
    const float E = F.E[q];
    const float xnq = F.xn[q];
    float xv[QK_SHADOW_MAX_D / 64];
#pragma unroll
    for (int t = 0; t < QK_SHADOW_MAX_D / 64; t++) xv[t] = lane + 64 * t < F.d ? F.x[q * F.d + lane + 64 * t] : 0.0f;
#pragma unroll
    for (int t = 0; t < QK_SHADOW_MAX_D / 64; t++)
        if (lane + 64 * t < F.nblk * 16) xs[lane + 64 * t] = xv[t];
    const bool flagged = !(E >= 0.0f);
    __syncthreads();
    // the canonical key of an arena row and the row's id: columns in natural order, one fused step each (seed_row_key's arithmetic,
    // qk_scan.hip).  QK_SF_GROUP column blocks a group: a group's pieces (four of 16 B per block; blocks behind the last one are not
    // loaded) are issued before the first is used; the norm and the id are loaded behind the first group's pieces, so that the chain
    // starts as soon as those arrive.  The next group is loaded when the chain is through with this one: a round trip per group.
    auto exact_key = [&](int64_t row, int64_t &id) __attribute__((always_inline)) -> uint32_t {
        constexpr int G = QK_SF_GROUP;
        const int64_t tile = row >> 4;
        const int r = (int)(row & 15);
        float acc = 0.0f;
        float4 v[G][4];
        auto load_group = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < G; j++) {
                if (c0 + j < F.nblk) {
                    const float4 *blk = F.vecs + (tile * F.nblk + c0 + j) * 64 + r;
                    v[j][0] = blk[0];
                    v[j][1] = blk[16];
                    v[j][2] = blk[32];
                    v[j][3] = blk[48];
                }
            }
        };
        auto chain_group = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < G; j++) {
                if (c0 + j < F.nblk) {
                    // (columns 16c .. 16c + 15 in order: element t of lane group g is column 16c + 4t + g; written out, no indexed array)
                    const float *xc = xs + 16 * (c0 + j);
                    acc = __fmaf_rn(v[j][0].x, xc[0], acc);
                    acc = __fmaf_rn(v[j][1].x, xc[1], acc);
                    acc = __fmaf_rn(v[j][2].x, xc[2], acc);
                    acc = __fmaf_rn(v[j][3].x, xc[3], acc);
                    acc = __fmaf_rn(v[j][0].y, xc[4], acc);
                    acc = __fmaf_rn(v[j][1].y, xc[5], acc);
                    acc = __fmaf_rn(v[j][2].y, xc[6], acc);
                    acc = __fmaf_rn(v[j][3].y, xc[7], acc);
                    acc = __fmaf_rn(v[j][0].z, xc[8], acc);
                    acc = __fmaf_rn(v[j][1].z, xc[9], acc);
                    acc = __fmaf_rn(v[j][2].z, xc[10], acc);
                    acc = __fmaf_rn(v[j][3].z, xc[11], acc);
                    acc = __fmaf_rn(v[j][0].w, xc[12], acc);
                    acc = __fmaf_rn(v[j][1].w, xc[13], acc);
                    acc = __fmaf_rn(v[j][2].w, xc[14], acc);
                    acc = __fmaf_rn(v[j][3].w, xc[15], acc);
                }
            }
        };
        load_group(0);
        const float nrm = l2 ? F.norms[row] : 0.0f;
        id = F.ids[row];
        chain_group(0);
        for (int c0 = G; c0 < F.nblk; c0 += G) {
            load_group(c0);
            chain_group(c0);
        }
        return l2 ? ord_from_l2(l2_expanded(xnq, nrm, acc)) : ord_from_ip(acc);
    };
    int cnt = 0;
    uint32_t tau = 0xFFFFFFFFu;
    auto append = [&](bool pass, uint32_t o, int64_t id) __attribute__((always_inline)) {
        const uint64_t m = __ballot(pass);
        if (!m) return;
        if (pass) {
            const int sl = cnt + __popcll(m & ((1ull << lane) - 1ull));
            pool_ord[sl] = o;
            pool_id[sl] = id;
        }
        cnt += __popcll(m);
        if (cnt > QK_SF_POOL - 64) {
            uint32_t kth;
            cnt = select_pool<2>(pool_ord, pool_id, cnt, k, lane, kth);
            if (cnt >= k) tau = min(tau, kth);
        }
    };
    const int nrecs = __builtin_amdgcn_readlane(sv, 0);
    const bool chained = nrecs > QK_SLOTS - 1;
    bool verified = false;
    int ncand = 0;
    if (!flagged && nrecs > 0) {
        // trip 2: this lane's record of the slot line and its entry count
        const int ns = min(nrecs, QK_SLOTS - 1);
        const int myrec = (lane >= 1 && lane <= ns && sv >= 0 && sv < F.max_recs) ? sv : -1;
        int myn = 0;  // (first used behind the round's loads: the header is in flight next to them)
        if (myrec >= 0) myn = F.rec_hdr[myrec].y;
        const int h = lane >> 5, e = lane & 31;
        uint32_t o[4];   // the round's approximate keys (0xFFFFFFFF: no entry)
        int64_t rw[4];   // and arena rows (-1: no entry)
        uint32_t fullmin = 0xFFFFFFFFu;  // (this lane's share, built by step 1's reads only; reduced behind its last round)
        auto load_round = [&](int r0, bool step1) __attribute__((always_inline)) {
            // (the loads need the record numbers only: they are issued next to the headers', the entry counts mask them afterwards)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int rec = __shfl(myrec, r0 + 2 * j + h + 1);  // (lane <= 32: one without a record)
                o[j] = rec >= 0 ? F.rec_ord[(int64_t)rec * KP + e] : 0xFFFFFFFFu;
                rw[j] = rec >= 0 ? F.rec_id[(int64_t)rec * KP + e] : -1;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int n = min(__shfl(myn, r0 + 2 * j + h + 1), KP);
                const bool has = e < n;  // (no record: n = 0)
                if (step1 && has && n >= KP && e == KP - 1) fullmin = min(fullmin, o[j]);
                o[j] = has ? o[j] : 0xFFFFFFFFu;
                rw[j] = has ? rw[j] : -1;
            }
        };
        // a chained record: the lower half of one register
        auto load_chained = [&](int rec, int &next, bool step1) __attribute__((always_inline)) {
            const int2 hd = F.rec_hdr[rec];
            const uint32_t ov = lane < KP ? F.rec_ord[(int64_t)rec * KP + lane] : 0xFFFFFFFFu;
            const int64_t rv = lane < KP ? F.rec_id[(int64_t)rec * KP + lane] : -1;
            const int n = min(hd.y, KP);
            const bool has = lane < n;
            o[0] = has ? ov : 0xFFFFFFFFu;
            rw[0] = has ? rv : -1;
            if (step1 && has && n >= KP && lane == KP - 1) fullmin = min(fullmin, ov);
            next = hd.x;
        };
        // 1. the k-th smallest approximate key; the smallest last key of the full records
        const bool one_round = ns <= QK_SF_ROUND && !chained;  // (the keys and rows stay in their registers for step 2)
        uint32_t cr = 0xFFFFFFFFu, a_k = 0xFFFFFFFFu;
        for (int r0 = 0; r0 < ns; r0 += QK_SF_ROUND) {
            load_round(r0, true);
            a_k = sf_kth<4>(o, cr, k, lane, carry, r0 + QK_SF_ROUND < ns || chained);  // (the carry: only if a round follows)
        }
        if (chained) {
            int rec = F.pair_head[q];
            while (rec >= 0 && rec < F.max_recs) {
                int next;
                load_chained(rec, next, true);
                const uint32_t o1[1] = {o[0]};
                a_k = sf_kth<1>(o1, cr, k, lane, carry, true);
                rec = next;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) fullmin = min(fullmin, (uint32_t)__shfl_xor((int)fullmin, s));
        const uint32_t thr = qk_ord_widen(a_k, 2.0f * E, l2);
        // 2. exact keys of the candidates: their rows into one list, 64 of the list a round, the k best carried under (key, id)
        //    (one loop over the rounds of the slot line, the chained records and the list's rest: the re-score stands in the code once)
        int lcnt = 0;
        cnt = 0;
        auto take = [&](uint32_t ov, int64_t rv) __attribute__((always_inline)) {  // one register of entries
            const bool cand = rv >= 0 && ov <= thr;
            const uint64_t cm = __ballot(cand);
            if (cand) cand_row[lcnt + __popcll(cm & ((1ull << lane) - 1ull))] = rv;
            lcnt += __popcll(cm);
        };
        int r0 = 0;
        int crec = chained ? F.pair_head[q] : -1;
        for (bool last = false; !last;) {
            if (r0 < ns) {
                if (!one_round) load_round(r0, false);
#pragma unroll
                for (int j = 0; j < 4; j++) take(o[j], rw[j]);
                r0 += QK_SF_ROUND;
            } else if (crec >= 0 && crec < F.max_recs) {
                int next;
                load_chained(crec, next, false);
                take(o[0], rw[0]);
                crec = next;
            } else {
                last = true;
            }
            __builtin_amdgcn_wave_barrier();
            int base = 0;
            while (lcnt >= 64 || (last && lcnt > 0)) {  // trip 3: 64 rows of the list, a lane each
                const int m = min(lcnt, 64);
                uint32_t key = 0xFFFFFFFFu;
                int64_t id = -1;
                if (lane < m) {
                    key = exact_key(cand_row[base + lane], id);
                }
                const bool pass = key != 0xFFFFFFFFu;
                const uint64_t pm = __ballot(pass);
                if (pass) {
                    const int sl = cnt + __popcll(pm & ((1ull << lane) - 1ull));
                    pool_ord[sl] = key;
                    pool_id[sl] = id;
                }
                cnt += __popcll(pm);  // (<= k + 64)
                cnt = compact_pool<2>(pool_ord, pool_id, cnt, k, lane);
                ncand += m;
                base += m;
                lcnt -= m;
            }
            if (base > 0 && lcnt > 0) {  // fewer than 64 are left: to the list's front
                const int64_t rest = lane < lcnt ? cand_row[base + lane] : -1;
                __builtin_amdgcn_wave_barrier();
                if (lane < lcnt) cand_row[lane] = rest;
                __builtin_amdgcn_wave_barrier();
            }
        }
        // 3. no dropped row can belong to the answer
        const uint32_t tau_ex = cnt >= k ? pool_ord[k - 1] : 0xFFFFFFFFu;
        verified = fullmin == 0xFFFFFFFFu || (tau_ex != 0xFFFFFFFFu && fullmin > qk_ord_widen(tau_ex, E, l2));
    }
    bool fell_back = false;
    if (!verified) {
        // 4. the whole list, exactly: one row per lane
        int64_t p = -1;
        if (F.pids_packed) {
            const unsigned long long v = F.pids_packed[q];
            p = v == ~0ull ? -1 : (int64_t)(v & 0xFFFFFFFFull);
        } else if (F.pids) {
            p = F.pids[q];
        }
        const int size = (p >= 0 && p < F.npids) ? F.pt_size[p] : 0;
        cnt = 0;
        tau = 0xFFFFFFFFu;
        if (size > 0) {
            fell_back = true;
            const int64_t row_off = F.pt_off[p];
            for (int r0 = 0; r0 < size; r0 += 64) {
                const bool has = r0 + lane < size;
                uint32_t key = 0xFFFFFFFFu;
                int64_t id = -1;
                if (has) key = exact_key(row_off + r0 + lane, id);
                append(has && key != 0xFFFFFFFFu && key <= tau, key, id);
            }
        }
        cnt = compact_pool<2>(pool_ord, pool_id, cnt, k, lane);
    }
    for (int e = lane; e < k; e += 64) {  // (k_merge_flat's conversion)
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
    if (lane == 0) {
        if (verified) atomicAdd(&F.counters[0], 1ull);
        if (fell_back) atomicAdd(&F.counters[1], 1ull);
        if (ncand) atomicAdd(&F.counters[2], (unsigned long long)ncand);
        if (!flagged && chained) atomicAdd(&F.counters[3], 1ull);  // (the serial walk of the chained records ran)
    }
}

int qk_shadow_counters_ensure(qk_ctx *ctx, hipStream_t st) {
    if (ctx->shadow_counters) return QK_OK;
    QK_HIP(hipMalloc((void **)&ctx->shadow_counters, 4 * sizeof(unsigned long long)));
    QK_HIP(hipMemsetAsync(ctx->shadow_counters, 0, 4 * sizeof(unsigned long long), st));
    return QK_OK;
}

int qk_launch_shadow_finish(hipStream_t st, const ShadowFinishParams &fp, int64_t Q) {
    if (Q <= 0) return QK_OK;
    hipLaunchKernelGGL(k_shadow_finish, dim3((unsigned)Q), dim3(64), 0, st, fp);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// ---- test and diagnosis hook: the exact finish on caller-built records ------------------------------------------------------------
// What qk_scan_device does behind its shadow scan -- the same launcher, the same kernel -- on records the caller laid out over a
// real store (include/quake_hip.h).  Host arrays in and out; everything the kernel would trust is checked here first.
namespace {
struct sf_dev_bufs {  // device copies of one call, freed on every way out
    std::vector<void *> p;
    ~sf_dev_bufs() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
    template <class T>
    int up(hipStream_t st, const T *host, size_t n, T **dev) {
        *dev = nullptr;
        void *q = nullptr;
        if (hipMalloc(&q, std::max(n, (size_t)1) * sizeof(T)) != hipSuccess) QK_FAIL(QK_ERR_OOM, "qk_debug_shadow_finish: device allocation failed");
        p.push_back(q);
        if (host && n) QK_HIP(hipMemcpyAsync(q, host, n * sizeof(T), hipMemcpyHostToDevice, st));
        *dev = (T *)q;
        return QK_OK;
    }
};
}  // namespace

int qk_debug_shadow_finish(qk_ctx *ctx, qk_store *s, int64_t Q, int k, int metric, int sqrt_l2, const float *x, const float *E,
                           const int64_t *lists, const int32_t *pair_slots, const int32_t *pair_head, const int32_t *rec_hdr,
                           const uint32_t *rec_ord, const int64_t *ent_list, const int64_t *ent_pos, int32_t max_recs, int64_t *out_ids,
                           float *out_dist, int64_t *counters) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: ctx or store is null");
    if (Q < 0 || Q > INT32_MAX || k < 1 || max_recs < 0)
        QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: bad sizes (Q=%lld k=%d max_recs=%d)", (long long)Q, k, (int)max_recs);
    if (k > QK_SHADOW_MAX_K) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: k=%d exceeds %d", k, QK_SHADOW_MAX_K);
    if (s->d > QK_SHADOW_MAX_D) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: d=%d exceeds %d", s->d, QK_SHADOW_MAX_D);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (Q > 0 && (!x || !E || !lists || !pair_slots || !pair_head || !out_ids || !counters ||
                  (max_recs > 0 && (!rec_hdr || !rec_ord || !ent_list || !ent_pos))))
        QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: null argument");
    if (counters) counters[0] = counters[1] = counters[2] = counters[3] = 0;
    if (Q == 0) return QK_OK;
    const int64_t nlist = (int64_t)s->parts.size();
    auto rec_ok = [&](int64_t r) { return r >= -1 && r < max_recs; };
    // records: the header, and every entry's (list, position) -> arena row from the store's own table
    std::vector<int64_t> rows((size_t)max_recs * QK_SHADOW_KP, 0);
    for (int64_t r = 0; r < max_recs; r++) {
        const int next = rec_hdr[2 * r], n = rec_hdr[2 * r + 1];
        if (!rec_ok(next) || n < 0 || n > QK_SHADOW_KP)
            QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: record %lld: header {%d, %d}", (long long)r, next, n);
        for (int e = 0; e < n; e++) {
            const int64_t l = ent_list[r * QK_SHADOW_KP + e], pos = ent_pos[r * QK_SHADOW_KP + e];
            if (l < 0 || l >= nlist || !s->parts[(size_t)l].present || pos < 0 || pos >= s->parts[(size_t)l].size)
                QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: record %lld entry %d: no row %lld in list %lld", (long long)r, e, (long long)pos,
                        (long long)l);
            rows[(size_t)(r * QK_SHADOW_KP + e)] = s->parts[(size_t)l].row_off + pos;
        }
    }
    for (int64_t q = 0; q < Q; q++) {
        if (lists[q] < -1 || lists[q] >= nlist) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: query %lld: list %lld", (long long)q, (long long)lists[q]);
        const int32_t *sl = pair_slots + q * QK_SLOTS;
        if (sl[0] < 0) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: query %lld: record count %d", (long long)q, sl[0]);
        for (int i = 0; i < std::min(sl[0], QK_SLOTS - 1); i++)
            if (!rec_ok(sl[1 + i])) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: query %lld slot %d: record %d", (long long)q, i, sl[1 + i]);
        int64_t steps = 0;
        for (int r = pair_head[q]; r != -1; r = rec_hdr[2 * (int64_t)r]) {
            if (!rec_ok(r)) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: query %lld: chained record %d", (long long)q, r);
            if (++steps > max_recs) QK_FAIL(QK_ERR_INVALID, "qk_debug_shadow_finish: query %lld: the chain does not end", (long long)q);
        }
    }
    QK_HIP(hipSetDevice(ctx->device));
    QK_TRY(qk_store_sync_table(s));
    hipStream_t st = ctx->stream;
    QK_TRY(qk_shadow_counters_ensure(ctx, st));
    sf_dev_bufs B;
    float *d_x, *d_E, *d_dist;
    int64_t *d_lists, *d_rows, *d_ids;
    int32_t *d_slots, *d_head, *d_hdr;
    uint32_t *d_ord;
    const size_t nent = (size_t)max_recs * QK_SHADOW_KP;
    QK_TRY(B.up(st, x, (size_t)Q * s->d, &d_x));
    QK_TRY(B.up(st, E, (size_t)Q, &d_E));
    QK_TRY(B.up(st, lists, (size_t)Q, &d_lists));
    QK_TRY(B.up(st, pair_slots, (size_t)Q * QK_SLOTS, &d_slots));
    QK_TRY(B.up(st, pair_head, (size_t)Q, &d_head));
    QK_TRY(B.up(st, rec_hdr, (size_t)max_recs * 2, &d_hdr));
    QK_TRY(B.up(st, rec_ord, nent, &d_ord));
    QK_TRY(B.up(st, rows.data(), nent, &d_rows));
    QK_TRY(B.up(st, (const int64_t *)nullptr, (size_t)Q * k, &d_ids));
    QK_TRY(B.up(st, (const float *)nullptr, (size_t)Q * k, &d_dist));
    const float4 *xq4 = nullptr;
    const float *xn = nullptr;
    QK_TRY(qk_prep_queries(ctx, d_x, Q, s->d, &xq4, &xn));  // (the library's own preparation: the norms)
    unsigned long long c0[4], c1[4];
    QK_HIP(hipMemcpyAsync(c0, ctx->shadow_counters, sizeof(c0), hipMemcpyDeviceToHost, st));
    ShadowFinishParams fp;
    fp.pair_head = d_head;
    fp.pair_slots = d_slots;
    fp.rec_hdr = (const int2 *)d_hdr;
    fp.rec_ord = d_ord;
    fp.rec_id = d_rows;
    fp.max_recs = max_recs;
    fp.k = k;
    fp.metric = metric;
    fp.sqrt_l2 = sqrt_l2 ? 1 : 0;
    fp.out_ids = d_ids;
    fp.out_dist = out_dist ? d_dist : nullptr;
    fp.E = d_E;
    fp.x = d_x;
    fp.xn = xn;
    fp.vecs = (const float4 *)s->vecs;
    fp.norms = s->norms;
    fp.ids = s->ids;
    fp.nblk = s->nblk;
    fp.d = s->d;
    fp.pids = d_lists;
    fp.pids_packed = nullptr;
    fp.pt_off = s->d_off;
    fp.pt_size = s->d_size;
    fp.npids = (int)nlist;
    fp.counters = ctx->shadow_counters;
    QK_TRY(qk_launch_shadow_finish(st, fp, Q));
    QK_HIP(hipMemcpyAsync(c1, ctx->shadow_counters, sizeof(c1), hipMemcpyDeviceToHost, st));
    QK_HIP(hipMemcpyAsync(out_ids, d_ids, (size_t)Q * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (out_dist) QK_HIP(hipMemcpyAsync(out_dist, d_dist, (size_t)Q * k * sizeof(float), hipMemcpyDeviceToHost, st));
    QK_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) counters[i] = (int64_t)(c1[i] - c0[i]);
    return QK_OK;
}

extern "C" float qk_shadow_error_bound(int metric, int d, float qnorm, float rho_q, float rho, float xmax) {
    return qk_shadow_bound(metric == QK_METRIC_L2 ? 1 : 0, d, qnorm, rho_q, rho, xmax);
}
