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
constexpr int QK_SF_POOL = 128;  // pool entries (two per lane); compacted to k when more than 64 are held

__global__ __launch_bounds__(64) void k_shadow_finish(ShadowFinishParams F) {
    __shared__ int64_t pool_id[QK_SF_POOL];
    __shared__ uint32_t pool_ord[QK_SF_POOL];
    __shared__ float xs[QK_SHADOW_MAX_D];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int k = F.k;
    const bool l2 = F.metric == QK_METRIC_L2;
    constexpr int KP = QK_SHADOW_KP;
    const float E = F.E[q];
    const bool flagged = !(E >= 0.0f);
    for (int i = lane; i < F.nblk * 16; i += 64) xs[i] = i < F.d ? F.x[q * F.d + i] : 0.0f;
    __syncthreads();
    const float xnq = F.xn[q];
    // the canonical key of an arena row: columns in natural order, one fused step each (seed_row_key's arithmetic, qk_scan.hip)
    auto exact_key = [&](int64_t row) __attribute__((always_inline)) -> uint32_t {
        const int64_t tile = row >> 4;
        const int r = (int)(row & 15);
        float acc = 0.0f;
#pragma unroll 2
        for (int c = 0; c < F.nblk; c++) {
            const float4 *blk = F.vecs + (tile * F.nblk + c) * 64 + r;
            const float4 v0 = blk[0], v1 = blk[16], v2 = blk[32], v3 = blk[48];
            // (columns 16c .. 16c + 15 in order: element t of lane group g is column 16c + 4t + g; written out, no indexed array)
            const float *xc = xs + 16 * c;
            acc = __fmaf_rn(v0.x, xc[0], acc);
            acc = __fmaf_rn(v1.x, xc[1], acc);
            acc = __fmaf_rn(v2.x, xc[2], acc);
            acc = __fmaf_rn(v3.x, xc[3], acc);
            acc = __fmaf_rn(v0.y, xc[4], acc);
            acc = __fmaf_rn(v1.y, xc[5], acc);
            acc = __fmaf_rn(v2.y, xc[6], acc);
            acc = __fmaf_rn(v3.y, xc[7], acc);
            acc = __fmaf_rn(v0.z, xc[8], acc);
            acc = __fmaf_rn(v1.z, xc[9], acc);
            acc = __fmaf_rn(v2.z, xc[10], acc);
            acc = __fmaf_rn(v3.z, xc[11], acc);
            acc = __fmaf_rn(v0.w, xc[12], acc);
            acc = __fmaf_rn(v1.w, xc[13], acc);
            acc = __fmaf_rn(v2.w, xc[14], acc);
            acc = __fmaf_rn(v3.w, xc[15], acc);
        }
        return l2 ? ord_from_l2(l2_expanded(xnq, F.norms[row], acc)) : ord_from_ip(acc);
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
    const int nrecs = F.pair_slots[q * QK_SLOTS];
    // (every lambda here is inlined: a closure that is passed by address lives in scratch memory)
    auto each_record = [&](auto &&f) __attribute__((always_inline)) {
        const int ns = min(nrecs, QK_SLOTS - 1);
        for (int i = 0; i < ns; i++) {
            const int rec = F.pair_slots[q * QK_SLOTS + 1 + i];
            if (rec >= 0 && rec < F.max_recs) f(rec);
        }
        if (nrecs > QK_SLOTS - 1) {  // chained records (the header names the next one)
            int rec = F.pair_head[q];
            while (rec >= 0 && rec < F.max_recs) {
                f(rec);
                rec = F.rec_hdr[rec].x;
            }
        }
    };
    bool verified = false;
    int ncand = 0;
    if (!flagged && nrecs > 0) {
        // 1. the k-th smallest approximate key; the smallest last key of the full records
        uint32_t fullmin = 0xFFFFFFFFu;
        each_record([&](int rec) __attribute__((always_inline)) {
            const int n = min(F.rec_hdr[rec].y, KP);
            const bool has = lane < n;
            const uint32_t o = has ? F.rec_ord[(int64_t)rec * KP + lane] : 0xFFFFFFFFu;
            const int64_t row = has ? F.rec_id[(int64_t)rec * KP + lane] : -1;
            if (n >= KP) fullmin = min(fullmin, (uint32_t)__builtin_amdgcn_readlane((int)o, KP - 1));
            append(has && o <= tau, o, row);
        });
        cnt = compact_pool<2>(pool_ord, pool_id, cnt, k, lane);
        const uint32_t a_k = cnt >= k ? pool_ord[k - 1] : 0xFFFFFFFFu;
        const uint32_t thr = qk_ord_widen(a_k, 2.0f * E, l2);
        // 2. exact keys of the candidates, pooled under (key, id)
        cnt = 0;
        tau = 0xFFFFFFFFu;
        each_record([&](int rec) __attribute__((always_inline)) {
            const int n = min(F.rec_hdr[rec].y, KP);
            const bool has = lane < n;
            const uint32_t o = has ? F.rec_ord[(int64_t)rec * KP + lane] : 0xFFFFFFFFu;
            const bool cand = has && o <= thr;
            const uint64_t cm = __ballot(cand);
            if (!cm) return;
            ncand += __popcll(cm);
            uint32_t key = 0xFFFFFFFFu;
            int64_t id = -1;
            if (cand) {
                const int64_t row = F.rec_id[(int64_t)rec * KP + lane];
                key = exact_key(row);
                id = F.ids[row];
            }
            append(cand && key != 0xFFFFFFFFu && key <= tau, key, id);
        });
        cnt = compact_pool<2>(pool_ord, pool_id, cnt, k, lane);
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
                if (has) {
                    key = exact_key(row_off + r0 + lane);
                    id = F.ids[row_off + r0 + lane];
                }
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
        if (!flagged && nrecs > QK_SLOTS - 1) atomicAdd(&F.counters[3], 1ull);  // (the chain branch of each_record ran)
    }
}

int qk_launch_shadow_finish(hipStream_t st, const ShadowFinishParams &fp, int64_t Q) {
    if (Q <= 0) return QK_OK;
    hipLaunchKernelGGL(k_shadow_finish, dim3((unsigned)Q), dim3(64), 0, st, fp);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

extern "C" float qk_shadow_error_bound(int metric, int d, float qnorm, float rho_q, float rho, float xmax) {
    return qk_shadow_bound(metric == QK_METRIC_L2 ? 1 : 0, d, qnorm, rho_q, rho, xmax);
}
