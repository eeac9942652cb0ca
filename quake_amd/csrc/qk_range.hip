// qk_range.hip -- range search: every row of the probed lists within a radius of each query (include/quake_hip.h, "range search").
//
// The expensive half is the key-emission scan, run pass by pass by qk_emit_passes (qk_dense.hip): one pass over the vectors
// writes the canonical key of every (query, probed row) to keys[pair_base[pair] + row] -- pairs in (query, rank) order, rows in
// stored order, which is the order a range result wants.  The host turns the radius into ONE closed interval of keys
// [key_lo, key_hi] (qk_range_key_bounds below), so "inside the radius" is an integer comparison and inclusive means inclusive.
// This file's device work, per pass of queries:
//   k_range_count    a query's segment is cut into slices of QK_RANGE_SLICE keys; a workgroup takes one slice at a time, its four waves
//                    count the hits of their quarter (ballot + popcount), the per-wave counts are kept for the writer
//   k_range_qscan    one wave per query: exclusive scan of the counts of the query's slices, and the query's total
//   k_range_offsets  one workgroup: exclusive scan of the query totals of the pass, continued from a running total that lives on the
//                    device (no host synchronisation between passes): lims[q0 .. q0 + nq]
//   k_range_write    the same decomposition as the count: every wave starts at lims[q] + slice offset + the counts of the waves
//                    before it and gives each hit its position with a ballot prefix -- a stable compaction, no atomics; positions
//                    >= cap are skipped.  The hits of a wave are first listed in LDS, then written side by side.  List and row of
//                    key i: emit_key_row (qk_device.h); the id from the arena; the distance from the key, converted like every
//                    selection kernel does.
// A filter is tested here, not in the scan (the emission kernels take no mask): the mask bit of arena row pt_off[list] + row.
// The host side is this file's kernels plus one description: range_call states the call for qk_emit_run (qk_emit.hip), the host
// body of every entry point on the emission scan, and range_device hangs the launches above into qk_emit_device's skeleton.
// Only range search uses the driver's three hooks: lims[0] = 0 for Q == 0, the copy of lims first and then of the written prefix
// of ids and distances, and the list statistics of qk_timing.
#include "qk_internal.h"

#include <cmath>
#include <cstring>
#include "qk_device.h"

constexpr int QK_RANGE_SLICE = 4096;  // keys per workgroup: 4 waves x 16 steps x 64 lanes

namespace {

struct RangeParams {
    const uint32_t *keys;
    const int64_t *pair_base;  // [npairs + 1]
    const int64_t *pids;       // [nq][P] or nullptr (pair r -> list r)
    const int64_t *pt_off;
    const int64_t *ids;        // arena ids
    const uint16_t *mask;      // row mask of a filter, or nullptr
    int P, S, Sg;              // lists per query, slices per query (upper bound), workgroups per query
    uint32_t key_lo, key_hi;
    int metric, sqrt_l2;
    int32_t *cnt;              // [nq * S] hits of a slice (written for the slices that start inside the query's segment)
    int4 *cnt4;                // [nq * S] ... of its four waves
    int32_t *qexcl;            // [nq * S] position of a slice's first hit inside its query
    int32_t *qtot;             // [nq] hits of a query
    int64_t cap;
    int64_t *out_ids;
    float *out_dist;
};

// A wave's share of a slice: 16 steps of 64 consecutive keys from w0 on.  All 16 loads are issued before the first key is tested
// (a wave that waits for one 256-byte load at a time leaves the memory system idle); keys behind `end` read as 0 and fail `in`.
constexpr int QK_RANGE_STEPS = QK_RANGE_SLICE / 256;
__device__ __forceinline__ void range_load(const RangeParams &R, int64_t w0, int64_t end, int lane, uint32_t (&k)[QK_RANGE_STEPS]) {
#pragma unroll
    for (int step = 0; step < QK_RANGE_STEPS; step++) {
        const int64_t pos = w0 + step * 64 + lane;
        k[step] = pos < end ? R.keys[pos] : 0u;
    }
}

// is the key at absolute position pos a hit; *row: its arena row when the filter needed it, -1 otherwise
__device__ __forceinline__ bool range_hit(const RangeParams &R, const int64_t *pbase, const int64_t *qpids, int64_t pos, bool in, uint32_t key,
                                          int64_t *row) {
    *row = -1;
    if (!in || key < R.key_lo || key > R.key_hi) return false;
    if (!R.mask) return true;
    const int64_t r = emit_key_row(pbase, qpids, R.P, R.pt_off, pos);
    *row = r;
    return (R.mask[r >> 4] >> (r & 15)) & 1;
}

// blockIdx.x = query * Sg + g: the workgroup takes slices g, g + Sg, ... of its query while they start inside the segment (Sg <= S:
// the grid is sized for the work a pass can have, not for S slices of every query -- S comes from the LARGEST list of the store)
__global__ __launch_bounds__(256) void k_range_count(RangeParams R) {
    __shared__ int s_c[4];
    const int64_t q = blockIdx.x / R.Sg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t *pbase = R.pair_base + q * R.P;
    const int64_t *qpids = R.pids ? R.pids + q * R.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[R.P];
    for (int64_t s = blockIdx.x - q * R.Sg; beg + s * QK_RANGE_SLICE < end; s += R.Sg) {
        const int64_t b = q * R.S + s;
        const int64_t w0 = beg + s * QK_RANGE_SLICE + wave * (QK_RANGE_SLICE / 4);
        int c = 0;
        if (w0 < end) {
            uint32_t k[QK_RANGE_STEPS];
            range_load(R, w0, end, lane, k);
#pragma unroll
            for (int step = 0; step < QK_RANGE_STEPS; step++) {
                const int64_t pos = w0 + step * 64 + lane;
                int64_t row;
                c += __popcll(__ballot(range_hit(R, pbase, qpids, pos, pos < end, k[step], &row)));
            }
        }
        __syncthreads();  // (the previous slice's counts have been read)
        if (lane == 0) s_c[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            R.cnt[b] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
            R.cnt4[b] = make_int4(s_c[0], s_c[1], s_c[2], s_c[3]);
        }
    }
}

// one wave per query: the exclusive scan of the counts of the query's own slices (those that start inside its segment) ->
// qexcl[q * S + s], the position of slice s's first hit inside the query, and qtot[q], the query's hits
__global__ __launch_bounds__(256) void k_range_qscan(RangeParams R, int64_t nq) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int64_t *pbase = R.pair_base + q * R.P;
    const int64_t ns = (pbase[R.P] - pbase[0] + QK_RANGE_SLICE - 1) / QK_RANGE_SLICE;
    int run = 0;  // (a query's segment is shorter than 2^30 keys)
    for (int64_t s0 = 0; s0 < ns; s0 += 64) {
        const int64_t s = s0 + lane;
        const int c = s < ns ? R.cnt[q * R.S + s] : 0;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (s < ns) R.qexcl[q * R.S + s] = run + incl - c;
        run += __shfl(incl, 63);
    }
    if (lane == 0) R.qtot[q] = run;
}

// first[i] = run + tot[0] + ... + tot[i-1] over the nq queries of the pass (one workgroup: thread t owns a contiguous piece, the
// 1024 piece sums are scanned through LDS), written to lims[i] as well; lims[nq] = the new running total, left in run[0]
__global__ __launch_bounds__(1024) void k_range_offsets(const int32_t *__restrict__ tot, int64_t n, int64_t *run, int64_t *lims) {
    __shared__ int64_t part[1024];
    const int64_t base = run[0];
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = min(n, (int64_t)threadIdx.x * per), e = min(n, b + per);
    int64_t sum = 0;
    for (int64_t i = b; i < e; i++) sum += tot[i];
    part[threadIdx.x] = sum;
    __syncthreads();  // (every thread has read run[0])
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int64_t at = base + part[threadIdx.x] - sum;
    for (int64_t i = b; i < e; i++) {
        lims[i] = at;
        at += tot[i];
    }
    if (threadIdx.x == 1023) {
        const int64_t total = base + part[1023];
        lims[n] = total;
        run[0] = total;
    }
}

// the count's decomposition; a query's first position is its lims entry (lims points at the pass's first query)
__global__ __launch_bounds__(256) void k_range_write(RangeParams R, const int64_t *lims) {
    __shared__ uint16_t s_pos[4][QK_RANGE_SLICE / 4];
    const int64_t q = blockIdx.x / R.Sg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t *pbase = R.pair_base + q * R.P;
    const int64_t *qpids = R.pids ? R.pids + q * R.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[R.P];
    const int64_t first = lims[q];
    if (first >= R.cap) return;
    for (int64_t s = blockIdx.x - q * R.Sg; beg + s * QK_RANGE_SLICE < end; s += R.Sg) {
        const int64_t b = q * R.S + s;
        if (R.cnt[b] == 0) continue;
        const int4 c4 = R.cnt4[b];
        int64_t at = first + R.qexcl[b] + (wave > 0 ? c4.x : 0) + (wave > 1 ? c4.y : 0) + (wave > 2 ? c4.z : 0);
        const int mine = wave == 0 ? c4.x : wave == 1 ? c4.y : wave == 2 ? c4.z : c4.w;
        if (mine == 0 || at >= R.cap) continue;
        const int64_t w0 = beg + s * QK_RANGE_SLICE + wave * (QK_RANGE_SLICE / 4);
        // 1. the wave's hits, in order, as offsets from w0 into its own line of LDS (registers and ballots only: no memory traffic
        //    hangs on a hit); 2. hit j goes to position at + j: every lane follows its own chain of loads -- list, row, id, key --
        //    side by side with the other 63, and a wave's stores are consecutive
        uint32_t k[QK_RANGE_STEPS];
        range_load(R, w0, end, lane, k);
        int n = 0;
#pragma unroll
        for (int step = 0; step < QK_RANGE_STEPS; step++) {
            const int64_t pos = w0 + step * 64 + lane;
            int64_t row;
            const bool hit = range_hit(R, pbase, qpids, pos, pos < end, k[step], &row);
            const uint64_t m = __ballot(hit);
            if (hit) s_pos[wave][n + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(step * 64 + lane);
            n += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int j = lane; j < n && at + j < R.cap; j += 64) {
            const int64_t pos = w0 + s_pos[wave][j];
            const int64_t row = emit_key_row(pbase, qpids, R.P, R.pt_off, pos);
            R.out_ids[at + j] = R.ids[row];
            if (R.out_dist) {
                const uint32_t o = R.keys[pos];
                float od;
                if (R.metric == QK_METRIC_L2) {
                    const float d2 = __uint_as_float(o);
                    od = R.sqrt_l2 ? sqrtf(d2) : d2;
                } else {
                    od = ip_from_ord(o);
                }
                R.out_dist[at + j] = od;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the line is rewritten for the wave's next slice)
    }
}

// what qk_timing reports about the probed lists: a flag per list some pair of the call reached, and the count of such pairs
__global__ void k_range_mark(const int64_t *pids, int64_t npairs, int P, const int32_t *pt_size, int npids, unsigned char *flags,
                             unsigned long long *live_pairs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = false;
    if (i < npairs) {
        const int64_t p = pids ? pids[i] : (i % P);
        if (p >= 0 && p < npids && pt_size[p] > 0) {
            live = true;
            flags[p] = 1;
        }
    }
    const uint64_t m = __ballot(live);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(live_pairs, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_range_rows(const unsigned char *flags, const int32_t *pt_size, int npids, int64_t *rows_out) {
    __shared__ int64_t s_r[256];
    int64_t r = 0;
    for (int p = threadIdx.x; p < npids; p += 256)
        if (flags[p]) r += pt_size[p];
    s_r[threadIdx.x] = r;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_r[threadIdx.x] += s_r[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *rows_out = s_r[0];
}

inline uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// host copy of ord_from_ip (qk_device.h)
inline uint32_t host_ord_from_ip(float ip) {
    uint32_t b = f2u(ip);
    if (ip != ip) return 0xFFFFFFFFu;  // NaN: no candidate
    if (b == 0x80000000u) b = 0u;      // -0 -> +0
    const uint32_t asc = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ~asc;
}

// The closed key interval of "dist <= radius" (L2) / "dist >= radius" (IP) on the float32 distance the caller sees.  The key of a
// NaN distance (0xFFFFFFFF, qk_device.h) lies outside every interval: the widest one ends at the key of +inf (L2) / -inf (IP).
// Returns false when no distance can pass.  (Shared with qk_facet.hip: declared in qk_internal.h.)
}  // namespace

bool qk_range_key_bounds(int metric, bool sqrt_l2, float radius, uint32_t *lo, uint32_t *hi) {
    if (metric == QK_METRIC_IP) {
        // (+0 >= -0 and -0 >= +0 in float32: both zeros have one key)
        *lo = host_ord_from_ip(INFINITY);
        *hi = host_ord_from_ip(radius);
        return true;
    }
    *lo = 0;
    if (radius < 0.0f) return false;
    if (radius == 0.0f) radius = 0.0f;  // (-0)
    float t;
    if (!sqrt_l2 || std::isinf(radius)) {
        t = radius;
    } else {
        // the largest t >= 0 with sqrtf(t) <= radius: sqrtf is correctly rounded and monotone, radius * radius is a few ulps off
        t = radius * radius;
        while (t > 0.0f && sqrtf(t) > radius) t = nextafterf(t, 0.0f);
        for (;;) {
            const float up = nextafterf(t, INFINITY);
            if (std::isinf(up) || sqrtf(up) > radius) break;
            t = up;
        }
    }
    *hi = f2u(t);
    return true;
}


namespace {

// the device half: lims [Q + 1], out_ids / out_dist [cap] on the device
int range_device(const qk_emit_call &c, qk_emit_env &e, int64_t cap, int64_t *lims, int64_t *out_ids, float *out_dist) {
    qk_ctx *ctx = c.ctx;
    qk_store *s = c.s;
    const qk_scan_args &a = e.a;
    qk_timing *timing = c.timing;
    hipStream_t st = ctx->stream;
    const int npids = e.npids, P = e.P;
    // this pipeline's bytes of the call's buffer, sized for the largest pass:
    // [run: total hits, live pairs, rows of the lists reached, -] [list flags] [cnt] [cnt4] [excl] [qtot]
    int S = 0;
    const size_t o_flags = 256, o_cnt = o_flags + qk_al256((size_t)npids);
    size_t o_cnt4 = 0, o_excl = 0, o_qtot = 0;
    int64_t *run = nullptr;
    unsigned char *flags = nullptr;
    qk_emit_stages g;
    g.pad = [&]() -> int {  // no hits
        QK_HIP(hipMemsetAsync(lims, 0, (size_t)(a.Q + 1) * 8, st));
        return QK_OK;
    };
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        S = (int)((per_query_ub + QK_RANGE_SLICE - 1) / QK_RANGE_SLICE);
        if (*qc * (int64_t)S > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "range search: Q too large");
        const int64_t nsl_max = *qc * S;
        o_cnt4 = o_cnt + qk_al256((size_t)nsl_max * 4);
        o_excl = o_cnt4 + qk_al256((size_t)nsl_max * 16);
        o_qtot = o_excl + qk_al256((size_t)nsl_max * 4);
        *extra_bytes = o_qtot + qk_al256((size_t)*qc * 4);
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        if (p.q0 == 0) {
            run = (int64_t *)p.extra;
            flags = (unsigned char *)(p.extra + o_flags);
            QK_HIP(hipMemsetAsync(p.extra, 0, timing ? o_cnt : 256, st));
        }
        if (timing)
            hipLaunchKernelGGL(k_range_mark, dim3((unsigned)((p.nq * P + 255) / 256)), dim3(256), 0, st, p.pids, p.nq * P, P, s->d_size, npids,
                               flags, (unsigned long long *)(run + 1));
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        RangeParams R;
        R.keys = p.keys;
        R.pair_base = p.pair_base;
        R.pids = p.pids;
        R.pt_off = s->d_off;
        R.ids = s->ids;
        R.mask = e.mask;
        R.P = P;
        R.S = S;
        R.key_lo = e.key_lo;
        R.key_hi = e.key_hi;
        R.metric = a.metric;
        R.sqrt_l2 = a.sqrt_l2 ? 1 : 0;
        R.cnt = (int32_t *)(p.extra + o_cnt);
        R.cnt4 = (int4 *)(p.extra + o_cnt4);
        R.qexcl = (int32_t *)(p.extra + o_excl);
        R.qtot = (int32_t *)(p.extra + o_qtot);
        R.cap = cap;
        R.out_ids = out_ids;
        R.out_dist = out_dist;
        R.Sg = qk_emit_sg(S, p.nq);
        const unsigned grid = (unsigned)(p.nq * R.Sg);
        hipLaunchKernelGGL(k_range_count, dim3(grid), dim3(256), 0, st, R);
        hipLaunchKernelGGL(k_range_qscan, dim3((unsigned)((p.nq + 3) / 4)), dim3(256), 0, st, R, p.nq);
        hipLaunchKernelGGL(k_range_offsets, dim3(1), dim3(1024), 0, st, R.qtot, p.nq, run, lims + p.q0);
        if (cap > 0) hipLaunchKernelGGL(k_range_write, dim3(grid), dim3(256), 0, st, R, (const int64_t *)(lims + p.q0));
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    g.tail = [&]() -> int {
        if (timing) hipLaunchKernelGGL(k_range_rows, dim3(1), dim3(256), 0, st, flags, s->d_size, npids, run + 2);
        return QK_OK;
    };
    QK_TRY(qk_emit_device(c, e, g));
    if (timing) {  // the scalars qk_timing reports, into pinned memory behind the last event: zeros where no pass ran
        QK_TRY(qk_pinned_reserve(ctx, 64));
        if (run) {
            QK_HIP(hipMemcpyAsync(ctx->pinned, run, 32, hipMemcpyDeviceToHost, st));
        } else {
            QK_HIP(hipStreamSynchronize(st));
            memset(ctx->pinned, 0, 32);
        }
    }
    return QK_OK;
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int range_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
               int metric, float radius, qk_filter *filter, int64_t cap, int64_t *out_lims, int64_t *out_ids, float *out_dist, int mem,
               qk_timing *timing) {
    hipStream_t st = ctx->stream;
    // [lims] [ids] [distances]; cap == 0 counts only
    qk_emit_out outs[3] = {{out_lims, (size_t)(Q + 1) * 8, false},
                           {cap > 0 ? out_ids : nullptr, (size_t)cap * 8, false},
                           {cap > 0 ? out_dist : nullptr, (size_t)cap * 4, false}};
    qk_emit_call c;
    c.who = who;
    c.pipeline = "range search";
    c.label = "k_scan (range)";
    c.label_wide = "k_scan_wide (range)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.Q = Q, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.radius = radius, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 3;
    c.check = [&]() -> int {
        if (cap < 0) QK_FAIL(QK_ERR_INVALID, "%s: cap must not be negative", who);
        if (!out_lims) QK_FAIL(QK_ERR_INVALID, "%s: out_lims is null", who);
        if (cap > 0 && !out_ids) QK_FAIL(QK_ERR_INVALID, "%s: cap > 0 needs an id buffer", who);
        return QK_OK;
    };
    c.on_empty = [&]() -> int {
        if (mem == QK_MEM_HOST) out_lims[0] = 0;
        else QK_HIP(hipMemsetAsync(out_lims, 0, 8, st));
        return QK_OK;
    };
    c.device = [&](qk_emit_env &e) -> int {
        return range_device(c, e, cap, (int64_t *)outs[0].dev, (int64_t *)outs[1].dev, (float *)outs[2].dev);
    };
    c.copy_back = [&]() -> int {
        QK_HIP(hipMemcpyAsync(out_lims, outs[0].dev, outs[0].bytes, hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
        const int64_t n = std::min<int64_t>(cap, out_lims[Q]);  // the prefix that was written: nothing behind it is touched
        if (n > 0) {
            QK_HIP(hipMemcpyAsync(out_ids, outs[1].dev, (size_t)n * 8, hipMemcpyDeviceToHost, st));
            if (out_dist) QK_HIP(hipMemcpyAsync(out_dist, outs[2].dev, (size_t)n * 4, hipMemcpyDeviceToHost, st));
            QK_HIP(hipStreamSynchronize(st));
        }
        return QK_OK;
    };
    c.fill_timing = [&]() -> int {
        int64_t sc[4];
        memcpy(sc, ctx->pinned, 32);
        timing->partitions_scanned = sc[1];
        timing->scan_bytes = sc[2] * (int64_t)s->d * 4;
        return QK_OK;
    };
    return qk_emit_run(c);
}

}  // namespace

extern "C" {

int qk_range_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                    qk_filter *filter, int64_t cap, int64_t *out_lims, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_range_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_range_search: nprobe must be positive");
    return range_call("qk_range_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, metric, radius, filter, cap, out_lims, out_ids, out_dist,
                      mem, timing);
}

int qk_range_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                  qk_filter *filter, int64_t cap, int64_t *out_lims, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_range_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_range_scan: bad partition id list");
    return range_call("qk_range_scan", ctx, nullptr, s, x, Q, pids, P, 0, metric, radius, filter, cap, out_lims, out_ids, out_dist, mem,
                      timing);
}

}  // extern "C"
