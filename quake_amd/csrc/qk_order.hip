// qk_order.hip -- ordered search: per query, the k first of its range hits under (has a value, value of an attribute column in the
// direction asked, key, id) -- "the 10 cheapest items near this query" (include/quake_hip.h, "ordered search").
//
// The expensive half is the key-emission scan, run pass by pass by qk_emit_passes (qk_dense.hip) exactly as for range search and
// the facets; the hit test is facet_hit (qk_facet.h).  Every hit has a record of four words
//   c   0: the row's id has a value in the column, 1: it has none (2: padding, behind every hit)
//   v   the value as an unsigned word that orders as asked: value ^ 2^63 ascending, its complement descending; 0 for class 1
//   k   the search order's key of the pair (smaller = nearer under both metrics)
//   id  the row's id ^ 2^63 (signed ascending)
// compared lexicographically: a total order up to rows stored twice, whose records are equal and interchangeable.  Per pass:
//   k_order_partial  blockIdx.x = query * Sg + g, the decomposition of k_facet_stats in steps of 256 keys (one per thread, so that
//                    every step ends at a barrier of the whole workgroup).  A hit's record that lies below the workgroup's bound goes
//                    into an LDS buffer of B >= 2 * KP records; when fewer than 256 slots are left the buffer is sorted (bitonic, over
//                    the power of two that holds what is in it), cut to the k smallest, and the k-th becomes the bound, which every
//                    thread keeps in registers.  total and missing are counted with ballot + popcount.  At its end the workgroup
//                    writes its at most k sorted records and their number to the pass's workspace (a list has room for KP).
//   k_order_merge    one workgroup per query streams the Sg partial lists through the same buffer, bound and cut, sorts what is
//                    left and writes the outputs at q0 + q: id, the distance as qk_search reports it for the key, value, counters.
// KP is the instantiation's 64 / 256 / 1024 >= k, B its 512 / 1024 / 2048: behind a cut at least B - KP >= 448 slots are free.
// No thread waits for another, every loop is bounded, only comparisons of integers decide the result: it is a pure function of
// the store, the column and the call.
// The host side is this file's kernels plus one description: order_call states the call for qk_emit_run (qk_emit.hip), the host
// body of every entry point on the emission scan, and order_device hangs the launches above into qk_emit_device's skeleton.
#include "qk_facet.h"

#include <cstring>

namespace {

constexpr unsigned long long OR_SIGN = 0x8000000000000000ull;
constexpr int OR_STEP = 256;                    // keys per workgroup step
constexpr int OR_REC_BYTES = 24;                // a record in the workspace: v, id (8 each), k, c (4 each)
constexpr int64_t OR_PARTIAL_BYTES = 128ll << 20;  // what the partial lists of a pass may take before Sg is lowered
constexpr int OR_MAX_SG = 256;                  // partial lists one merge workgroup streams at the most

struct ORec {
    uint32_t c;
    unsigned long long v;
    uint32_t k;
    unsigned long long id;
};
__device__ __forceinline__ bool orec_less(const ORec &a, const ORec &b) {
    if (a.c != b.c) return a.c < b.c;
    if (a.v != b.v) return a.v < b.v;
    if (a.k != b.k) return a.k < b.k;
    return a.id < b.id;
}

template <int B>
struct OrderBuf {
    unsigned long long v[B], id[B];
    uint32_t k[B], c[B];
    uint32_t n;  // records in the buffer (the slot counter of a step)
    ORec bound;
};
template <int B>
__device__ __forceinline__ ORec obuf_get(const OrderBuf<B> &sb, int i) { return ORec{sb.c[i], sb.v[i], sb.k[i], sb.id[i]}; }
template <int B>
__device__ __forceinline__ void obuf_put(OrderBuf<B> &sb, int i, const ORec &r) {
    sb.c[i] = r.c;
    sb.v[i] = r.v;
    sb.k[i] = r.k;
    sb.id[i] = r.id;
}

// One step of the whole workgroup: the candidates of its 256 threads get consecutive slots per wave (one LDS atomic per wave).  The
// caller guarantees 256 free slots.  Returns the candidates of the workgroup (uniform); behind it every record is visible.
template <int B>
__device__ __forceinline__ int obuf_push(OrderBuf<B> &sb, bool cand, const ORec &r, int lane) {
    const uint64_t m = __ballot(cand);
    if (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&sb.n, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        const uint32_t at = base + __popcll(m & ((1ull << lane) - 1ull));
        if (cand && at < (uint32_t)B) obuf_put(sb, (int)at, r);
    }
    return __syncthreads_count(cand ? 1 : 0);
}

// The n records of the buffer (uniform, n <= B, all visible) sorted ascending, cut to the `keep` smallest (keep = the call's k);
// the bound becomes the keep-th or, with fewer, the padding record.  Returns min(n, keep); ends behind a barrier.
template <int B>
__device__ __forceinline__ int obuf_compact(OrderBuf<B> &sb, int n, int keep, int tid) {
    int n2 = 2;
    while (n2 < n) n2 <<= 1;  // (<= B: B is a power of two)
    for (int i = n + tid; i < n2; i += 256) obuf_put(sb, i, ORec{2u, 0ull, 0u, 0ull});
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;
                const ORec a = obuf_get(sb, i), b = obuf_get(sb, o);
                const bool up = (i & k) == 0;
                if (up ? orec_less(b, a) : orec_less(a, b)) {
                    obuf_put(sb, i, b);
                    obuf_put(sb, o, a);
                }
            }
            __syncthreads();
        }
    const int m = min(n, keep);
    if (tid == 0) {
        sb.n = (uint32_t)m;
        sb.bound = n >= keep ? obuf_get(sb, keep - 1) : ORec{2u, 0ull, 0u, 0ull};
    }
    __syncthreads();
    return m;
}

struct OrderParams {
    FacetParams F;       // keys, segments, mask, has[0] / rowval[0], total, missing, nq, P, Sg, the key interval (tables unused)
    const int64_t *ids;  // the arena's ids
    int desc, missing_last, k;
    // the partial lists of the pass: list b = query * Sg + g holds pcnt[b] <= k <= KP sorted records at b * KP
    unsigned long long *pv, *pid;
    uint32_t *pk, *pc, *pcnt;
};

template <int KP, int B>
__global__ __launch_bounds__(256) void k_order_partial(OrderParams S) {
    static_assert(B >= 2 * KP && B - KP >= OR_STEP && (B & (B - 1)) == 0, "a step of 256 candidates fits behind every cut");
    __shared__ OrderBuf<B> sb;
    const FacetParams &F = S.F;
    const int64_t q = blockIdx.x / F.Sg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t *pbase = F.pair_base + q * F.P;
    const int64_t *qpids = F.pids ? F.pids + q * F.P : nullptr;
    const int64_t beg = pbase[0], end = pbase[F.P];
    const int64_t first = beg + (int64_t)(blockIdx.x - q * F.Sg) * FC_SLICE;
    if (first >= end) {  // (the whole workgroup: it has no slice)
        if (tid == 0) S.pcnt[blockIdx.x] = 0u;
        return;
    }
    if (tid == 0) sb.n = 0u;
    __syncthreads();
    ORec bound{2u, 0ull, 0u, 0ull};
    int n = 0;                             // records in the buffer (uniform)
    uint32_t n_total = 0, n_missing = 0;   // (wave-uniform)
    for (int64_t s0 = first; s0 < end; s0 += (int64_t)F.Sg * FC_SLICE) {
        const int64_t lim = min(end, s0 + FC_SLICE);
        for (int64_t w0 = s0; w0 < lim; w0 += OR_STEP) {  // (uniform over the workgroup)
            const int64_t pos = w0 + tid;
            int64_t row;
            const bool hit = facet_hit(F, pbase, qpids, pos, lim, &row);
            const uint64_t hm = __ballot(hit);
            const bool has = hit && ((F.has[0][row >> 4] >> (row & 15)) & 1);
            n_total += __popcll(hm);
            n_missing += __popcll(hm) - __popcll(__ballot(has));
            bool cand = hit && (has || S.missing_last);
            ORec r{has ? 0u : 1u, 0ull, 0u, 0ull};
            if (cand) {
                if (has) {
                    const unsigned long long u = (unsigned long long)F.rowval[0][row] ^ OR_SIGN;
                    r.v = S.desc ? ~u : u;
                }
                r.k = F.keys[pos];
                // the id is read only where the three words in front of it do not decide against the record
                cand = r.c < bound.c || (r.c == bound.c && (r.v < bound.v || (r.v == bound.v && r.k <= bound.k)));
                if (cand) {
                    r.id = (unsigned long long)S.ids[row] ^ OR_SIGN;
                    cand = orec_less(r, bound);
                }
            }
            n += obuf_push(sb, cand, r, lane);
            if (n > B - OR_STEP) {
                n = obuf_compact<B>(sb, n, S.k, tid);
                bound = sb.bound;
            }
        }
    }
    if (n > 0) n = obuf_compact<B>(sb, n, S.k, tid);
    const int64_t at = (int64_t)blockIdx.x * KP;
    for (int i = tid; i < n; i += 256) {
        S.pv[at + i] = sb.v[i];
        S.pid[at + i] = sb.id[i];
        S.pk[at + i] = sb.k[i];
        S.pc[at + i] = sb.c[i];
    }
    if (tid == 0) S.pcnt[blockIdx.x] = (uint32_t)n;
    if (lane == 0) {
        if (n_total) atomicAdd(&F.total[q], n_total);
        if (n_missing) atomicAdd(&F.missing[q], n_missing);
    }
}

struct OrderMergeParams {
    const unsigned long long *pv, *pid;
    const uint32_t *pk, *pc, *pcnt;
    const uint32_t *total, *missing;  // [nq]
    int64_t q0;                       // the pass's queries are q0 .. of the call's
    int Sg, k, desc, metric, sqrt_l2;
    int64_t *out_ids;                 // [Q][k]
    float *out_dist;                  // [Q][k] or nullptr
    int64_t *out_values;              // [Q][k] or nullptr
    int64_t *out_count, *out_missing, *out_total;  // [Q] or nullptr
};

// blockIdx.x = query of the pass
template <int KP, int B>
__global__ __launch_bounds__(256) void k_order_merge(OrderMergeParams M) {
    __shared__ OrderBuf<B> sb;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) sb.n = 0u;
    __syncthreads();
    ORec bound{2u, 0ull, 0u, 0ull};
    int n = 0;
    for (int g = 0; g < M.Sg; g++) {
        const int64_t b = q * M.Sg + g;
        const int cnt = min((int)M.pcnt[b], M.k);  // (uniform; a list holds at most k records)
        for (int i0 = 0; i0 < cnt; i0 += OR_STEP) {
            const int i = i0 + tid;
            bool cand = i < cnt;
            ORec r{2u, 0ull, 0u, 0ull};
            if (cand) {
                const int64_t at = b * KP + i;
                r = ORec{M.pc[at], M.pv[at], M.pk[at], M.pid[at]};
                cand = orec_less(r, bound);
            }
            n += obuf_push(sb, cand, r, lane);
            if (n > B - OR_STEP) {
                n = obuf_compact<B>(sb, n, M.k, tid);
                bound = sb.bound;
            }
        }
    }
    if (n > 0) n = obuf_compact<B>(sb, n, M.k, tid);
    const int64_t oq = M.q0 + q;
    for (int j = tid; j < M.k; j += 256) {
        const bool real = j < n;
        const bool has = real && sb.c[j] == 0u;
        M.out_ids[oq * M.k + j] = real ? (int64_t)(sb.id[j] ^ OR_SIGN) : -1;
        if (M.out_values) {
            const unsigned long long u = has ? (M.desc ? ~sb.v[j] : sb.v[j]) : OR_SIGN;
            M.out_values[oq * M.k + j] = (int64_t)(u ^ OR_SIGN);
        }
        if (M.out_dist) {
            float od;
            if (M.metric == QK_METRIC_L2) {
                const float d2 = __uint_as_float(real ? sb.k[j] : 0x7F800000u);
                od = (M.sqrt_l2 && real) ? sqrtf(d2) : d2;
            } else {
                od = real ? ip_from_ord(sb.k[j]) : -INFINITY;
            }
            M.out_dist[oq * M.k + j] = od;
        }
    }
    if (tid == 0) {
        const int64_t tot = M.total[q], mis = M.missing[q];
        if (M.out_count) M.out_count[oq] = tot - mis;
        if (M.out_missing) M.out_missing[oq] = mis;
        if (M.out_total) M.out_total[oq] = tot;
    }
}

__global__ __launch_bounds__(256) void k_order_fill(float *p, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

struct OrderOut {
    int64_t *ids;
    float *dist;
    int64_t *values, *count, *missing, *total;
};

// the device half; o: the call's outputs on the device (nullptr: not wanted)
int order_device(const qk_emit_call &c, qk_emit_env &e, int desc, int missing_last, int k, const OrderOut &o) {
    qk_store *s = c.s;
    const qk_scan_args &a = e.a;
    const int64_t Q = a.Q;
    const int P = e.P;
    hipStream_t st = c.ctx->stream;
    qk_emit_stages g;
    g.pad = [&]() -> int {  // no hits: padding and zeros
        QK_HIP(hipMemsetAsync(o.ids, 0xFF, (size_t)Q * k * 8, st));
        if (o.values) QK_HIP(hipMemsetAsync(o.values, 0, (size_t)Q * k * 8, st));
        if (o.dist)
            hipLaunchKernelGGL(k_order_fill, dim3((unsigned)((Q * k + 255) / 256)), dim3(256), 0, st, o.dist, Q * k,
                               a.metric == QK_METRIC_L2 ? INFINITY : -INFINITY);
        for (int64_t *p : {o.count, o.missing, o.total})
            if (p) QK_HIP(hipMemsetAsync(p, 0, (size_t)Q * 8, st));
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    const int KP = k <= 64 ? 64 : k <= 256 ? 256 : 1024;
    // this pipeline's bytes of the call's buffer, sized for the largest pass: [total] [missing] [pcnt] [pv] [pid] [pk] [pc]
    int64_t S = 0, Sg_cap = 1;
    size_t o_missing = 0, o_pcnt = 0, o_pv = 0, o_pid = 0, o_pk = 0, o_pc = 0;
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        S = (per_query_ub + FC_SLICE - 1) / FC_SLICE;
        // the partial lists: Sg of KP records per query.  A large k lowers Sg (down to 1) before it shortens the pass, and the pass
        // is shortened only where one list per query would exceed QK_GROUPED_PASS_BYTES
        const int64_t lbytes = (int64_t)KP * OR_REC_BYTES + 4;
        *qc = std::max<int64_t>(1, std::min<int64_t>(*qc, QK_GROUPED_PASS_BYTES / (lbytes + 8)));
        Sg_cap = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S, OR_MAX_SG), OR_PARTIAL_BYTES / (*qc * lbytes)));
        if (*qc * Sg_cap > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "ordered search: Q too large");
        const int64_t nl = *qc * Sg_cap;
        o_missing = qk_al256((size_t)*qc * 4);
        o_pcnt = o_missing + qk_al256((size_t)*qc * 4);
        o_pv = o_pcnt + qk_al256((size_t)nl * 4);
        o_pid = o_pv + qk_al256((size_t)nl * KP * 8);
        o_pk = o_pid + qk_al256((size_t)nl * KP * 8);
        o_pc = o_pk + qk_al256((size_t)nl * KP * 4);
        *extra_bytes = o_pc + qk_al256((size_t)nl * KP * 4);
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        QK_HIP(hipMemsetAsync(p.extra, 0, o_pcnt, st));  // total and missing; every partial list's counter is written by its workgroup
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        OrderParams T;
        FacetParams &F = T.F;
        facet_params_fill(F, p, s, e.mask, c.cols, 1, e.key_lo, e.key_hi, P, S);
        F.total = (uint32_t *)p.extra;
        F.missing = (uint32_t *)(p.extra + o_missing);
        F.Sg = qk_emit_sg(std::min(S, Sg_cap), p.nq);  // no more partial lists per query than the workspace was planned for
        T.ids = s->ids;
        T.desc = desc;
        T.missing_last = missing_last;
        T.k = k;
        T.pcnt = (uint32_t *)(p.extra + o_pcnt);
        T.pv = (unsigned long long *)(p.extra + o_pv);
        T.pid = (unsigned long long *)(p.extra + o_pid);
        T.pk = (uint32_t *)(p.extra + o_pk);
        T.pc = (uint32_t *)(p.extra + o_pc);
        OrderMergeParams M;
        M.pv = T.pv;
        M.pid = T.pid;
        M.pk = T.pk;
        M.pc = T.pc;
        M.pcnt = T.pcnt;
        M.total = F.total;
        M.missing = F.missing;
        M.q0 = p.q0;
        M.Sg = F.Sg;
        M.k = k;
        M.desc = desc;
        M.metric = a.metric;
        M.sqrt_l2 = a.sqrt_l2 ? 1 : 0;
        M.out_ids = o.ids;
        M.out_dist = o.dist;
        M.out_values = o.values;
        M.out_count = o.count;
        M.out_missing = o.missing;
        M.out_total = o.total;
        const dim3 gp((unsigned)(p.nq * F.Sg)), gm((unsigned)p.nq);
#define OR_LAUNCH(KP_, B_)                                                               \
    do {                                                                                 \
        hipLaunchKernelGGL((k_order_partial<KP_, B_>), gp, dim3(256), 0, st, T);         \
        hipLaunchKernelGGL((k_order_merge<KP_, B_>), gm, dim3(256), 0, st, M);           \
    } while (0)
        if (KP == 64) OR_LAUNCH(64, 512);
        else if (KP == 256) OR_LAUNCH(256, 1024);
        else OR_LAUNCH(1024, 2048);
#undef OR_LAUNCH
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    return qk_emit_device(c, e, g);
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int order_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
               int metric, float radius, qk_filter *filter, qk_attr *order_by, int flags, int k, const OrderOut &out, int mem,
               qk_timing *timing) {
    // [ids] [values] [dist] [count] [missing] [total]
    const size_t b8 = (size_t)Q * k * 8, bq = (size_t)Q * 8;
    qk_emit_out outs[6] = {{out.ids, b8, true},     {out.values, b8, false},  {out.dist, (size_t)Q * k * 4, false},
                           {out.count, bq, false}, {out.missing, bq, false}, {out.total, bq, false}};
    qk_emit_call c;
    c.who = who;
    c.pipeline = "ordered search";
    c.label = "k_scan (order)";
    c.label_wide = "k_scan_wide (order)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.Q = Q, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.radius = radius, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 6;
    c.check = [&]() -> int {
        if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
        if (k > QK_MAX_ORDER_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_ORDER_K=%d", who, k, QK_MAX_ORDER_K);
        if (flags & ~(QK_ORDER_DESC | QK_ORDER_MISSING_LAST)) QK_FAIL(QK_ERR_INVALID, "%s: unknown flags %d", who, flags);
        if (!order_by) QK_FAIL(QK_ERR_INVALID, "%s: order_by is null", who);
        c.cols[0] = order_by->d.get();
        c.n_cols = 1;
        if (c.cols[0]->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "%s: the order column belongs to another store", who);
        return QK_OK;
    };
    c.device = [&](qk_emit_env &e) -> int {
        const OrderOut dv{(int64_t *)outs[0].dev, (float *)outs[2].dev,   (int64_t *)outs[1].dev,
                          (int64_t *)outs[3].dev, (int64_t *)outs[4].dev, (int64_t *)outs[5].dev};
        return order_device(c, e, (flags & QK_ORDER_DESC) ? 1 : 0, (flags & QK_ORDER_MISSING_LAST) ? 1 : 0, k, dv);
    };
    return qk_emit_run(c);
}

}  // namespace

extern "C" {

int qk_order_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                    qk_filter *filter, qk_attr *order_by, int flags, int k, int64_t *out_ids, float *out_dist, int64_t *out_values,
                    int64_t *out_count, int64_t *out_missing, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_order_search: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_order_search: nprobe must be positive");
    const OrderOut out{out_ids, out_dist, out_values, out_count, out_missing, out_total};
    return order_call("qk_order_search", ctx, parent, s, x, Q, nullptr, 0, nprobe, metric, radius, filter, order_by, flags, k, out, mem,
                     timing);
}

int qk_order_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                  qk_filter *filter, qk_attr *order_by, int flags, int k, int64_t *out_ids, float *out_dist, int64_t *out_values,
                  int64_t *out_count, int64_t *out_missing, int64_t *out_total, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_order_scan: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_order_scan: bad partition id list");
    const OrderOut out{out_ids, out_dist, out_values, out_count, out_missing, out_total};
    return order_call("qk_order_scan", ctx, nullptr, s, x, Q, pids, P, 0, metric, radius, filter, order_by, flags, k, out, mem, timing);
}

}  // extern "C"
