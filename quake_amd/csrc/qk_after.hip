// qk_after.hip -- paged search: continue a search behind a (key, id) cursor (include/quake_hip.h, "paged search").
//
// Results are totally ordered by (integer key, id).  A cursor is a position in that order; the page behind it is the k smallest
// candidates whose (key, id) is greater.  The test is one more condition in the epilogue of the filtered tile form, where the
// row's key and id are in registers anyway: k_scan_after (here) and k_scan_wide_after (qk_scan_wide.hip) compile the filtered
// scan bodies once more with QK_SCAN_AFTER.  The plan is the filtered call's -- no bound is learnt from a row nobody tested: the
// k nearest rows of page two all lie BEFORE the cursor, and a bound seeded from them would drop the whole page.  A call without
// a filter runs the same kernels under a deny-nothing filter kept on the store (qk_store::allow_all).
//
// The next cursor is written on the device by k_next_cursor behind the merge: the id of the query's k-th result and the key the
// merge compared for it, read back from the scan's records -- not re-derived from the reported distance, which has been through
// sqrt (not injective in fp32).
#include "qk_internal.h"
#include "qk_device.h"
#include "qk_scan_types.h"
#include "qk_scan_opts.h"

#include <algorithm>
#include <mutex>

// ---- the scan kernel ---------------------------------------------------------------------------------------------------------------
// k_scan_filt's body plus the cursor (see qk_scan_body.inc).  Its own kernel in its own translation unit: no instantiation of
// k_scan, k_scan_filt or k_scan_filtq changes.
template <int DB, int MAXCH, bool L2>
__global__ __launch_bounds__(256) void k_scan_after(ScanParams P) {
    constexpr int MODE = 0;
#define QK_SCAN_FILT 1
#define QK_SCAN_AFTER
#include "qk_scan_body.inc"
#undef QK_SCAN_AFTER
#undef QK_SCAN_FILT
}

template <int DB, int MAXCH>
static int launch_scan_after(dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
    if (sp.metric == QK_METRIC_L2) {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_after<DB, MAXCH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_after<DB, MAXCH, true>), grid, block, lds, st, sp);
    } else {
        QK_HIP(hipFuncSetAttribute((const void *)k_scan_after<DB, MAXCH, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_scan_after<DB, MAXCH, false>), grid, block, lds, st, sp);
    }
    return QK_OK;
}

// the instantiation table of k_scan_filt (launch_scan, qk_scan.hip)
int qk_launch_scan_after(int db, int maxch, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ScanParams &sp) {
#define QK_CASEA(D, M) \
    if (db == D && maxch == M) return launch_scan_after<D, M>(grid, block, lds, st, sp);
    QK_CASEA(1, 1) QK_CASEA(1, 2) QK_CASEA(1, 4) QK_CASEA(1, 8) QK_CASEA(2, 1) QK_CASEA(2, 2) QK_CASEA(2, 4) QK_CASEA(2, 8)
    QK_CASEA(4, 1) QK_CASEA(4, 2) QK_CASEA(4, 4) QK_CASEA(4, 8) QK_CASEA(8, 1) QK_CASEA(8, 2) QK_CASEA(8, 4) QK_CASEA(8, 8)
    QK_CASEA(16, 1) QK_CASEA(16, 2) QK_CASEA(16, 4) QK_CASEA(16, 8)
#undef QK_CASEA
    QK_FAIL(QK_ERR_UNSUPPORTED, "no paged scan kernel for DB=%d MAXCH=%d", db, maxch);
}

// ---- the next cursor ---------------------------------------------------------------------------------------------------------------
// One wave per query behind the merge.  The row's last entry says whether it is full: ids are non-negative, padding is -1 and sits
// behind the results.  A full row's cursor is (key, id) of that entry; the key is looked up where the merge found it -- in the
// records of the query's pairs (the slot line's records, then the chain: k_merge's walk, read only), by the id, which is unique.
// A row with fewer than k results exhausted the probed lists: the cursor no row lies behind.
__global__ __launch_bounds__(64) void k_next_cursor(MergeParams M, const int64_t *out_ids, uint32_t *next_key, int64_t *next_id) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int k = M.k;
    const int64_t want = out_ids[q * k + k - 1];
    uint32_t key = 0xFFFFFFFFu;  // (never the key of a result)
    if (want >= 0) {
        auto look = [&](int rec) -> bool {  // (rec is the same in every lane)
            const int n = min(M.rec_hdr[rec].y, k);
            for (int e0 = 0; e0 < n; e0 += 64) {
                const int e = e0 + lane;
                if (e < n && M.rec_id[(int64_t)rec * k + e] == want) key = M.rec_ord[(int64_t)rec * k + e];
                if (__ballot(key != 0xFFFFFFFFu)) return true;
            }
            return false;
        };
        bool found = false;
        for (int r = 0; r < M.P && !found; r++) {
            const int64_t pair = q * M.P + r;
            const int nrecs = M.pair_slots[pair * QK_SLOTS];
            const int ns = min(nrecs, QK_SLOTS - 1);
            for (int i = 0; i < ns && !found; i++) {
                const int rec = M.pair_slots[pair * QK_SLOTS + 1 + i];
                if (rec >= 0 && rec < M.max_recs) found = look(rec);
            }
            if (nrecs > QK_SLOTS - 1) {
                int rec = M.pair_head[pair];
                while (!found && rec >= 0 && rec < M.max_recs) {
                    found = look(rec);
                    rec = M.rec_hdr[rec].x;
                }
            }
        }
        const uint64_t who = __ballot(key != 0xFFFFFFFFu);
        key = who ? (uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll((unsigned long long)who) - 1) : 0xFFFFFFFFu;
    }
    if (lane == 0) {
        next_key[q] = key;
        next_id[q] = key != 0xFFFFFFFFu ? want : INT64_MAX;
    }
}

int qk_launch_next_cursor(qk_ctx *ctx, const MergeParams &mp, int64_t Q, const int64_t *out_ids, uint32_t *next_key, int64_t *next_id) {
    if (Q <= 0) return QK_OK;
    hipLaunchKernelGGL(k_next_cursor, dim3((unsigned)Q), dim3(64), 0, ctx->stream, mp, out_ids, next_key, next_id);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
namespace {

int after_run(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
              int k, int metric, const uint32_t *after_key, const int64_t *after_id, qk_filter *filter, int64_t *out_ids, float *out_dist,
              uint32_t *next_key, int64_t *next_id, int mem, qk_timing *timing) {
    if (!ctx || !s || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if ((after_key == nullptr) != (after_id == nullptr))
        QK_FAIL(QK_ERR_INVALID, "%s: after_key and after_id go together (both NULL: the start cursor for every query)", who);
    if ((next_key == nullptr) != (next_id == nullptr)) QK_FAIL(QK_ERR_INVALID, "%s: next_key and next_id go together", who);
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "%s: k must be positive", who);
    if (k > QK_MAX_K)
        QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d (a page is one fused top-k; ask for the rest with the next cursor)", who, k, QK_MAX_K);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    QK_HIP(hipSetDevice(ctx->device));
    if (Q <= 0) {
        if (timing) *timing = qk_timing{};
        return QK_OK;
    }
    // no filter: the store's own deny-nothing filter (made once; qk_filter_ensure keeps its mask current like any other's)
    // (made under a lock: the first such calls of two threads on one store, through different contexts, make it once)
    if (!filter) {
        static std::mutex allow_all_lock;
        std::lock_guard<std::mutex> guard(allow_all_lock);
        if (!s->allow_all) QK_TRY(qk_filter_create(s, nullptr, 0, QK_FILTER_DENY, QK_MEM_HOST, &s->allow_all));
        filter = s->allow_all;
    }
    // the cursors on the device: [Q] keys | [Q] ids coming in, the same going out
    const size_t bk = qk_al256((size_t)Q * sizeof(uint32_t)), bi = qk_al256((size_t)Q * sizeof(int64_t));
    const bool host = mem == QK_MEM_HOST;
    qk_cursors cu;
    if (host || !after_key) {
        const size_t need = 2 * (bk + bi);
        if (need > ctx->after_cap) {
            // (a scan in flight may still read the old buffer: hipFree waits for the device)
            if (ctx->after_buf) QK_HIP(hipFree(ctx->after_buf));
            ctx->after_buf = nullptr;
            ctx->after_cap = 0;
            if (hipMalloc((void **)&ctx->after_buf, need + need / 4) != hipSuccess) {
                (void)hipGetLastError();
                QK_FAIL(QK_ERR_OOM, "%s: no device memory for the cursors of %lld queries", who, (long long)Q);
            }
            ctx->after_cap = need + need / 4;
        }
    }
    char *b = ctx->after_buf;
    if (!after_key) {  // the start cursor (0, -1): below every row
        QK_HIP(hipMemsetAsync(b, 0, (size_t)Q * sizeof(uint32_t), ctx->stream));
        QK_HIP(hipMemsetAsync(b + bk, 0xFF, (size_t)Q * sizeof(int64_t), ctx->stream));
        cu.after_key = (const uint32_t *)b;
        cu.after_id = (const int64_t *)(b + bk);
    } else if (host) {
        // (pageable source: copied out when the call returns)
        QK_HIP(hipMemcpyAsync(b, after_key, (size_t)Q * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        QK_HIP(hipMemcpyAsync(b + bk, after_id, (size_t)Q * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        cu.after_key = (const uint32_t *)b;
        cu.after_id = (const int64_t *)(b + bk);
    } else {
        cu.after_key = after_key;
        cu.after_id = after_id;
    }
    if (next_key) {
        cu.next_key = host ? (uint32_t *)(b + bk + bi) : next_key;
        cu.next_id = host ? (int64_t *)(b + 2 * bk + bi) : next_id;
    }
    QK_TRY(qk_run_search(ctx, parent, s, x, Q, pids, P, nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, nullptr, filter, nullptr,
                         nullptr, &cu));
    if (host && next_key) {  // (the call has synchronised for the results; the cursors follow them)
        QK_HIP(hipMemcpyAsync(next_key, cu.next_key, (size_t)Q * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        QK_HIP(hipMemcpyAsync(next_id, cu.next_id, (size_t)Q * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        QK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return QK_OK;
}

}  // namespace

extern "C" {

int qk_search_after(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                    const uint32_t *after_key, const int64_t *after_id, qk_filter *filter, int64_t *out_ids, float *out_dist,
                    uint32_t *next_key, int64_t *next_id, int mem, qk_timing *timing) {
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_after: nprobe must be positive");
    return after_run("qk_search_after", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, metric, after_key, after_id, filter, out_ids, out_dist,
                     next_key, next_id, mem, timing);
}

int qk_scan_after(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                  const uint32_t *after_key, const int64_t *after_id, qk_filter *filter, int64_t *out_ids, float *out_dist, uint32_t *next_key,
                  int64_t *next_id, int mem, qk_timing *timing) {
    if (P <= 0 || !pids) QK_FAIL(QK_ERR_INVALID, "qk_scan_after: bad partition id list");
    if (s && mem == QK_MEM_HOST && Q > 0) {
        for (int64_t i = 0; i < Q * (int64_t)P; i++) {
            const int64_t p = pids[i];
            if (p < 0) continue;
            if (p >= (int64_t)s->parts.size() || !s->parts[p].present)
                QK_FAIL(QK_ERR_NOT_FOUND, "List does not exist in get_codes (list %lld)", (long long)p);
        }
    }
    return after_run("qk_scan_after", ctx, nullptr, s, x, Q, pids, P, 0, k, metric, after_key, after_id, filter, out_ids, out_dist, next_key,
                     next_id, mem, timing);
}

}  // extern "C"
