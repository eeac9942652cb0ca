// qk_filter.hip -- filtered search: the filter object of the C ABI (include/quake_hip.h, "filtered search") and the kernel that
// turns its id set into the row mask the scan kernels read (k_scan_filt, qk_scan.hip; k_scan_wide_filt, qk_scan_wide.hip).
//
// A filter is a set of ids S and a mode (allow / deny).  What the scan needs is a statement about ROWS: the lists of a store are
// extents of 16-row tiles of its arena (qk_part::row_off and cap are multiples of 16), so one 16-bit word per arena tile says which
// rows of the tile are candidates -- cap_rows / 8 bytes, 1.25 MB at 10M rows.  The word of a tile has one writer (16 lanes of one
// wave combine their bits with a ballot), so the build needs no atomics on the mask; rows behind a list's size and abandoned
// extents keep the 0 of the memset in front of the kernel.
//
// The mask is stamped with the store's (uid, version, cap_rows): every operation that changes which id sits in which arena row --
// append, in-place removal (swap with last), list relocation, both arena compactions, qk_store_refine_lists (remove + re-add),
// list creation / removal, bulk builds -- sets qk_store::table_dirty, and the table sync in front of every scan turns that into a
// new version.  qk_filter_ensure compares the stamp after that sync and re-derives the mask from the ids when it differs: a filter
// is defined by ids and stays correct whatever moves rows.
//
// A filter is of one of two kinds (qk_attr.h): an id set, as above, or a PREDICATE over attribute columns (qk_attr.hip), whose
// mask k_filter_build_where derives and whose stamp also holds the version of every column it names.  Everything behind the mask
// -- the scans, the per-query table, the union -- is the same for both.
#include "qk_attr.h"

#include <algorithm>
#include <atomic>
#include <vector>

namespace {

struct FilterBuildParams {
    const int64_t *ids;      // arena ids
    const int64_t *pt_off;   // [npids] first arena row of every list
    const int32_t *pt_size;  // [npids] rows, -1 = absent
    const int64_t *set;      // [n] sorted id set
    int64_t n;
    int deny;
    uint16_t *mask;
    int64_t mask_words;
    unsigned long long *allowed;
};

// blockIdx.x = list, blockIdx.y strides over its chunks of 16 tiles (one tile per 16 lanes of the 256-thread block)
__global__ __launch_bounds__(256) void k_filter_build(FilterBuildParams F) {
    const int p = blockIdx.x;
    const int size = F.pt_size[p];
    if (size <= 0) return;
    const int64_t row_off = F.pt_off[p];
    const int ntl = (size + 15) >> 4;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int sub = threadIdx.x >> 4;  // tile of the chunk
    unsigned long long mine = 0;
    for (int t0 = blockIdx.y * 16; t0 < ntl; t0 += gridDim.y * 16) {
        const int tile = t0 + sub;
        const int row = tile * 16 + j;
        bool bit = false;
        if (tile < ntl && row < size) {
            const int64_t id = F.ids[row_off + row];
            int64_t lo = 0, hi = F.n;  // first element >= id
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (F.set[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            const bool found = lo < F.n && F.set[lo] == id;
            bit = F.deny ? !found : found;
        }
        const uint64_t b = __ballot(bit);
        const uint32_t word = (uint32_t)((b >> (16 * (lane >> 4))) & 0xFFFFull);
        const int64_t w = (row_off >> 4) + tile;
        if (j == 0 && tile < ntl && w < F.mask_words) {
            F.mask[w] = (uint16_t)word;
            mine += __popc(word);
        }
    }
    // one atomic per wave
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane == 0 && mine) atomicAdd(F.allowed, mine);
}

// the mask sized for the store and cleared, the counter cleared, on ctx's stream
int filter_build_prepare(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    const int64_t words = s->cap_rows / 16;
    if (words > f->mask_words || !f->mask) {
        // (the old mask may still be read by a scan in flight on some context: hipFree waits for the device)
        if (f->mask) QK_HIP(hipFree(f->mask));
        f->mask = nullptr;
        f->mask_words = 0;
        const int64_t cap = std::max<int64_t>(words + words / 4, 64);
        if (hipMalloc((void **)&f->mask, (size_t)cap * sizeof(uint16_t)) != hipSuccess) {
            (void)hipGetLastError();
            QK_FAIL(QK_ERR_OOM, "qk_filter: no memory for a row mask of %lld tiles", (long long)cap);
        }
        f->mask_words = cap;
    }
    hipStream_t st = ctx->stream;
    // a build on another context than the last one: behind that one's (its scans may still read the mask it wrote)
    if (f->built_ctx && f->built_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, f->built_ev, 0));
    QK_HIP(hipMemsetAsync(f->mask, 0, (size_t)f->mask_words * sizeof(uint16_t), st));
    QK_HIP(hipMemsetAsync(f->d_allowed, 0, sizeof(unsigned long long), st));
    return QK_OK;
}

int filter_build_ids(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    hipStream_t st = ctx->stream;
    const int64_t npids = (int64_t)s->parts.size();
    if (npids > 0 && s->ntotal > 0) {
        FilterBuildParams F;
        F.ids = s->ids;
        F.pt_off = s->d_off;
        F.pt_size = s->d_size;
        F.set = f->d_ids;
        F.n = f->n_ids;
        F.deny = f->mode == QK_FILTER_DENY ? 1 : 0;
        F.mask = f->mask;
        F.mask_words = f->mask_words;
        F.allowed = f->d_allowed;
        const int64_t max_tiles = (std::max<int64_t>(1, s->max_size) + 15) / 16;
        const unsigned gy = (unsigned)std::min<int64_t>(65535, (max_tiles + 15) / 16);
        hipLaunchKernelGGL(k_filter_build, dim3((unsigned)npids, gy), dim3(256), 0, st, F);
        QK_HIP(hipGetLastError());
    }
    return QK_OK;
}

int filter_build(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    QK_TRY(filter_build_prepare(ctx, s, f));
    // (a predicate's clauses are stamped with their columns' versions even when there is no row to look at)
    if (f->kind == QK_FILTER_KIND_WHERE) QK_TRY(qk_launch_filter_build_where(ctx, s, f));
    else QK_TRY(filter_build_ids(ctx, s, f));
    hipStream_t st = ctx->stream;
    QK_HIP(hipEventRecord(f->built_ev, st));
    if (f->built) f->rebuilds++;
    f->built = true;
    f->counts_built = false;  // (adaptive probing: re-derived by the next call that needs them)
    f->built_ctx = ctx;
    f->version = s->version;
    f->cap_rows = s->cap_rows;
    return QK_OK;
}

// the mask of a filter of this store and device, current for the store's table (the caller has synced it)
int filter_current(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    if (!f->built || f->version != s->version || f->cap_rows != s->cap_rows ||
        (f->kind == QK_FILTER_KIND_WHERE && !qk_filter_where_current(f))) {
        QK_TRY(filter_build(ctx, s, f));
    } else if (f->built_ctx != ctx) {
        QK_HIP(hipStreamWaitEvent(ctx->stream, f->built_ev, 0));  // the build ran on another context's stream
    }
    return QK_OK;
}

int filter_belongs(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    if (!f || !s) QK_FAIL(QK_ERR_INVALID, "filtered search: null filter");
    if (f->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "filtered search: the filter was made for another store");
    if (f->device != ctx->device) QK_FAIL(QK_ERR_INVALID, "filtered search: the filter lives on device %d, the context on %d", f->device, ctx->device);
    return QK_OK;
}

// ---- one filter per query: the OR of the call's F masks ------------------------------------------------------------------------
// The scan of a per-query call walks the tiles that hold a candidate of ANY of its filters (ScanParams::mask) and tests every row
// against its own query's word (ScanParams::qmasks): the first is this kernel's output.  One lane per word, a loop over the F
// masks -- the 64 lanes of a wave read 128 consecutive bytes of each -- plain vector stores, no atomics.
__global__ __launch_bounds__(256) void k_filter_union(const uint16_t *const *masks, int F, int64_t words, uint16_t *out) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint32_t acc = 0;
    for (int f = 0; f < F; f++) acc |= (uint32_t)masks[f][w];
    out[w] = (uint16_t)acc;
}

// ---- adaptive probing: candidates per list, and the cut of every query's ranked lists ---------------------------------------------
// counts[p] = candidates of list number p: the popcount of the mask words of its extent (rows behind its size keep the 0 of the
// build's memset; an absent or empty list has 0).  One wave per list, lanes on consecutive 16-bit words, a shuffle reduction:
// every counts[p] has one writer.
__global__ __launch_bounds__(256) void k_filter_list_counts(const uint16_t *mask, int64_t mask_words, const int64_t *pt_off,
                                                            const int32_t *pt_size, int npids, int32_t *counts) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npids) return;  // (the whole wave)
    const int size = pt_size[p];
    int n = 0;
    if (size > 0) {
        const int64_t w0 = pt_off[p] >> 4;
        const int ntl = (size + 15) >> 4;
        for (int t = lane; t < ntl; t += 64) {
            const int64_t w = w0 + t;
            if (w < mask_words) n += __popc((uint32_t)mask[w]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if (lane == 0) counts[p] = n;
}

// One wave per query over its row of M ranked list numbers: nprobed = the smallest t in [n0, M] whose first t lists hold
// min_candidates candidates of the query's filter (M if none does), -1 over the rest of the row.  Chunks of 64 lists: a gather of
// counts[pid] (-1 and numbers the store does not know: 0), an inclusive prefix sum over the wave carried from chunk to chunk, a
// ballot for the first lane that is there.  A qfilter value outside [0, F) is checked before the table is indexed: nprobed = 0.
__global__ __launch_bounds__(256) void k_probe_trim(int64_t *pids, int64_t Q, int M, int n0, long long minc, const int32_t *counts,
                                                    const int32_t *const *ctable, const int32_t *qfilter, int F, int npids,
                                                    int32_t *nprobed) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;  // (the whole wave)
    const int32_t *cnt = counts;
    bool live = true;
    if (ctable) {
        const int f = qfilter[q];
        live = (unsigned)f < (unsigned)F;
        cnt = live ? ctable[f] : nullptr;
    }
    int64_t *row = pids + q * (int64_t)M;
    int t = live ? M : 0;
    if (live) {
        long long carry = 0;
        for (int c0 = 0; c0 < M; c0 += 64) {
            const int i = c0 + lane;
            long long v = 0;
            if (i < M) {
                const int64_t p = row[i];
                if (p >= 0 && p < (int64_t)npids) v = cnt[p];
            }
            for (int off = 1; off < 64; off <<= 1) {
                const long long u = __shfl_up(v, off);
                if (lane >= off) v += u;
            }
            v += carry;
            const uint64_t b = __ballot(i < M && i + 1 >= n0 && v >= minc);
            if (b) {  // (the same for every lane)
                t = c0 + __ffsll((unsigned long long)b);
                break;
            }
            carry = __shfl(v, 63);
        }
    }
    for (int i = t + lane; i < M; i += 64) row[i] = -1;
    if (lane == 0 && nprobed) nprobed[q] = t;
}

}  // namespace

int qk_filter_counts_ensure(qk_ctx *ctx, qk_store *s, qk_filter *f, const int32_t **counts) {
    hipStream_t st = ctx->stream;
    const int64_t npids = (int64_t)s->parts.size();
    if (!f->counts_ev) QK_HIP(hipEventCreateWithFlags(&f->counts_ev, hipEventDisableTiming));
    if (npids > f->counts_cap || !f->counts) {
        // (a trim in flight on some context may still read the old array: hipFree waits for the device)
        if (f->counts) QK_HIP(hipFree(f->counts));
        f->counts = nullptr;
        f->counts_cap = 0;
        f->counts_built = false;
        const int64_t cap = std::max<int64_t>(npids + npids / 4, 64);
        if (hipMalloc((void **)&f->counts, (size_t)cap * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            QK_FAIL(QK_ERR_OOM, "qk_filter: no memory for the candidate counts of %lld lists", (long long)cap);
        }
        f->counts_cap = cap;
    }
    if (!f->counts_built) {
        // behind the mask (built on this stream, or waited for by filter_current) and behind the last derivation on another
        // context.  counts_ev covers derivations only, not the trims that read the array: like the mask's built_ev it relies on
        // the rule of the header that nobody changes the store while searches are in flight
        if (f->counts_ctx && f->counts_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, f->counts_ev, 0));
        if (npids > 0) {
            hipLaunchKernelGGL(k_filter_list_counts, dim3((unsigned)((npids + 3) / 4)), dim3(256), 0, st, (const uint16_t *)f->mask,
                               f->mask_words, (const int64_t *)s->d_off, (const int32_t *)s->d_size, (int)npids, f->counts);
            QK_HIP(hipGetLastError());
        }
        QK_HIP(hipEventRecord(f->counts_ev, st));
        f->counts_built = true;
        f->counts_ctx = ctx;
    } else if (f->counts_ctx != ctx) {
        QK_HIP(hipStreamWaitEvent(st, f->counts_ev, 0));  // derived on another context's stream
    }
    *counts = f->counts;
    return QK_OK;
}

int qk_filter_batch_counts_ensure(qk_ctx *ctx, qk_store *s, qk_filter *const *filters, int F, const int32_t *const **ctable) {
    std::vector<const int32_t *> h((size_t)F);
    for (int i = 0; i < F; i++) QK_TRY(qk_filter_counts_ensure(ctx, s, filters[i], &h[i]));
    // the rule of the mask table: its key (the masks are current: qk_filter_batch_ensure ran), and every count pointer
    std::vector<uint64_t> key = ctx->fb_key;
    for (int i = 0; i < F; i++) key.push_back((uint64_t)(uintptr_t)h[i]);
    if (key != ctx->fb_ckey || !ctx->fb_ctable) {
        ctx->fb_ckey.clear();
        if (F > ctx->fb_ctable_cap || !ctx->fb_ctable) {
            if (ctx->fb_ctable) QK_HIP(hipFree((void *)ctx->fb_ctable));
            ctx->fb_ctable = nullptr;
            ctx->fb_ctable_cap = 0;
            const int64_t cap = std::max<int64_t>(F, 64);
            if (hipMalloc((void **)&ctx->fb_ctable, (size_t)cap * sizeof(int32_t *)) != hipSuccess) {
                (void)hipGetLastError();
                QK_FAIL(QK_ERR_OOM, "filtered search: no memory for a table of %lld count arrays", (long long)cap);
            }
            ctx->fb_ctable_cap = cap;
        }
        // (pageable source: copied out when the call returns)
        QK_HIP(hipMemcpyAsync((void *)ctx->fb_ctable, h.data(), (size_t)F * sizeof(int32_t *), hipMemcpyHostToDevice, ctx->stream));
        ctx->fb_ckey = std::move(key);
    }
    *ctable = (const int32_t *const *)ctx->fb_ctable;
    return QK_OK;
}

int qk_launch_probe_trim(qk_ctx *ctx, qk_store *s, int64_t *pids, int64_t Q, int M, int n0, int64_t min_candidates, const int32_t *counts,
                         const int32_t *const *ctable, const int32_t *qfilter, int F, int32_t *nprobed) {
    if (Q <= 0 || M <= 0) return QK_OK;
    hipLaunchKernelGGL(k_probe_trim, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, ctx->stream, pids, Q, M, n0, (long long)min_candidates,
                       counts, ctable, qfilter, F, (int)s->parts.size(), nprobed);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

int qk_filter_ensure(qk_ctx *ctx, qk_store *s, qk_filter *f, const uint16_t **mask) {
    QK_TRY(filter_belongs(ctx, s, f));
    QK_TRY(qk_store_sync_table(s));
    QK_TRY(filter_current(ctx, s, f));
    *mask = f->mask;
    return QK_OK;
}

int qk_filter_batch_ensure(qk_ctx *ctx, qk_store *s, qk_filter *const *filters, int F, const uint16_t *const **table, const uint16_t **uni) {
    for (int i = 0; i < F; i++) QK_TRY(filter_belongs(ctx, s, filters[i]));
    QK_TRY(qk_store_sync_table(s));  // once: every filter is compared with the same version
    for (int i = 0; i < F; i++) QK_TRY(filter_current(ctx, s, filters[i]));
    // what the table and the union were derived from; a mask that was re-derived has another version (or capacity) or -- a
    // predicate whose column changed under an unchanged store -- another build count, a handle that was freed and allocated again
    // another serial
    std::vector<uint64_t> key;
    key.reserve((size_t)F * 5);
    for (int i = 0; i < F; i++) {
        const qk_filter *f = filters[i];
        key.push_back(f->serial);
        key.push_back(f->version);
        key.push_back((uint64_t)f->cap_rows);
        key.push_back((uint64_t)(uintptr_t)f->mask);
        key.push_back((uint64_t)f->rebuilds);
    }
    const int64_t words = s->cap_rows / 16;
    if (key != ctx->fb_key || !ctx->fb_table || !ctx->fb_union) {
        hipStream_t st = ctx->stream;
        ctx->fb_key.clear();
        if (F > ctx->fb_table_cap || !ctx->fb_table) {
            // (scans in flight may still read the old table: hipFree waits for the device)
            if (ctx->fb_table) QK_HIP(hipFree((void *)ctx->fb_table));
            ctx->fb_table = nullptr;
            ctx->fb_table_cap = 0;
            const int64_t cap = std::max<int64_t>(F, 64);
            if (hipMalloc((void **)&ctx->fb_table, (size_t)cap * sizeof(uint16_t *)) != hipSuccess) {
                (void)hipGetLastError();
                QK_FAIL(QK_ERR_OOM, "filtered search: no memory for a table of %lld masks", (long long)cap);
            }
            ctx->fb_table_cap = cap;
        }
        if (words > ctx->fb_union_words || !ctx->fb_union) {
            if (ctx->fb_union) QK_HIP(hipFree(ctx->fb_union));
            ctx->fb_union = nullptr;
            ctx->fb_union_words = 0;
            const int64_t cap = std::max<int64_t>(words + words / 4, 64);
            if (hipMalloc((void **)&ctx->fb_union, (size_t)cap * sizeof(uint16_t)) != hipSuccess) {
                (void)hipGetLastError();
                QK_FAIL(QK_ERR_OOM, "filtered search: no memory for the union of the masks (%lld tiles)", (long long)cap);
            }
            ctx->fb_union_words = cap;
        }
        // stream-ordered, no synchronisation: the source is pageable, so it has been copied out when the call returns
        std::vector<const uint16_t *> h((size_t)F);
        for (int i = 0; i < F; i++) h[i] = filters[i]->mask;
        QK_HIP(hipMemcpyAsync((void *)ctx->fb_table, h.data(), (size_t)F * sizeof(uint16_t *), hipMemcpyHostToDevice, st));
        if (words > 0) {
            hipLaunchKernelGGL(k_filter_union, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st,
                               (const uint16_t *const *)ctx->fb_table, F, words, ctx->fb_union);
            QK_HIP(hipGetLastError());
        }
        ctx->fb_key = std::move(key);
    }
    *table = (const uint16_t *const *)ctx->fb_table;
    *uni = ctx->fb_union;
    return QK_OK;
}

uint64_t qk_filter_next_serial() {
    static std::atomic<uint64_t> next_serial{1};
    return next_serial.fetch_add(1);
}

int qk_filter_first_build(qk_store *s, qk_filter *f) {
    QK_TRY(qk_store_sync_table(s));
    return filter_build(s->ctx, s, f);
}

extern "C" {

int qk_filter_create(qk_store *s, const int64_t *ids, int64_t n, int mode, int mem, qk_filter **out) {
    if (!s || !out || n < 0 || (n > 0 && !ids)) QK_FAIL(QK_ERR_INVALID, "qk_filter_create: bad argument");
    if (mode != QK_FILTER_ALLOW && mode != QK_FILTER_DENY) QK_FAIL(QK_ERR_INVALID, "qk_filter_create: mode must be QK_FILTER_ALLOW or QK_FILTER_DENY");
    qk_ctx *c = s->ctx;
    QK_HIP(hipSetDevice(c->device));
    // the request sorted and de-duplicated on the host (the product path has no device library)
    std::vector<int64_t> h((size_t)n);
    if (n > 0) {
        if (mem == QK_MEM_DEVICE) {
            QK_HIP(hipStreamSynchronize(c->stream));
            QK_HIP(hipMemcpy(h.data(), ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        } else {
            std::copy(ids, ids + n, h.begin());
        }
        std::sort(h.begin(), h.end());
        h.erase(std::unique(h.begin(), h.end()), h.end());
    }
    qk_filter *f = new qk_filter();
    f->serial = qk_filter_next_serial();
    f->store_uid = s->uid;
    f->device = c->device;
    f->mode = mode;
    f->n_ids = (int64_t)h.size();
    bool ok = hipMalloc((void **)&f->d_ids, std::max<size_t>(h.size(), 1) * sizeof(int64_t)) == hipSuccess &&
              hipMalloc((void **)&f->d_allowed, sizeof(unsigned long long)) == hipSuccess &&
              hipEventCreateWithFlags(&f->built_ev, hipEventDisableTiming) == hipSuccess;
    if (ok && !h.empty()) ok = hipMemcpy(f->d_ids, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        qk_filter_destroy(f);
        QK_FAIL(QK_ERR_OOM, "qk_filter_create: no device memory for %lld ids", (long long)n);
    }
    // the first mask now, on the store's context: the first filtered search does not pay for it
    const int rc = qk_filter_first_build(s, f);
    if (rc != QK_OK) {
        qk_filter_destroy(f);
        return rc;
    }
    *out = f;
    return QK_OK;
}

int qk_filter_destroy(qk_filter *f) {
    if (!f) return QK_OK;
    hipSetDevice(f->device);
    if (f->built_ev) {
        hipEventSynchronize(f->built_ev);
        hipEventDestroy(f->built_ev);
    }
    if (f->counts_ev) hipEventDestroy(f->counts_ev);
    if (f->mask) hipFree(f->mask);  // (hipFree waits for the device: no scan still reads the mask)
    if (f->counts) hipFree(f->counts);
    if (f->d_ids) hipFree(f->d_ids);
    if (f->d_allowed) hipFree(f->d_allowed);
    (void)hipGetLastError();
    delete f;
    return QK_OK;
}

int qk_filter_info(qk_filter *f, int64_t *n_ids, int64_t *rows_allowed, uint64_t *store_version, int64_t *rebuilds, int64_t *device_bytes) {
    if (!f) QK_FAIL(QK_ERR_INVALID, "qk_filter_info: null filter");
    QK_HIP(hipSetDevice(f->device));
    if (n_ids) *n_ids = f->kind == QK_FILTER_KIND_WHERE ? -1 : f->n_ids;
    if (rows_allowed) {
        unsigned long long v = 0;
        QK_HIP(hipEventSynchronize(f->built_ev));
        QK_HIP(hipMemcpy(&v, f->d_allowed, sizeof(v), hipMemcpyDeviceToHost));
        *rows_allowed = (int64_t)v;
    }
    if (store_version) *store_version = f->version;
    if (rebuilds) *rebuilds = f->rebuilds;
    if (device_bytes) {
        if (f->kind == QK_FILTER_KIND_WHERE) *device_bytes = (int64_t)(f->mask_words * sizeof(uint16_t));  // (no ids: the mask only)
        else *device_bytes = (int64_t)(f->mask_words * sizeof(uint16_t) + std::max<int64_t>(f->n_ids, 1) * sizeof(int64_t) + 8);
        *device_bytes += (int64_t)(f->counts_cap * sizeof(int32_t));  // (adaptive probing: once a call has derived them)
    }
    return QK_OK;
}

int qk_search_filtered(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                       qk_filter *f, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s || !f || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered: null argument");
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered: k must be positive");
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_search_filtered: k=%d exceeds QK_MAX_K=%d (filtered search has no wide-k path)", k, QK_MAX_K);
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered: nprobe must be positive");
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, nullptr, f);
}

int qk_search_filtered_tracked(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                               qk_filter *f, int64_t *out_ids, float *out_dist, int64_t *out_probed, int mem, qk_timing *timing) {
    if (!ctx || !s || !f || !parent || (Q > 0 && (!x || !out_ids || !out_probed))) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_tracked: null argument");
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_tracked: k must be positive");
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_search_filtered_tracked: k=%d exceeds QK_MAX_K=%d (filtered search has no wide-k path)", k, QK_MAX_K);
    if (nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_tracked: nprobe must be positive");
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, out_probed, f);
}

int qk_scan_filtered(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric, qk_filter *f,
                     int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s || !f || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "qk_scan_filtered: null argument");
    if (P <= 0 || !pids) QK_FAIL(QK_ERR_INVALID, "qk_scan_filtered: bad partition id list");
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "qk_scan_filtered: k must be positive");
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_scan_filtered: k=%d exceeds QK_MAX_K=%d (filtered search has no wide-k path)", k, QK_MAX_K);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (mem == QK_MEM_HOST) {
        for (int64_t i = 0; i < Q * (int64_t)P; i++) {
            const int64_t p = pids[i];
            if (p < 0) continue;
            if (p >= (int64_t)s->parts.size() || !s->parts[p].present)
                QK_FAIL(QK_ERR_NOT_FOUND, "List does not exist in get_codes (list %lld)", (long long)p);
        }
    }
    return qk_run_search(ctx, nullptr, s, x, Q, pids, P, 0, k, metric, out_ids, out_dist, mem, timing, false, false, nullptr, f);
}

// ---- one filter per query ------------------------------------------------------------------------------------------------------
static int check_filter_batch(const char *who, qk_filter *const *filters, int F, const int32_t *qfilter, int64_t Q, int k, int mem) {
    if (!filters || F < 1) QK_FAIL(QK_ERR_INVALID, "%s: at least one filter is required (F=%d)", who, F);
    if (F > QK_MAX_BATCH_FILTERS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: F=%d exceeds QK_MAX_BATCH_FILTERS=%d", who, F, QK_MAX_BATCH_FILTERS);
    for (int i = 0; i < F; i++)
        if (!filters[i]) QK_FAIL(QK_ERR_INVALID, "%s: filter %d of %d is null", who, i, F);
    if (Q > 0 && !qfilter) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "%s: k must be positive", who);
    if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d (filtered search has no wide-k path)", who, k, QK_MAX_K);
    if (mem == QK_MEM_HOST)
        for (int64_t i = 0; i < Q; i++)
            if (qfilter[i] < 0 || qfilter[i] >= F)
                QK_FAIL(QK_ERR_INVALID, "%s: qfilter[%lld]=%d is outside [0, F=%d)", who, (long long)i, (int)qfilter[i], F);
    return QK_OK;
}

int qk_search_filtered_batch(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                             qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids, float *out_dist, int mem,
                             qk_timing *timing) {
    if (!ctx || !s || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_batch: null argument");
    QK_TRY(check_filter_batch("qk_search_filtered_batch", filters, F, qfilter, Q, k, mem));
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_batch: nprobe must be positive");
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    const qk_filter_batch fb{filters, F, qfilter};
    return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, nullptr, nullptr, &fb);
}

int qk_search_filtered_batch_tracked(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                                     qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids, float *out_dist,
                                     int64_t *out_probed, int mem, qk_timing *timing) {
    if (!ctx || !s || !parent || (Q > 0 && (!x || !out_ids || !out_probed))) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_batch_tracked: null argument");
    QK_TRY(check_filter_batch("qk_search_filtered_batch_tracked", filters, F, qfilter, Q, k, mem));
    if (nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_batch_tracked: nprobe must be positive");
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    const qk_filter_batch fb{filters, F, qfilter};
    return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, out_probed, nullptr, &fb);
}

int qk_scan_filtered_batch(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                           qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids, float *out_dist, int mem,
                           qk_timing *timing) {
    if (!ctx || !s || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "qk_scan_filtered_batch: null argument");
    if (P <= 0 || !pids) QK_FAIL(QK_ERR_INVALID, "qk_scan_filtered_batch: bad partition id list");
    QK_TRY(check_filter_batch("qk_scan_filtered_batch", filters, F, qfilter, Q, k, mem));
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (mem == QK_MEM_HOST) {
        for (int64_t i = 0; i < Q * (int64_t)P; i++) {
            const int64_t p = pids[i];
            if (p < 0) continue;
            if (p >= (int64_t)s->parts.size() || !s->parts[p].present)
                QK_FAIL(QK_ERR_NOT_FOUND, "List does not exist in get_codes (list %lld)", (long long)p);
        }
    }
    const qk_filter_batch fb{filters, F, qfilter};
    return qk_run_search(ctx, nullptr, s, x, Q, pids, P, 0, k, metric, out_ids, out_dist, mem, timing, false, false, nullptr, nullptr, &fb);
}

// ---- adaptive probing ----------------------------------------------------------------------------------------------------------
int qk_search_filtered_adaptive(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int max_nprobe,
                                int64_t min_candidates, int k, int metric, qk_filter *const *filters, int F, const int32_t *qfilter,
                                int64_t *out_ids, float *out_dist, int32_t *out_nprobed, int64_t *out_probed, int mem, qk_timing *timing) {
    const char *who = "qk_search_filtered_adaptive";
    if (!ctx || !s || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (!parent) QK_FAIL(QK_ERR_INVALID, "%s: parent is null (a flat index has nothing to adapt)", who);
    const bool one = F == 1 && !qfilter;  // one filter for every query
    if (one) {
        if (!filters || !filters[0]) QK_FAIL(QK_ERR_INVALID, "%s: null filter", who);
        if (k <= 0) QK_FAIL(QK_ERR_INVALID, "%s: k must be positive", who);
        if (k > QK_MAX_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds QK_MAX_K=%d (filtered search has no wide-k path)", who, k, QK_MAX_K);
    } else {
        QK_TRY(check_filter_batch(who, filters, F, qfilter, Q, k, mem));
    }
    if (nprobe < 1) QK_FAIL(QK_ERR_INVALID, "%s: nprobe must be positive", who);
    if (max_nprobe < nprobe) QK_FAIL(QK_ERR_INVALID, "%s: max_nprobe=%d < nprobe=%d", who, max_nprobe, nprobe);
    if (min_candidates < 1) QK_FAIL(QK_ERR_INVALID, "%s: min_candidates must be positive", who);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    qk_adaptive ad;
    ad.nprobe = nprobe;
    ad.min_candidates = min_candidates;
    ad.out_nprobed = out_nprobed;
    if (one)
        return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, max_nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, out_probed,
                             filters[0], nullptr, &ad);
    const qk_filter_batch fb{filters, F, qfilter};
    return qk_run_search(ctx, parent, s, x, Q, nullptr, 0, max_nprobe, k, metric, out_ids, out_dist, mem, timing, false, false, out_probed,
                         nullptr, &fb, &ad);
}

}  // extern "C"
