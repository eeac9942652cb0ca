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
// A filter is of one of three kinds (qk_attr.h): an id set, as above, or a PREDICATE over attribute columns (qk_attr.hip) -- a
// conjunction, whose mask k_filter_build_where derives, or an EXPRESSION (an OR of conjunctions with value sets,
// k_filter_build_expr) -- whose stamp also holds the version of every column it names.  Everything behind the mask -- the scans,
// the per-query table, the union -- is the same for all.
#include "qk_attr.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace {

void pool_release(qk_filter *f);  // (the candidate pool, below)

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
    else if (f->kind == QK_FILTER_KIND_EXPR) QK_TRY(qk_launch_filter_build_expr(ctx, s, f));
    else QK_TRY(filter_build_ids(ctx, s, f));
    hipStream_t st = ctx->stream;
    QK_HIP(hipEventRecord(f->built_ev, st));
    if (f->built) f->rebuilds++;
    f->built = true;
    f->counts_built = false;  // (adaptive probing: re-derived by the next call that needs them)
    f->cand_built = false;    // (exact search: the candidate store too, and the count is read again)
    f->cand_rows = -1;
    if (f->pool_slot >= 0) pool_release(f);  // (exact search per query: the slot in the store's candidate pool)
    f->built_ctx = ctx;
    f->version = s->version;
    f->cap_rows = s->cap_rows;
    return QK_OK;
}

// the mask of a filter of this store and device, current for the store's table (the caller has synced it)
int filter_current(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    if (!f->built || f->version != s->version || f->cap_rows != s->cap_rows ||
        (f->kind != QK_FILTER_KIND_IDS && !qk_filter_where_current(f))) {
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

// ---- exact search: the candidate rows of a filter, compacted into a one-list store ------------------------------------------------
// The mask is a bitmap of arena rows: bit r of word w is row 16 w + r, and four consecutive words read as one little-endian
// 64-bit CHUNK are rows 64 c .. 64 c + 63.  A scan BLOCK is QK_CAND_BLOCK = 64 words = 16 chunks = 1024 rows.  Three launches, no
// atomics, no device library, int64 offsets: the candidates of every block (k_filter_block_counts), their exclusive prefix sum
// (k_filter_block_scan, one workgroup), and the gather, which finds its source rows from the block offsets and the block's own
// 128 bytes of mask (k_filter_gather).
constexpr int QK_CAND_BLOCK = 64;

// chunk c of a mask of nwords words (8-byte aligned: the mask is a hipMalloc of its own); words behind the end read as 0
__device__ __forceinline__ uint64_t mask_chunk(const uint16_t *mask, int64_t c, int64_t nwords) {
    const int64_t w = c * 4;
    if (w + 4 <= nwords) return *(const uint64_t *)(mask + w);
    uint64_t v = 0;
    for (int i = 0; i < 4; i++)
        if (w + i < nwords) v |= (uint64_t)mask[w + i] << (16 * i);
    return v;
}

// one lane per chunk, 16 lanes per block: a wave reads 512 consecutive bytes; every cnt[b] has one writer
__global__ __launch_bounds__(256) void k_filter_block_counts(const uint16_t *mask, int64_t nwords, int64_t nb, int64_t *cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t c = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    int n = __popcll(mask_chunk(mask, c, nwords));
    for (int off = 1; off < 16; off <<= 1) n += __shfl_xor(n, off);
    const int64_t b = c >> 4;
    if ((lane & 15) == 0 && b < nb) cnt[b] = n;
}

// off[i] = cnt[0] + .. + cnt[i - 1] for i in [0, nb]; one workgroup: thread t owns a contiguous slice, the 1024 slice sums are
// scanned through LDS (nb is cap_rows / 1024: 9766 at 10M rows)
__global__ __launch_bounds__(1024) void k_filter_block_scan(const int64_t *__restrict__ cnt, int64_t *__restrict__ off, int64_t nb) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b = min(nb, (int64_t)t * per), e = min(nb, b + per);
    int64_t s = 0;
    for (int64_t i = b; i < e; i++) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t i = b; i < e; i++) {
        off[i] = run;
        run += cnt[i];
    }
    if (t == 1023) off[nb] = part[1023];
}

struct GatherParams {
    const uint16_t *mask;
    int64_t nwords;      // live words of the mask (the source arena's tiles)
    const int64_t *boff;  // [nb + 1]
    int64_t nb;
    int64_t n;           // candidates = boff[nb]
    int64_t ntiles;      // destination tiles: ceil(n / 16)
    int nblk;
    const float4 *sv;    // source arena
    const uint32_t *sn;
    const int64_t *si;
    int64_t src_rows;    // its capacity
    float4 *dv;          // destination arena (>= ntiles tiles)
    uint32_t *dn;
    int64_t *di;
};

// The stable compaction, destination-driven: destination row j is the j-th candidate in ascending arena-row order.  One wave per
// destination tile, lane g * 16 + dr: the lane finds the source of row dr -- a binary search of the block offsets, a walk over
// the block's 16 chunks, the (j - offset)-th set bit of the chunk it lands in -- and then copies, per 16-column block, the float4
// of (row, g): 16-byte gathers, one coalesced 1 KiB store per wave.  The rows behind the last candidate in the last tile get
// what a fresh arena holds (zeros, norm 0, id -1) on every build.  The four lanes of a row do the search redundantly.
__global__ __launch_bounds__(256) void k_filter_gather(GatherParams G) {
    const int lane = threadIdx.x & 63, dr = lane & 15, g = lane >> 4;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= G.ntiles) return;  // (the whole wave)
    const int64_t j = tile * 16 + dr;
    int64_t src = -1;
    if (j < G.n) {
        int64_t lo = 0, hi = G.nb;  // boff[lo] <= j < boff[hi]: the last block that starts at or below j holds row j
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (G.boff[mid] <= j) lo = mid;
            else hi = mid;
        }
        int64_t rem = j - G.boff[lo];
        const int64_t c0 = lo * (QK_CAND_BLOCK / 4);
        for (int c = 0; c < QK_CAND_BLOCK / 4; c++) {
            uint64_t v = mask_chunk(G.mask, c0 + c, G.nwords);
            const int pc = __popcll(v);
            if (rem < pc) {
                for (int i = 0; i < (int)rem; i++) v &= v - 1;  // drop the `rem` lowest set bits
                src = (c0 + c) * 64 + (__ffsll((unsigned long long)v) - 1);
                break;
            }
            rem -= pc;
        }
        if (src >= G.src_rows) src = -1;  // (cannot happen with offsets derived from this mask: never read outside the arena)
    }
    const bool live = src >= 0;
    const float4 *sp = G.sv + ((live ? src >> 4 : 0) * G.nblk) * 64 + g * 16 + (live ? (int)(src & 15) : 0);
    float4 *dp = G.dv + (tile * G.nblk) * 64 + lane;
#pragma unroll 4
    for (int c = 0; c < G.nblk; c++) dp[(int64_t)c * 64] = live ? sp[(int64_t)c * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (g == 0) {
        G.dn[j] = live ? G.sn[src] : 0u;  // (the norm's bits, not a recomputation)
        G.di[j] = live ? G.si[src] : -1;
    }
}

void cand_free_arena(qk_store *c) {
    if (c->vecs) hipFree(c->vecs);  // (hipFree waits for the device: no scan still reads the rows)
    if (c->norms) hipFree(c->norms);
    if (c->ids) hipFree(c->ids);
    c->vecs = nullptr;
    c->norms = nullptr;
    c->ids = nullptr;
    c->cap_rows = 0;
    (void)hipGetLastError();
}

int64_t cand_device_bytes(const qk_filter *f) {
    const qk_store *c = f->cand;
    if (!c) return 0;
    return c->cap_rows * ((int64_t)c->dpad * 4 + 12) + c->table_cap * 12 + c->rowmajor_cap * 4;
}

// the candidates of a filter whose mask is current on ctx's stream (filter_current ran): 8 bytes of d_allowed, once per mask build
int cand_count(qk_filter *f, int64_t *rows) {
    if (f->cand_rows < 0) {
        unsigned long long v = 0;
        QK_HIP(hipEventSynchronize(f->built_ev));
        QK_HIP(hipMemcpy(&v, f->d_allowed, sizeof(v), hipMemcpyDeviceToHost));
        f->cand_rows = (int64_t)v;
    }
    *rows = f->cand_rows;
    return QK_OK;
}

// the candidate store of a filter whose mask the caller has just brought up to date on ctx's stream and whose n candidates it has
// counted: derived behind the mask if the mask is newer than it is.  max_rows > 0 bounds the capacity a growth may ask for
int cand_ensure(qk_ctx *ctx, qk_store *s, qk_filter *f, int64_t n, int64_t max_rows) {
    hipStream_t st = ctx->stream;
    if (f->cand_built) {
        f->cand->ctx = ctx;  // (a row-major copy the dense forms may ask for is made on the calling context, complete on return)
        if (f->cand_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, f->cand_ev, 0));  // derived on another context's stream
        return QK_OK;
    }
    if (n > (int64_t)INT32_MAX - 16) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_search_filtered_exact: %lld candidates exceed a list's 2^31 rows", (long long)n);
    if (!f->cand_ev) QK_HIP(hipEventCreateWithFlags(&f->cand_ev, hipEventDisableTiming));
    if (!f->cand) {
        QK_TRY(qk_store_create(ctx, s->d, &f->cand));
        QK_TRY(qk_store_add_list(f->cand, 0));
    }
    qk_store *c = f->cand;
    // behind the last derivation on another context (its gather wrote the arena this one rewrites).  cand_ev covers derivations
    // only, not the searches that read the rows: like the mask's built_ev it relies on the rule of the header that nobody changes
    // the store while searches are in flight
    if (f->cand_ctx && f->cand_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, f->cand_ev, 0));
    const int64_t need = std::max<int64_t>(qk_round_up64(n, 16), 1024);  // (at least 1024 rows, like every arena)
    if (need > c->cap_rows || !c->vecs) {
        cand_free_arena(c);
        int64_t cap = need + need / 4;
        if (max_rows > 0) cap = std::min(cap, max_rows);
        cap = qk_round_up64(std::max(cap, need), 16);
        if (hipMalloc((void **)&c->vecs, (size_t)cap * c->dpad * sizeof(float)) != hipSuccess ||
            hipMalloc((void **)&c->norms, (size_t)cap * sizeof(float)) != hipSuccess ||
            hipMalloc((void **)&c->ids, (size_t)cap * sizeof(int64_t)) != hipSuccess) {
            (void)hipGetLastError();
            cand_free_arena(c);
            QK_FAIL(QK_ERR_OOM, "qk_search_filtered_exact: no memory for %lld candidate rows x %d dims", (long long)cap, c->dpad);
        }
        c->cap_rows = cap;
        // what a fresh arena holds: rows behind the data are only ever read masked, but finite and deterministic
        QK_HIP(hipMemsetAsync(c->vecs, 0, (size_t)cap * c->dpad * sizeof(float), st));
        QK_HIP(hipMemsetAsync(c->norms, 0, (size_t)cap * sizeof(float), st));
        QK_HIP(hipMemsetAsync(c->ids, 0xFF, (size_t)cap * sizeof(int64_t), st));
    }
    if (n > 0) {
        const int64_t nwords = f->cap_rows / 16;  // (the mask was built for this capacity: filter_current)
        const int64_t nb = (nwords + QK_CAND_BLOCK - 1) / QK_CAND_BLOCK;
        QK_TRY(qk_ws_reserve(ctx, (size_t)(2 * nb + 1) * sizeof(int64_t) + 1024));
        int64_t *cnt = (int64_t *)qk_ws_alloc(ctx, (size_t)nb * sizeof(int64_t));
        int64_t *boff = (int64_t *)qk_ws_alloc(ctx, (size_t)(nb + 1) * sizeof(int64_t));
        if (!cnt || !boff) QK_FAIL(QK_ERR_OOM, "qk_search_filtered_exact: workspace exhausted");
        hipLaunchKernelGGL(k_filter_block_counts, dim3((unsigned)((nb + 15) / 16)), dim3(256), 0, st, (const uint16_t *)f->mask, nwords, nb, cnt);
        hipLaunchKernelGGL(k_filter_block_scan, dim3(1), dim3(1024), 0, st, (const int64_t *)cnt, boff, nb);
        GatherParams G;
        G.mask = f->mask;
        G.nwords = nwords;
        G.boff = boff;
        G.nb = nb;
        G.n = n;
        G.ntiles = (n + 15) / 16;
        G.nblk = s->nblk;
        G.sv = (const float4 *)s->vecs;
        G.sn = (const uint32_t *)s->norms;
        G.si = s->ids;
        G.src_rows = s->cap_rows;
        G.dv = (float4 *)c->vecs;
        G.dn = (uint32_t *)c->norms;
        G.di = c->ids;
        hipLaunchKernelGGL(k_filter_gather, dim3((unsigned)((G.ntiles + 3) / 4)), dim3(256), 0, st, G);
        QK_HIP(hipGetLastError());
    }
    QK_HIP(hipEventRecord(f->cand_ev, st));
    // the one list: rows 0 .. n - 1.  The id bounds are the source's (bounds of a subset); the host id mirror stays empty
    c->ctx = ctx;  // (its table upload and row-major copy run on the stream that ran the gather)
    qk_part &pt = c->parts[0];
    pt.row_off = 0;
    pt.size = n;
    pt.cap = c->cap_rows;
    c->ntotal = n;
    c->used_rows = qk_round_up64(n, 16);
    c->min_id_seen = s->min_id_seen;
    c->max_id_seen = s->max_id_seen;
    c->table_dirty = true;
    QK_TRY(qk_store_sync_table(c));
    f->cand_built = true;
    f->cand_builds++;
    f->cand_ctx = ctx;
    return QK_OK;
}

// ---- exact search per query: the candidate pool -----------------------------------------------------------------------------------
// A batch that mixes filters needs the candidates of all of them as lists of ONE store: the partition scan addresses one arena.
// The pool is that store, private to the searched store.  A filter that was admitted holds a SLOT = a list number of the pool,
// whose extent holds what the filter's private candidate store holds (the same rows in the same order, copied by the same
// construction), and keeps it from call to call: a call gathers only the filters that have no valid slot.  Query i of
// qk_search_filtered_exact_batch then scans list slot(filters[qfilter[i]]) -- the ordinary partition scan with one list per query.
//
// Extents are tile-aligned pieces of the pool arena handed out first-fit from the extents given back (mask builds, evictions,
// qk_filter_destroy), then from the bump pointer; when neither fits, the live extents are copied, packed, into a fresh arena
// (`repack`: the only place capacity changes).  The pool's device table is written by admit itself, from pageable memory in
// stream order: qk_store_sync_table and its two synchronisations never run for the pool.
struct PoolAdmit {      // one filter of an admission that has candidates
    const uint16_t *mask;
    int64_t n;          // candidates
    int64_t dst_row;    // first row of its extent in the pool arena (a multiple of 16)
    int64_t tile0;      // destination tiles of the entries in front of it; entry M (the sentinel): all of them
};

// out[i] = *allowed[i]: the candidate counts of the filters of a call whose count has not been read since their mask build
__global__ __launch_bounds__(256) void k_pool_counts(const unsigned long long *const *allowed, int M, int64_t *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) out[i] = (int64_t)*allowed[i];
}

// k_filter_block_counts for entry blockIdx.y: cnt[m * nb + b]
__global__ __launch_bounds__(256) void k_pool_block_counts(const PoolAdmit *tab, int64_t nwords, int64_t nb, int64_t *cnt) {
    const int m = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t c = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    int n = __popcll(mask_chunk(tab[m].mask, c, nwords));
    for (int off = 1; off < 16; off <<= 1) n += __shfl_xor(n, off);
    const int64_t b = c >> 4;
    if ((lane & 15) == 0 && b < nb) cnt[(int64_t)m * nb + b] = n;
}

// k_filter_block_scan, one workgroup per entry: off[m * (nb + 1) + i]
__global__ __launch_bounds__(1024) void k_pool_block_scan(const int64_t *__restrict__ cnt_all, int64_t *__restrict__ off_all, int64_t nb) {
    __shared__ int64_t part[1024];
    const int64_t *cnt = cnt_all + (int64_t)blockIdx.x * nb;
    int64_t *off = off_all + (int64_t)blockIdx.x * (nb + 1);
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b = min(nb, (int64_t)t * per), e = min(nb, b + per);
    int64_t s = 0;
    for (int64_t i = b; i < e; i++) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t i = b; i < e; i++) {
        off[i] = run;
        run += cnt[i];
    }
    if (t == 1023) off[nb] = part[1023];
}

struct PoolGatherParams {
    const PoolAdmit *tab;  // [M + 1]
    int M;
    int64_t ntiles;        // destination tiles of all entries = tab[M].tile0
    int64_t nwords;        // live words of every mask (the source arena's tiles)
    const int64_t *boff;   // [M][nb + 1]
    int64_t nb;
    int nblk;
    const float4 *sv;      // source arena
    const uint32_t *sn;
    const int64_t *si;
    int64_t src_rows;      // its capacity
    float4 *dv;            // pool arena
    uint32_t *dn;
    int64_t *di;
    int64_t dst_rows;      // its capacity
};

// k_filter_gather over the destination tiles of all entries: a wave finds the entry of its tile (the last one whose tile0 is not
// behind it: a binary search of M + 1 words), then does what k_filter_gather does with that entry's mask, offsets and extent --
// the rows behind the entry's last candidate in its last tile get what a fresh arena holds.
__global__ __launch_bounds__(256) void k_pool_gather(PoolGatherParams G) {
    const int lane = threadIdx.x & 63, dr = lane & 15, g = lane >> 4;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= G.ntiles) return;  // (the whole wave)
    int m = 0, mh = G.M;
    while (mh - m > 1) {
        const int mid = (m + mh) >> 1;
        if (G.tab[mid].tile0 <= tile) m = mid;
        else mh = mid;
    }
    const PoolAdmit e = G.tab[m];
    const int64_t j = (tile - e.tile0) * 16 + dr;  // row of the slot
    const int64_t drow = e.dst_row + j;            // row of the pool arena
    if (drow - dr + 16 > G.dst_rows) return;       // (cannot happen with extents the host laid out: never write outside the arena)
    const int64_t *boff = G.boff + (int64_t)m * (G.nb + 1);
    int64_t src = -1;
    if (j < e.n) {
        int64_t lo = 0, hi = G.nb;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (boff[mid] <= j) lo = mid;
            else hi = mid;
        }
        int64_t rem = j - boff[lo];
        const int64_t c0 = lo * (QK_CAND_BLOCK / 4);
        for (int c = 0; c < QK_CAND_BLOCK / 4; c++) {
            uint64_t v = mask_chunk(e.mask, c0 + c, G.nwords);
            const int pc = __popcll(v);
            if (rem < pc) {
                for (int i = 0; i < (int)rem; i++) v &= v - 1;
                src = (c0 + c) * 64 + (__ffsll((unsigned long long)v) - 1);
                break;
            }
            rem -= pc;
        }
        if (src >= G.src_rows) src = -1;
    }
    const bool live = src >= 0;
    const float4 *sp = G.sv + ((live ? src >> 4 : 0) * G.nblk) * 64 + g * 16 + (live ? (int)(src & 15) : 0);
    float4 *dp = G.dv + ((drow >> 4) * G.nblk) * 64 + lane;
#pragma unroll 4
    for (int c = 0; c < G.nblk; c++) dp[(int64_t)c * 64] = live ? sp[(int64_t)c * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (g == 0) {
        G.dn[drow] = live ? G.sn[src] : 0u;
        G.di[drow] = live ? G.si[src] : -1;
    }
}

// pids[q] = the pool list of query q's filter, -1 for a qfilter value outside [0, F) (checked before the table is indexed)
__global__ __launch_bounds__(256) void k_pool_pids(const int32_t *qfilter, int64_t Q, int F, const int64_t *slot_of, int64_t *pids) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int f = qfilter[q];
    pids[q] = (unsigned)f < (unsigned)F ? slot_of[f] : -1;
}

struct PoolSlot {
    bool used = false;
    uint64_t serial = 0;  // the filter that owns it
    int64_t n = 0;        // candidates; the extent is parts[slot] of the pool store: rows [row_off, row_off + round_up(n, 16))
    int64_t stamp = 0;    // the last call that named it (qk_pool::clock)
};

}  // namespace

struct qk_pool {
    qk_store *st = nullptr;  // parts[slot]
    std::vector<PoolSlot> slots;
    std::vector<std::pair<int64_t, int64_t>> free_ext;  // (first row, rows) given back, ascending, merged, none at the bump pointer
    int64_t rows = 0;        // sum of round_up(n, 16) over the used slots: what pool_rows bounds
    int64_t nused = 0;
    int64_t clock = 0, builds = 0, evictions = 0;
    hipEvent_t ev = nullptr;  // behind the last admission, on the stream of ev_ctx
    qk_ctx *ev_ctx = nullptr;
};

namespace {

// filters outlive stores and the other way round: a filter finds the pool of its store by uid, under this lock
std::mutex g_pool_mu;
std::unordered_map<uint64_t, qk_pool *> g_pools;

void pool_free_extent(qk_pool *p, int64_t off, int64_t len) {
    if (len <= 0) return;
    auto &fe = p->free_ext;
    auto it = std::lower_bound(fe.begin(), fe.end(), std::make_pair(off, (int64_t)0));
    it = fe.insert(it, {off, len});
    if (it + 1 != fe.end() && it->first + it->second == (it + 1)->first) {
        it->second += (it + 1)->second;
        it = fe.erase(it + 1) - 1;
    }
    if (it != fe.begin() && (it - 1)->first + (it - 1)->second == it->first) {
        (it - 1)->second += it->second;
        it = fe.erase(it) - 1;
    }
    if (it->first + it->second == p->st->used_rows) {  // the last extent: the bump pointer falls back
        p->st->used_rows = it->first;
        fe.erase(it);
    }
}

// first fit among the extents given back, then the bump pointer; -1: neither has room
int64_t pool_take_extent(qk_pool *p, int64_t len) {
    if (len <= 0) return 0;
    for (auto it = p->free_ext.begin(); it != p->free_ext.end(); ++it)
        if (it->second >= len) {
            const int64_t off = it->first;
            it->first += len;
            it->second -= len;
            if (it->second == 0) p->free_ext.erase(it);
            return off;
        }
    if (p->st->used_rows + len > p->st->cap_rows) return -1;
    const int64_t off = p->st->used_rows;
    p->st->used_rows += len;
    return off;
}

// host bookkeeping only: the rows stay where they are until the extent is handed out again
void pool_free_slot(qk_pool *p, int64_t slot) {
    PoolSlot &sl = p->slots[slot];
    qk_part &pt = p->st->parts[slot];
    pool_free_extent(p, pt.row_off, pt.cap);
    p->rows -= pt.cap;
    p->nused--;
    pt = qk_part();
    sl = PoolSlot();
    p->st->table_dirty = true;  // (written by the next admission or, if none follows, by the next call's pool_publish)
}

void pool_release(qk_filter *f) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pools.find(f->store_uid);
    if (it != g_pools.end()) {
        qk_pool *p = it->second;
        if (f->pool_slot < (int64_t)p->slots.size() && p->slots[f->pool_slot].used && p->slots[f->pool_slot].serial == f->serial)
            pool_free_slot(p, f->pool_slot);
    }
    f->pool_slot = -1;
}

bool pool_slot_valid(const qk_pool *p, const qk_filter *f) {
    return p && f->pool_slot >= 0 && f->pool_slot < (int64_t)p->slots.size() && p->slots[f->pool_slot].used &&
           p->slots[f->pool_slot].serial == f->serial;
}

int64_t pool_device_bytes(const qk_pool *p) {
    const qk_store *c = p->st;
    return c->cap_rows * ((int64_t)c->dpad * 4 + 12) + c->table_cap * 12;
}

// what qk_store_sync_table does for the pool store, without waiting: the whole table from pageable memory (copied out when the
// call returns), in stream order behind the scans that read the old one
int pool_publish(qk_ctx *ctx, qk_pool *p, const qk_store *s) {
    qk_store *c = p->st;
    if (!c->table_dirty) return QK_OK;
    const int64_t n = (int64_t)c->parts.size();
    if (n > c->table_cap) {
        // (scans in flight may still read the old table: hipFree waits for the device.  4096 entries at first, then doubling)
        if (c->d_off) QK_HIP(hipFree(c->d_off));
        if (c->d_size) QK_HIP(hipFree(c->d_size));
        c->d_off = nullptr;
        c->d_size = nullptr;
        c->table_cap = 0;
        const int64_t cap = std::max<int64_t>(2 * n, 4096);
        if (hipMalloc((void **)&c->d_off, (size_t)cap * sizeof(int64_t)) != hipSuccess ||
            hipMalloc((void **)&c->d_size, (size_t)cap * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            QK_FAIL(QK_ERR_OOM, "qk_search_filtered_exact_batch: no memory for a table of %lld lists", (long long)cap);
        }
        c->table_cap = cap;
    }
    std::vector<int64_t> ho((size_t)n);
    std::vector<int32_t> hs((size_t)n);
    int64_t mx = 0, nonempty = 0, total = 0;
    for (int64_t i = 0; i < n; i++) {
        const qk_part &pt = c->parts[i];
        ho[i] = pt.row_off;
        hs[i] = pt.present ? (int32_t)pt.size : -1;
        if (pt.present) {
            mx = std::max(mx, pt.size);
            total += pt.size;
            if (pt.size > 0) nonempty++;
        }
    }
    if (n > 0) {
        QK_HIP(hipMemcpyAsync(c->d_off, ho.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        QK_HIP(hipMemcpyAsync(c->d_size, hs.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    c->max_size = mx;
    c->n_nonempty = nonempty;
    c->ntotal = total;
    c->nlist = p->nused;
    c->min_id_seen = s->min_id_seen;  // (bounds of a subset; the host id mirrors stay empty: no id travels to the host)
    c->max_id_seen = s->max_id_seen;
    c->version++;
    c->counters[5]++;
    c->rowmajor_valid = false;
    c->table_dirty = false;
    return QK_OK;
}

// the live extents packed into a fresh arena of `cap` rows, on ctx's stream; the old arena is freed behind the copies
int pool_repack(qk_ctx *ctx, qk_pool *p, int64_t cap) {
    qk_store *c = p->st;
    hipStream_t st = ctx->stream;
    float *nv = nullptr, *nn = nullptr;
    int64_t *ni = nullptr;
    if (hipMalloc((void **)&nv, (size_t)cap * c->dpad * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&nn, (size_t)cap * sizeof(float)) != hipSuccess || hipMalloc((void **)&ni, (size_t)cap * sizeof(int64_t)) != hipSuccess) {
        (void)hipGetLastError();
        if (nv) hipFree(nv);
        if (nn) hipFree(nn);
        if (ni) hipFree(ni);
        QK_FAIL(QK_ERR_OOM, "qk_search_filtered_exact_batch: no memory for a pool of %lld rows x %d dims", (long long)cap, c->dpad);
    }
    // what a fresh arena holds: rows outside the extents are only ever read masked, but finite and deterministic
    QK_HIP(hipMemsetAsync(nv, 0, (size_t)cap * c->dpad * sizeof(float), st));
    QK_HIP(hipMemsetAsync(nn, 0, (size_t)cap * sizeof(float), st));
    QK_HIP(hipMemsetAsync(ni, 0xFF, (size_t)cap * sizeof(int64_t), st));
    std::vector<int64_t> order;
    for (int64_t i = 0; i < (int64_t)p->slots.size(); i++)
        if (p->slots[i].used && c->parts[i].cap > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return c->parts[a].row_off < c->parts[b].row_off; });
    int64_t cur = 0;
    for (int64_t i : order) {  // (a tile-aligned extent is one contiguous piece of each of the three arrays)
        qk_part &pt = c->parts[i];
        QK_HIP(hipMemcpyAsync(nv + cur * c->dpad, c->vecs + pt.row_off * c->dpad, (size_t)pt.cap * c->dpad * sizeof(float), hipMemcpyDeviceToDevice, st));
        QK_HIP(hipMemcpyAsync(nn + cur, c->norms + pt.row_off, (size_t)pt.cap * sizeof(float), hipMemcpyDeviceToDevice, st));
        QK_HIP(hipMemcpyAsync(ni + cur, c->ids + pt.row_off, (size_t)pt.cap * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        pt.row_off = cur;
        cur += pt.cap;
    }
    if (c->cap_rows > 0) {
        c->counters[0]++;
        c->counters[3] += cur;
    }
    cand_free_arena(c);  // (hipFree waits for the device: the copies above and every scan that reads the old rows)
    c->vecs = nv;
    c->norms = nn;
    c->ids = ni;
    c->cap_rows = cap;
    c->used_rows = cur;
    p->free_ext.clear();
    c->table_dirty = true;
    return QK_OK;
}

void pool_free(qk_pool *p) {
    if (p->ev) hipEventDestroy(p->ev);
    if (p->st) {  // (not qk_store_destroy: every hipFree waits for the device)
        qk_store *c = p->st;
        cand_free_arena(c);
        if (c->d_off) hipFree(c->d_off);
        if (c->d_size) hipFree(c->d_size);
        if (c->rowmajor) hipFree(c->rowmajor);
        delete c;
    }
    (void)hipGetLastError();
    delete p;
}

// One admission: the U distinct filters `fs` of a call (masks current on ctx's stream, counts read: cand_rows), of which those
// without a valid slot are gathered -- evictions, extents, one launch series per chunk of entries, the table.  The caller has
// checked the budget (`evict`: the slots to give up, in order).
int pool_admit(qk_ctx *ctx, qk_store *s, qk_pool *p, const std::vector<qk_filter *> &fs, const std::vector<int64_t> &evict, int64_t pool_rows) {
    hipStream_t st = ctx->stream;
    qk_store *c = p->st;
    std::vector<qk_filter *> todo;
    int64_t need = 0;
    for (qk_filter *f : fs)
        if (!pool_slot_valid(p, f)) {
            todo.push_back(f);
            need += qk_round_up64(f->cand_rows, 16);
        }
    for (int64_t slot : evict) {
        pool_free_slot(p, slot);
        p->evictions++;
    }
    // (an arena that grew under a larger budget, or none, is brought back under this call's bound)
    const bool shrink = pool_rows > 0 && c->cap_rows > std::max<int64_t>(2 * pool_rows, 1024) / 16 * 16;
    if (todo.empty() && !shrink) return QK_OK;
    // behind the last admission on another context (its gather wrote the arena this one writes).  Like cand_ev the event covers
    // admissions only, not the scans that read the rows: the rule of the header that nobody changes the store while searches are
    // in flight covers the pool of the store too
    if (p->ev_ctx && p->ev_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, p->ev, 0));
    // slots: the lowest free numbers; extents: first fit, or everything packed into a fresh arena
    std::vector<int64_t> slot_of(todo.size());
    {
        int64_t next = 0;
        for (size_t i = 0; i < todo.size(); i++) {
            while (next < (int64_t)p->slots.size() && p->slots[next].used) next++;
            if (next == (int64_t)p->slots.size()) {
                p->slots.emplace_back();
                c->parts.emplace_back();
            }
            slot_of[i] = next;
            p->slots[next].used = true;  // (filled in below)
        }
    }
    std::vector<int64_t> ext(todo.size(), -1);
    bool fits = c->vecs != nullptr && !shrink;
    {
        const auto saved_free = p->free_ext;
        const int64_t saved_used = c->used_rows;
        for (size_t i = 0; i < todo.size() && fits; i++) {
            ext[i] = pool_take_extent(p, qk_round_up64(todo[i]->cand_rows, 16));
            fits = ext[i] >= 0;
        }
        if (!fits) {
            p->free_ext = saved_free;
            c->used_rows = saved_used;
        }
    }
    if (!fits) {
        const int64_t tot = p->rows + need;
        int64_t cap = qk_round_up64(std::max<int64_t>(tot + tot / 4, 1024), 16);  // (at least 1024 rows, like every arena)
        if (pool_rows > 0) cap = std::max(tot, std::min(cap, std::max<int64_t>(2 * pool_rows, 1024) / 16 * 16));
        else cap = std::max(cap, c->cap_rows);
        const int rc = pool_repack(ctx, p, cap);
        if (rc != QK_OK) {
            for (size_t i = 0; i < todo.size(); i++) p->slots[slot_of[i]].used = false;
            return rc;
        }
        for (size_t i = 0; i < todo.size(); i++) ext[i] = pool_take_extent(p, qk_round_up64(todo[i]->cand_rows, 16));
    }
    for (size_t i = 0; i < todo.size(); i++) {
        qk_filter *f = todo[i];
        PoolSlot &sl = p->slots[slot_of[i]];
        sl.serial = f->serial;
        sl.n = f->cand_rows;
        qk_part &pt = c->parts[slot_of[i]];
        pt = qk_part();
        pt.present = true;
        pt.row_off = ext[i];
        pt.size = f->cand_rows;
        pt.cap = qk_round_up64(f->cand_rows, 16);
        p->rows += pt.cap;
        p->nused++;
        p->builds++;
        f->pool_slot = slot_of[i];
    }
    c->table_dirty = true;
    // the launch series, in chunks whose block counts and offsets stay under 64 MiB of workspace (2 (nb + 1) words per entry:
    // 400 entries per chunk at 10M rows)
    std::vector<PoolAdmit> tab;
    const int64_t nwords = s->cap_rows / 16;  // (every mask was built for this capacity: filter_current)
    const int64_t nb = (nwords + QK_CAND_BLOCK - 1) / QK_CAND_BLOCK;
    const int64_t per_entry = (2 * nb + 1) * (int64_t)sizeof(int64_t);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)64 << 20) / per_entry));
    std::vector<PoolAdmit> live;
    for (size_t i = 0; i < todo.size(); i++)
        if (todo[i]->cand_rows > 0) live.push_back(PoolAdmit{todo[i]->mask, todo[i]->cand_rows, ext[i], 0});
    for (size_t i0 = 0; i0 < live.size(); i0 += (size_t)chunk) {
        const int M = (int)std::min<size_t>((size_t)chunk, live.size() - i0);
        tab.assign(live.begin() + i0, live.begin() + i0 + M);
        int64_t tiles = 0;
        for (PoolAdmit &e : tab) {
            e.tile0 = tiles;
            tiles += (e.n + 15) / 16;
        }
        tab.push_back(PoolAdmit{nullptr, 0, 0, tiles});
        const size_t tab_bytes = (size_t)(M + 1) * sizeof(PoolAdmit);
        QK_TRY(qk_ws_reserve(ctx, tab_bytes + (size_t)M * per_entry + 1024));
        PoolAdmit *d_tab = (PoolAdmit *)qk_ws_alloc(ctx, tab_bytes);
        int64_t *cnt = (int64_t *)qk_ws_alloc(ctx, (size_t)M * nb * sizeof(int64_t));
        int64_t *boff = (int64_t *)qk_ws_alloc(ctx, (size_t)M * (nb + 1) * sizeof(int64_t));
        if (!d_tab || !cnt || !boff) QK_FAIL(QK_ERR_OOM, "qk_search_filtered_exact_batch: workspace exhausted");
        // (pageable source: copied out when the call returns)
        QK_HIP(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pool_block_counts, dim3((unsigned)((nb + 15) / 16), (unsigned)M), dim3(256), 0, st, (const PoolAdmit *)d_tab, nwords, nb, cnt);
        hipLaunchKernelGGL(k_pool_block_scan, dim3((unsigned)M), dim3(1024), 0, st, (const int64_t *)cnt, boff, nb);
        PoolGatherParams G;
        G.tab = d_tab;
        G.M = M;
        G.ntiles = tiles;
        G.nwords = nwords;
        G.boff = boff;
        G.nb = nb;
        G.nblk = s->nblk;
        G.sv = (const float4 *)s->vecs;
        G.sn = (const uint32_t *)s->norms;
        G.si = s->ids;
        G.src_rows = s->cap_rows;
        G.dv = (float4 *)c->vecs;
        G.dn = (uint32_t *)c->norms;
        G.di = c->ids;
        G.dst_rows = c->cap_rows;
        hipLaunchKernelGGL(k_pool_gather, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, G);
        QK_HIP(hipGetLastError());
    }
    if (!p->ev) QK_HIP(hipEventCreateWithFlags(&p->ev, hipEventDisableTiming));
    QK_HIP(hipEventRecord(p->ev, st));
    p->ev_ctx = ctx;
    return QK_OK;
}

}  // namespace

void qk_pool_destroy(qk_store *s) {
    if (!s->pool) return;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pools.erase(s->uid);
    }
    pool_free(s->pool);
    s->pool = nullptr;
}

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
    if (f->pool_slot >= 0) pool_release(f);
    if (f->cand_ev) hipEventDestroy(f->cand_ev);
    if (f->cand) {  // (not qk_store_destroy: its context may be gone; every hipFree waits for the device)
        qk_store *c = f->cand;
        cand_free_arena(c);
        if (c->d_off) hipFree(c->d_off);
        if (c->d_size) hipFree(c->d_size);
        if (c->rowmajor) hipFree(c->rowmajor);
        delete c;
    }
    if (f->d_ids) hipFree(f->d_ids);
    if (f->d_sets) hipFree(f->d_sets);
    if (f->d_allowed) hipFree(f->d_allowed);
    (void)hipGetLastError();
    delete f;
    return QK_OK;
}

int qk_filter_info(qk_filter *f, int64_t *n_ids, int64_t *rows_allowed, uint64_t *store_version, int64_t *rebuilds, int64_t *device_bytes) {
    if (!f) QK_FAIL(QK_ERR_INVALID, "qk_filter_info: null filter");
    QK_HIP(hipSetDevice(f->device));
    if (n_ids) *n_ids = f->kind != QK_FILTER_KIND_IDS ? -1 : f->n_ids;
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
        else if (f->kind == QK_FILTER_KIND_EXPR)  // (the mask and the set buffer; the clause table travels in the kernel arguments)
            *device_bytes = (int64_t)(f->mask_words * sizeof(uint16_t) + std::max<int64_t>(f->sets_len, 1) * sizeof(int64_t));
        else *device_bytes = (int64_t)(f->mask_words * sizeof(uint16_t) + std::max<int64_t>(f->n_ids, 1) * sizeof(int64_t) + 8);
        *device_bytes += (int64_t)(f->counts_cap * sizeof(int32_t));  // (adaptive probing: once a call has derived them)
        *device_bytes += cand_device_bytes(f);                        // (exact search: once a call has derived the store)
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

// ---- exact search --------------------------------------------------------------------------------------------------------------
int qk_filter_candidate_rows(qk_ctx *ctx, qk_store *s, qk_filter *f, int64_t *rows) {
    if (!ctx || !s || !f || !rows) QK_FAIL(QK_ERR_INVALID, "qk_filter_candidate_rows: null argument");
    QK_HIP(hipSetDevice(ctx->device));
    const uint16_t *mask = nullptr;
    QK_TRY(qk_filter_ensure(ctx, s, f, &mask));
    return cand_count(f, rows);
}

int qk_search_filtered_exact(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, int k, int metric, qk_filter *f, int64_t max_rows,
                             int64_t *out_ids, float *out_dist, int mem, qk_timing *timing) {
    if (!ctx || !s || !f || (Q > 0 && (!x || !out_ids))) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_exact: null argument");
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_exact: k must be positive");
    if (k > QK_MAX_WIDE_K) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_search_filtered_exact: k=%d exceeds %d", k, QK_MAX_WIDE_K);
    if (max_rows < 0) QK_FAIL(QK_ERR_INVALID, "qk_search_filtered_exact: max_rows must not be negative");
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    QK_TRY(qk_check_overflow(ctx));
    QK_HIP(hipSetDevice(ctx->device));
    if (timing) memset(timing, 0, sizeof(*timing));
    // (a mask build and the gather lie in front of the scan's events: part of total_ms only, like the cut of an adaptive call)
    const bool tm = ctx->timing && timing && Q > 0;
    if (tm) QK_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    const uint16_t *mask = nullptr;
    QK_TRY(qk_filter_ensure(ctx, s, f, &mask));
    int64_t n = 0;
    QK_TRY(cand_count(f, &n));
    if (max_rows > 0 && n > max_rows)
        QK_FAIL(QK_ERR_UNSUPPORTED, "qk_search_filtered_exact: the filter has %lld candidates, max_rows=%lld", (long long)n, (long long)max_rows);
    if (Q <= 0) return QK_OK;
    QK_TRY(cand_ensure(ctx, s, f, n, max_rows));
    QK_TRY(qk_run_search(ctx, nullptr, f->cand, x, Q, nullptr, 0, 0, k, metric, out_ids, out_dist, mem, timing, false, false));
    if (tm) {
        float ms = 0.f;
        QK_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[7]));
        timing->total_ms = ms;
    }
    return QK_OK;
}

int qk_filter_exact_info(qk_filter *f, int64_t *rows, int64_t *builds, int64_t *device_bytes) {
    if (!f) QK_FAIL(QK_ERR_INVALID, "qk_filter_exact_info: null filter");
    if (rows) *rows = f->cand ? f->cand->ntotal : 0;
    if (builds) *builds = f->cand_builds;
    if (device_bytes) *device_bytes = cand_device_bytes(f);
    return QK_OK;
}

// ---- exact search, one filter per query ----------------------------------------------------------------------------------------
int qk_search_filtered_exact_batch(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, int k, int metric, qk_filter *const *filters, int F,
                                   const int32_t *qfilter, int64_t max_rows, int64_t pool_rows, int64_t *out_ids, float *out_dist, int mem,
                                   qk_timing *timing) {
    const char *who = "qk_search_filtered_exact_batch";
    if (!ctx || !s || (Q > 0 && (!x || !out_ids || !qfilter))) QK_FAIL(QK_ERR_INVALID, "%s: null argument", who);
    if (!filters || F < 1) QK_FAIL(QK_ERR_INVALID, "%s: at least one filter is required (F=%d)", who, F);
    if (F > QK_MAX_BATCH_FILTERS) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: F=%d exceeds QK_MAX_BATCH_FILTERS=%d", who, F, QK_MAX_BATCH_FILTERS);
    for (int i = 0; i < F; i++)
        if (!filters[i]) QK_FAIL(QK_ERR_INVALID, "%s: filter %d of %d is null", who, i, F);
    if (k <= 0) QK_FAIL(QK_ERR_INVALID, "%s: k must be positive", who);
    if (k > QK_MAX_WIDE_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds %d", who, k, QK_MAX_WIDE_K);
    if (max_rows < 0) QK_FAIL(QK_ERR_INVALID, "%s: max_rows must not be negative", who);
    if (pool_rows < 0) QK_FAIL(QK_ERR_INVALID, "%s: pool_rows must not be negative", who);
    if (metric != QK_METRIC_L2 && metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (mem == QK_MEM_HOST)
        for (int64_t i = 0; i < Q; i++)
            if (qfilter[i] < 0 || qfilter[i] >= F)
                QK_FAIL(QK_ERR_INVALID, "%s: qfilter[%lld]=%d is outside [0, F=%d)", who, (long long)i, (int)qfilter[i], F);
    for (int i = 0; i < F; i++) QK_TRY(filter_belongs(ctx, s, filters[i]));
    QK_TRY(qk_check_overflow(ctx));
    QK_HIP(hipSetDevice(ctx->device));
    if (timing) memset(timing, 0, sizeof(*timing));
    // (mask builds and the admission lie in front of the scan's events: part of total_ms only, like the single-filter call's)
    const bool tm = ctx->timing && timing && Q > 0;
    hipStream_t st = ctx->stream;
    if (tm) QK_HIP(hipEventRecord(ctx->ev[0], st));
    QK_TRY(qk_store_sync_table(s));  // once: every filter is compared with the same version
    // the distinct handles in the order of their first appearance (a handle listed twice shares one slot)
    std::vector<qk_filter *> fs;
    std::vector<int> uidx((size_t)F);
    {
        std::unordered_map<const qk_filter *, int> seen;
        for (int i = 0; i < F; i++) {
            auto it = seen.find(filters[i]);
            if (it == seen.end()) {
                it = seen.emplace(filters[i], (int)fs.size()).first;
                fs.push_back(filters[i]);
            }
            uidx[i] = it->second;
        }
    }
    for (qk_filter *f : fs) QK_TRY(filter_current(ctx, s, f));
    // the candidate counts nobody has read since the mask build: one kernel collects them, one copy behind one wait brings them
    {
        std::vector<qk_filter *> unread;
        for (qk_filter *f : fs)
            if (f->cand_rows < 0) unread.push_back(f);
        if (!unread.empty()) {
            const size_t M = unread.size();
            std::vector<const unsigned long long *> hp(M);
            for (size_t i = 0; i < M; i++) hp[i] = unread[i]->d_allowed;
            QK_TRY(qk_ws_reserve(ctx, M * 16 + 1024));
            const unsigned long long **d_p = (const unsigned long long **)qk_ws_alloc(ctx, M * 8);
            int64_t *d_n = (int64_t *)qk_ws_alloc(ctx, M * 8);
            if (!d_p || !d_n) QK_FAIL(QK_ERR_OOM, "%s: workspace exhausted", who);
            QK_HIP(hipMemcpyAsync((void *)d_p, hp.data(), M * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_pool_counts, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const unsigned long long *const *)d_p, (int)M, d_n);
            QK_HIP(hipGetLastError());
            std::vector<int64_t> hn(M);
            QK_HIP(hipMemcpyAsync(hn.data(), d_n, M * 8, hipMemcpyDeviceToHost, st));
            QK_HIP(hipStreamSynchronize(st));
            for (size_t i = 0; i < M; i++) unread[i]->cand_rows = hn[i];
        }
    }
    if (max_rows > 0)
        for (int i = 0; i < F; i++)
            if (filters[i]->cand_rows > max_rows)
                QK_FAIL(QK_ERR_UNSUPPORTED, "%s: filter %d of %d has %lld candidates, max_rows=%lld", who, i, F,
                        (long long)filters[i]->cand_rows, (long long)max_rows);
    for (int i = 0; i < F; i++)
        if (filters[i]->cand_rows > (int64_t)INT32_MAX - 16)
            QK_FAIL(QK_ERR_UNSUPPORTED, "%s: the %lld candidates of filter %d exceed a list's 2^31 rows", who, (long long)filters[i]->cand_rows, i);
    // the budget: what the call's own filters need must fit; slots nobody in this call names go, least recently named first
    qk_pool *p = s->pool;
    std::vector<int64_t> evict;
    if (pool_rows > 0) {
        int64_t named = 0, need = 0;
        std::vector<char> is_named(p ? p->slots.size() : 0, 0);
        for (qk_filter *f : fs) {
            const int64_t r = qk_round_up64(f->cand_rows, 16);
            named += r;
            if (pool_slot_valid(p, f)) is_named[f->pool_slot] = 1;
            else need += r;
        }
        if (named > pool_rows)
            QK_FAIL(QK_ERR_UNSUPPORTED, "%s: the filters of the call need %lld pool rows, pool_rows=%lld", who, (long long)named, (long long)pool_rows);
        if (p && p->rows + need > pool_rows) {
            std::vector<int64_t> cand;
            for (int64_t i = 0; i < (int64_t)p->slots.size(); i++)
                if (p->slots[i].used && !is_named[i]) cand.push_back(i);
            std::sort(cand.begin(), cand.end(), [&](int64_t a, int64_t b) {
                return p->slots[a].stamp != p->slots[b].stamp ? p->slots[a].stamp < p->slots[b].stamp : a < b;
            });
            int64_t total = p->rows + need;
            for (int64_t i : cand) {
                if (total <= pool_rows) break;
                total -= p->st->parts[i].cap;
                evict.push_back(i);
            }
        }
    }
    if (!p) {
        p = new qk_pool();
        const int rc = qk_store_create(ctx, s->d, &p->st);
        if (rc != QK_OK) {
            delete p;
            return rc;
        }
        s->pool = p;
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pools[s->uid] = p;
    }
    qk_store *c = p->st;
    c->ctx = ctx;
    QK_TRY(pool_admit(ctx, s, p, fs, evict, pool_rows));
    p->clock++;
    for (qk_filter *f : fs) p->slots[f->pool_slot].stamp = p->clock;
    QK_TRY(pool_publish(ctx, p, s));
    if (p->ev_ctx && p->ev_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, p->ev, 0));  // admitted on another context's stream
    if (Q <= 0) return QK_OK;
    // query i scans the list of its filter: P = 1 of the ordinary partition scan (the wide-k pipeline beyond QK_MAX_K)
    std::vector<int64_t> h_pids;
    const int64_t *pids = nullptr;
    if (mem == QK_MEM_HOST) {  // (range-checked above)
        h_pids.resize((size_t)Q);
        for (int64_t i = 0; i < Q; i++) h_pids[i] = fs[uidx[qfilter[i]]]->pool_slot;
        pids = h_pids.data();
    } else {
        const size_t tab_bytes = (size_t)QK_MAX_BATCH_FILTERS * sizeof(int64_t);
        const size_t need = tab_bytes + (size_t)Q * sizeof(int64_t);
        if (need > ctx->pool_buf_cap) {
            // (a scan in flight may still read the old pids: hipFree waits for the device)
            if (ctx->pool_buf) QK_HIP(hipFree(ctx->pool_buf));
            ctx->pool_buf = nullptr;
            ctx->pool_buf_cap = 0;
            ctx->pool_key.clear();
            const size_t cap = tab_bytes + std::max<size_t>((size_t)(Q + Q / 2), 1024) * sizeof(int64_t);
            if (hipMalloc((void **)&ctx->pool_buf, cap) != hipSuccess) {
                (void)hipGetLastError();
                QK_FAIL(QK_ERR_OOM, "%s: no memory for the list numbers of %lld queries", who, (long long)Q);
            }
            ctx->pool_buf_cap = cap;
        }
        std::vector<int64_t> key((size_t)F);
        for (int i = 0; i < F; i++) key[i] = fs[uidx[i]]->pool_slot;
        if (key != ctx->pool_key) {  // (pageable source: copied out when the call returns)
            QK_HIP(hipMemcpyAsync(ctx->pool_buf, key.data(), (size_t)F * sizeof(int64_t), hipMemcpyHostToDevice, st));
            ctx->pool_key = std::move(key);
        }
        int64_t *d_pids = (int64_t *)(ctx->pool_buf + tab_bytes);
        hipLaunchKernelGGL(k_pool_pids, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, qfilter, Q, F, (const int64_t *)ctx->pool_buf, d_pids);
        QK_HIP(hipGetLastError());
        pids = d_pids;
    }
    QK_TRY(qk_run_search(ctx, nullptr, c, x, Q, pids, 1, 0, k, metric, out_ids, out_dist, mem, timing, false, false));
    if (tm) {
        float ms = 0.f;
        QK_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[7]));
        timing->total_ms = ms;
    }
    return QK_OK;
}

int qk_store_exact_pool_info(qk_store *s, int64_t *slots, int64_t *rows, int64_t *cap_rows, int64_t *builds, int64_t *evictions,
                             int64_t *device_bytes) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_exact_pool_info: null store");
    const qk_pool *p = s->pool;
    if (slots) *slots = p ? p->nused : 0;
    if (rows) *rows = p ? p->rows : 0;
    if (cap_rows) *cap_rows = p ? p->st->cap_rows : 0;
    if (builds) *builds = p ? p->builds : 0;
    if (evictions) *evictions = p ? p->evictions : 0;
    if (device_bytes) *device_bytes = p ? pool_device_bytes(p) : 0;
    return QK_OK;
}

int qk_store_exact_pool_drop(qk_store *s) {
    if (!s) QK_FAIL(QK_ERR_INVALID, "qk_store_exact_pool_drop: null store");
    QK_HIP(hipSetDevice(s->ctx->device));
    qk_pool_destroy(s);
    return QK_OK;
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
