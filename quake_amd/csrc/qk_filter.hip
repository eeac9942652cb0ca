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
#include <cstring>
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
    f->cand_built = false;    // (exact search: the candidate store too, and the count is read again)
    f->cand_rows = -1;
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
