// qk_attr.hip -- attribute filters (include/quake_hip.h, "attribute filters"): int64 columns keyed by vector id, kept on the device,
// and the kernel that turns (stored ids x columns x clauses) into the row mask of a qk_filter (qk_filter.hip owns the mask, its
// stamp and every consumer; the scan kernels do not know where a mask came from).
//
// A column has one of two layouts behind one lookup.  The DIRECT TABLE -- values[id] and one presence bit per id -- is kept while
// max_id < 4 * n_ids + 65536: at most ~twice the bytes of the pairs plus half a megabyte, a rule about memory, not speed.
// Otherwise SORTED PAIRS: ascending ids with their values, one binary search per lookup.  Every set / unset re-decides and converts.
// No device library on any path: a request is de-duplicated on the host; the pairs have a host mirror that an upsert merges into
// and uploads; a table update is a scatter of (id, value) and of whole presence words -- the host mirrors the presence bits, so it
// knows which ids are new and sends every touched word once, complete: no atomic decides a value or a bit.
//
// Errors.  Arguments are checked before anything is touched (a negative id changes nothing).  A failure behind that -- out of
// device memory, a HIP error -- can strike after the host mirror took the update and before the device did: the call returns the
// error, the version is not bumped, and the column's contents are then undefined; destroy it (a mask build or a get refuses a
// column whose device arrays are gone: no kernel reads freed or null memory).  Host-to-device copies come from pageable memory
// and are stream-ordered: as everywhere in this library (qk_store.hip, qk_kmeans.hip) they rely on the runtime having staged a
// pageable source when hipMemcpyAsync returns.
#include "qk_attr.h"

#include <algorithm>
#include <atomic>
#include <new>
#include <numeric>
#include <vector>

qk_attr_data::~qk_attr_data() {
    // (runs wherever the last owner goes -- qk_attr_destroy, qk_filter_destroy -- so the caller's current device is put back)
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    hipSetDevice(device);
    if (upd_ev) {
        hipEventSynchronize(upd_ev);
        hipEventDestroy(upd_ev);
    }
    // (hipFree waits for the device: no build still reads the column)
    if (t_vals) hipFree(t_vals);
    if (t_bits) hipFree(t_bits);
    if (s_ids) hipFree(s_ids);
    if (s_vals) hipFree(s_vals);
    if (stage) hipFree(stage);
    if (rv_vals) hipFree(rv_vals);
    if (rv_has) hipFree(rv_has);
    if (rv_ev) hipEventDestroy(rv_ev);
    if (have_cur && cur != device) hipSetDevice(cur);
    (void)hipGetLastError();
}

namespace {

__device__ __forceinline__ bool where_op(int op, int64_t a, int64_t b, int64_t v) {
    switch (op) {
    case QK_OP_RANGE: return a <= v && v <= b;
    case QK_OP_NOT_RANGE: return !(a <= v && v <= b);
    case QK_OP_ANY_BITS: return (v & a) != 0;
    case QK_OP_ALL_BITS: return (v & a) == a;
    default: return (v & a) == 0;  // QK_OP_NO_BITS (the host admits no other op)
    }
}

// ---- the mask of a predicate ----------------------------------------------------------------------------------------------------
struct WhereClause {
    AttrCol col;
    int op;
    int64_t a, b;
};

struct WhereBuildParams {
    const int64_t *ids;      // arena ids
    const int64_t *pt_off;   // [npids] first arena row of every list
    const int32_t *pt_size;  // [npids] rows, -1 = absent
    uint16_t *mask;
    int64_t mask_words;
    unsigned long long *allowed;
    int nc;
    WhereClause c[QK_MAX_CLAUSES];
};

#ifndef QK_WB_U
#define QK_WB_U 4  // (-DQK_WB_U=1 / 2 / 8: the side builds DESIGN.md 5.9 compares)
#endif
constexpr int WB_U = QK_WB_U;  // rows in flight per lane

// k_filter_build's sibling: the same grid -- blockIdx.x = list, blockIdx.y strides over its chunks, here of WB_U x 16 tiles -- and
// the same writer rule: the word of a tile is the ballot of the 16 lanes that looked at its rows, stored by the first of them; rows
// behind a list's size keep the memset's 0; one atomic per wave counts the candidates.  Per row: the id once, then clause by clause
// the value of the id in the clause's column and the op, ANDed; a row is done at its first failing clause (a wave when all its
// rows are), which cannot change the result: the clauses are a conjunction.
__global__ __launch_bounds__(256) void k_filter_build_where(WhereBuildParams F) {
    const int p = blockIdx.x;
    const int size = F.pt_size[p];
    if (size <= 0) return;
    const int64_t row_off = F.pt_off[p];
    const int ntl = (size + 15) >> 4;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int sub = threadIdx.x >> 4;  // tile of a 16-tile chunk
    unsigned long long mine = 0;
    for (int t0 = blockIdx.y * 16 * WB_U; t0 < ntl; t0 += gridDim.y * 16 * WB_U) {
        int64_t id[WB_U];
        bool ok[WB_U];
#pragma unroll
        for (int u = 0; u < WB_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const int row = tile * 16 + j;
            ok[u] = tile < ntl && row < size;
            id[u] = F.ids[row_off + (ok[u] ? row : 0)];  // (unconditional: the loads leave together; row 0 exists)
        }
        // (not unrolled: the clause index is wave-uniform, a clause's parameters are scalar loads from the kernel arguments;
        // unrolled, the eight clauses' worth of them were live at once and 42 SGPRs spilled)
#pragma unroll 1
        for (int ci = 0; ci < F.nc; ci++) {
            bool any = false;
#pragma unroll
            for (int u = 0; u < WB_U; u++) any = any || ok[u];
            if (!__any(any)) break;
            int64_t v[WB_U];
            bool has[WB_U];
            attr_lookup<WB_U>(F.c[ci].col, id, ok, v, has);
#pragma unroll
            for (int u = 0; u < WB_U; u++) ok[u] = ok[u] && has[u] && where_op(F.c[ci].op, F.c[ci].a, F.c[ci].b, v[u]);
        }
#pragma unroll
        for (int u = 0; u < WB_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const uint64_t b = __ballot(ok[u]);
            const uint32_t word = (uint32_t)((b >> (16 * (lane >> 4))) & 0xFFFFull);
            const int64_t w = (row_off >> 4) + tile;
            if (j == 0 && tile < ntl && w < F.mask_words) {
                F.mask[w] = (uint16_t)word;
                mine += __popc(word);
            }
        }
    }
    // one atomic per wave
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane == 0 && mine) atomicAdd(F.allowed, mine);
}

// ---- the mask of an expression: an OR of conjunctions, with value sets ---------------------------------------------------------
struct ExprClause {
    AttrCol col;
    int op;
    int64_t a, b;        // the five ops of where_op
    const int64_t *set;  // IN_SET / NOT_IN_SET: the clause's slice of the filter's set buffer, ascending and distinct
    int64_t n_set;       //                      its length, 0 = the empty set (set is not read)
};

// (the clause table travels in the kernel arguments: 32 x 80 bytes + the rest < 4 KB; term and clause numbers are wave-uniform, so a
// clause's parameters are scalar loads from there, as in k_filter_build_where)
struct ExprBuildParams {
    const int64_t *ids;
    const int64_t *pt_off;
    const int32_t *pt_size;
    uint16_t *mask;
    int64_t mask_words;
    unsigned long long *allowed;
    int nt;
    int term_end[QK_MAX_TERMS];  // term t is the clauses [term_end[t - 1], term_end[t])
    ExprClause c[QK_MAX_EXPR_CLAUSES];
};

// is v[u] an element of set[0 .. n), n >= 1: the sorted layout's search of attr_lookup -- the last element <= v, all U searches in
// step, every probe inside [0, n) -- and one comparison.  live[u] == false: the probes go to element 0 and the answer is "no".
template <int U>
__device__ __forceinline__ void set_member(const int64_t *set, int64_t n, const int64_t (&v)[U], const bool (&live)[U], bool (&in)[U]) {
    int64_t base[U];
#pragma unroll
    for (int u = 0; u < U; u++) base[u] = 0;
    for (int64_t len = n; len > 1;) {
        const int64_t half = len >> 1;
        int64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) k[u] = set[base[u] + half];
#pragma unroll
        for (int u = 0; u < U; u++) base[u] += (live[u] && k[u] <= v[u]) ? half : 0;
        len -= half;
    }
    int64_t k[U];
#pragma unroll
    for (int u = 0; u < U; u++) k[u] = set[base[u]];
#pragma unroll
    for (int u = 0; u < U; u++) in[u] = live[u] && k[u] == v[u];
}

// k_filter_build_where's sibling for qk_filter_create_expr: the same grid, the same writer rule, the same WB_U ids in flight.  Per
// lane and row two flags: acc -- an earlier term held -- and ok -- alive in the current term.  A term starts with the valid rows
// no earlier term accepted and ANDs its clauses like k_filter_build_where; the wave skips a term when none of its rows is left
// undecided and a clause when none is alive in the term.  OR and AND commute: neither order can change a bit of the mask.
__global__ __launch_bounds__(256) void k_filter_build_expr(ExprBuildParams F) {
    const int p = blockIdx.x;
    const int size = F.pt_size[p];
    if (size <= 0) return;
    const int64_t row_off = F.pt_off[p];
    const int ntl = (size + 15) >> 4;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int sub = threadIdx.x >> 4;  // tile of a 16-tile chunk
    unsigned long long mine = 0;
    for (int t0 = blockIdx.y * 16 * WB_U; t0 < ntl; t0 += gridDim.y * 16 * WB_U) {
        int64_t id[WB_U];
        bool valid[WB_U], acc[WB_U];
#pragma unroll
        for (int u = 0; u < WB_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const int row = tile * 16 + j;
            valid[u] = tile < ntl && row < size;
            acc[u] = false;
            id[u] = F.ids[row_off + (valid[u] ? row : 0)];  // (unconditional: the loads leave together; row 0 exists)
        }
        // (neither loop unrolled: see k_filter_build_where)
        int ci = 0;
#pragma unroll 1
        for (int t = 0; t < F.nt; t++) {
            const int end = F.term_end[t];
            bool ok[WB_U], open = false;
#pragma unroll
            for (int u = 0; u < WB_U; u++) {
                ok[u] = valid[u] && !acc[u];
                open = open || ok[u];
            }
            if (!__any(open)) break;  // (every valid row of the wave is accepted: no later term can change one)
#pragma unroll 1
            for (; ci < end; ci++) {
                bool any = false;
#pragma unroll
                for (int u = 0; u < WB_U; u++) any = any || ok[u];
                if (!__any(any)) break;
                int64_t v[WB_U];
                bool has[WB_U];
                attr_lookup<WB_U>(F.c[ci].col, id, ok, v, has);
                const int op = F.c[ci].op;
                if (op < QK_OP_IN_SET) {
#pragma unroll
                    for (int u = 0; u < WB_U; u++) ok[u] = ok[u] && has[u] && where_op(op, F.c[ci].a, F.c[ci].b, v[u]);
                } else {
                    bool in[WB_U];
#pragma unroll
                    for (int u = 0; u < WB_U; u++) {
                        ok[u] = ok[u] && has[u];  // (an id without a value fails NOT_IN_SET too)
                        in[u] = false;
                    }
                    const int64_t n_set = F.c[ci].n_set;
                    if (n_set > 0) set_member<WB_U>(F.c[ci].set, n_set, v, ok, in);  // (the empty set: no load)
                    const bool want = op == QK_OP_IN_SET;
#pragma unroll
                    for (int u = 0; u < WB_U; u++) ok[u] = ok[u] && in[u] == want;
                }
            }
            ci = end;
#pragma unroll
            for (int u = 0; u < WB_U; u++) acc[u] = acc[u] || ok[u];
        }
#pragma unroll
        for (int u = 0; u < WB_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const uint64_t b = __ballot(acc[u]);
            const uint32_t word = (uint32_t)((b >> (16 * (lane >> 4))) & 0xFFFFull);
            const int64_t w = (row_off >> 4) + tile;
            if (j == 0 && tile < ntl && w < F.mask_words) {
                F.mask[w] = (uint16_t)word;
                mine += __popc(word);
            }
        }
    }
    // one atomic per wave
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if (lane == 0 && mine) atomicAdd(F.allowed, mine);
}

// qk_attr_get: the values as the device holds them, through the lookup the mask build uses
__global__ __launch_bounds__(256) void k_attr_get(AttrCol c, const int64_t *ids, int64_t n, int64_t *vals, int32_t *found) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live[1] = {i < n};
    const int64_t id[1] = {live[0] ? ids[i] : 0};
    int64_t v[1];
    bool has[1];
    attr_lookup<1>(c, id, live, v, has);
    if (live[0]) {
        vals[i] = has[0] ? v[0] : 0;
        found[i] = has[0] ? 1 : 0;
    }
}

// a table update: the host has de-duplicated the ids (one writer per value) and sends every touched presence word complete
__global__ __launch_bounds__(256) void k_attr_scatter(int64_t *t_vals, uint32_t *t_bits, int64_t cap, const int64_t *ids, const int64_t *vals,
                                                      int64_t n, const int64_t *widx, const uint32_t *wval, int64_t nw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int64_t id = ids[i];
        if ((uint64_t)id < (uint64_t)cap) t_vals[id] = vals[i];
    }
    if (i < nw) {
        const int64_t w = widx[i];
        if ((uint64_t)w < (uint64_t)(cap >> 5)) t_bits[w] = wval[i];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
constexpr int64_t TABLE_MIN = 1024;

inline bool want_table(int64_t max_id, int64_t n_ids) { return max_id < 4 * n_ids + 65536; }

inline bool bit_of(const std::vector<uint32_t> &b, int64_t id) {
    return (size_t)(id >> 5) < b.size() && ((b[(size_t)(id >> 5)] >> (id & 31)) & 1u);
}

int fetch_i64(qk_ctx *c, const int64_t *p, int64_t n, int mem, std::vector<int64_t> &h) {
    h.resize((size_t)n);
    if (n == 0) return QK_OK;
    if (mem == QK_MEM_DEVICE) {
        QK_HIP(hipStreamSynchronize(c->stream));
        QK_HIP(hipMemcpy(h.data(), p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    } else {
        std::copy(p, p + n, h.begin());
    }
    return QK_OK;
}

template <typename T>
int dev_alloc(T **p, int64_t count, const char *what) {
    if (hipMalloc((void **)p, (size_t)std::max<int64_t>(count, 1) * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        QK_FAIL(QK_ERR_OOM, "qk_attr: no device memory for %s (%lld entries)", what, (long long)count);
    }
    return QK_OK;
}

void free_table(qk_attr_data &d) {
    if (d.t_vals) hipFree(d.t_vals);
    if (d.t_bits) hipFree(d.t_bits);
    d.t_vals = nullptr;
    d.t_bits = nullptr;
    d.t_cap = 0;
    std::vector<uint32_t>().swap(d.h_bits);
}

void free_sorted(qk_attr_data &d) {
    if (d.s_ids) hipFree(d.s_ids);
    if (d.s_vals) hipFree(d.s_vals);
    d.s_ids = d.s_vals = nullptr;
    d.s_cap = 0;
    std::vector<int64_t>().swap(d.h_ids);
    std::vector<int64_t>().swap(d.h_vals);
}

// a table that covers ids [0, need): kept, or grown geometrically with the old values copied over (the presence words come from
// the host mirror, which the caller uploads when *grown)
int table_reserve(qk_attr_data &d, hipStream_t st, int64_t need, bool *grown) {
    *grown = false;
    if (d.t_vals && need <= d.t_cap) return QK_OK;
    const int64_t cap = qk_round_up64(std::max<int64_t>(std::max<int64_t>(need, TABLE_MIN), d.t_cap + d.t_cap / 2), 32);
    int64_t *nv = nullptr;
    uint32_t *nb = nullptr;
    QK_TRY(dev_alloc(&nv, cap, "a value table"));
    if (dev_alloc(&nb, cap / 32, "presence bits") != QK_OK) {
        hipFree(nv);
        return QK_ERR_OOM;
    }
    if (d.t_vals && d.t_cap > 0) {
        const hipError_t e = hipMemcpyAsync(nv, d.t_vals, (size_t)d.t_cap * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {  // (the old table stays the column's)
            hipFree(nv);
            hipFree(nb);
            QK_FAIL(QK_ERR_HIP, "qk_attr: copying the value table -> %s", hipGetErrorString(e));
        }
    }
    // (hipFree waits for the device: the copy is done, no build reads the old table)
    if (d.t_vals) hipFree(d.t_vals);
    if (d.t_bits) hipFree(d.t_bits);
    d.t_vals = nv;
    d.t_bits = nb;
    d.t_cap = cap;
    d.h_bits.resize((size_t)(cap / 32), 0u);
    *grown = true;
    return QK_OK;
}

int upload_bits(qk_attr_data &d, hipStream_t st) {
    // stream-ordered; the source is pageable, so it has been copied out when the call returns
    QK_HIP(hipMemcpyAsync(d.t_bits, d.h_bits.data(), d.h_bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return QK_OK;
}

// (ids, vals) -- ascending, distinct, all < t_cap -- and the presence words `words` (ascending, distinct) to the device table
int table_scatter(qk_attr_data &d, hipStream_t st, const std::vector<int64_t> &ids, const std::vector<int64_t> &vals,
                  const std::vector<int64_t> &words) {
    const int64_t n = (int64_t)vals.size(), nw = (int64_t)words.size();
    if (n == 0 && nw == 0) return QK_OK;
    const size_t bytes = (size_t)(2 * n + nw) * sizeof(int64_t) + (size_t)nw * sizeof(uint32_t);
    if (bytes > d.stage_cap) {
        if (d.stage) hipFree(d.stage);
        d.stage = nullptr;
        d.stage_cap = 0;
        const size_t cap = std::max<size_t>(bytes + bytes / 2, 4096);
        QK_TRY(dev_alloc(&d.stage, (int64_t)cap, "update staging"));
        d.stage_cap = cap;
    }
    std::vector<char> h(bytes);
    int64_t *h_ids = (int64_t *)h.data(), *h_vals = h_ids + n, *h_widx = h_vals + n;
    uint32_t *h_wval = (uint32_t *)(h_widx + nw);
    std::copy(ids.begin(), ids.begin() + n, h_ids);
    std::copy(vals.begin(), vals.end(), h_vals);
    for (int64_t i = 0; i < nw; i++) {
        h_widx[i] = words[(size_t)i];
        h_wval[i] = d.h_bits[(size_t)words[(size_t)i]];
    }
    QK_HIP(hipMemcpyAsync(d.stage, h.data(), bytes, hipMemcpyHostToDevice, st));
    const int64_t *g_ids = (const int64_t *)d.stage, *g_vals = g_ids + n, *g_widx = g_vals + n;
    const uint32_t *g_wval = (const uint32_t *)(g_widx + nw);
    const int64_t m = std::max(n, nw);
    hipLaunchKernelGGL(k_attr_scatter, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d.t_vals, d.t_bits, d.t_cap, g_ids, g_vals, n,
                       g_widx, g_wval, nw);
    QK_HIP(hipGetLastError());
    return QK_OK;
}

// the host mirror of the pairs to the device, grown geometrically
int upload_sorted(qk_attr_data &d, hipStream_t st) {
    const int64_t n = (int64_t)d.h_ids.size();
    if (n > d.s_cap || !d.s_ids) {
        if (d.s_ids) hipFree(d.s_ids);
        if (d.s_vals) hipFree(d.s_vals);
        d.s_ids = d.s_vals = nullptr;
        d.s_cap = 0;
        const int64_t cap = std::max<int64_t>(n + n / 2, 1024);
        QK_TRY(dev_alloc(&d.s_ids, cap, "sorted ids"));
        if (dev_alloc(&d.s_vals, cap, "sorted values") != QK_OK) {
            hipFree(d.s_ids);
            d.s_ids = nullptr;
            return QK_ERR_OOM;
        }
        d.s_cap = cap;
    }
    if (n > 0) {
        QK_HIP(hipMemcpyAsync(d.s_ids, d.h_ids.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        QK_HIP(hipMemcpyAsync(d.s_vals, d.h_vals.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    return QK_OK;
}

// the column's contents as ascending pairs on the host (table: the values are read back from the device)
int to_pairs(qk_attr_data &d, hipStream_t st, std::vector<int64_t> &ids, std::vector<int64_t> &vals) {
    if (d.layout == QK_ATTR_SORTED) {
        ids = d.h_ids;
        vals = d.h_vals;
        return QK_OK;
    }
    ids.clear();
    vals.clear();
    if (d.max_id < 0) return QK_OK;
    std::vector<int64_t> dense((size_t)d.max_id + 1);
    QK_HIP(hipStreamSynchronize(st));
    QK_HIP(hipMemcpy(dense.data(), d.t_vals, dense.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    ids.reserve((size_t)d.n_ids);
    vals.reserve((size_t)d.n_ids);
    for (int64_t id = 0; id <= d.max_id; id++)
        if (bit_of(d.h_bits, id)) {
            ids.push_back(id);
            vals.push_back(dense[(size_t)id]);
        }
    return QK_OK;
}

// the pairs become the column, in the layout the rule asks for
int load_pairs(qk_attr_data &d, hipStream_t st, std::vector<int64_t> &ids, std::vector<int64_t> &vals) {
    const int64_t n = (int64_t)ids.size();
    const int64_t max_id = n ? ids.back() : -1;
    if (want_table(max_id, n)) {
        free_sorted(d);
        bool grown = false;
        QK_TRY(table_reserve(d, st, max_id + 1, &grown));
        std::fill(d.h_bits.begin(), d.h_bits.end(), 0u);
        for (int64_t id : ids) d.h_bits[(size_t)(id >> 5)] |= 1u << (id & 31);
        QK_TRY(upload_bits(d, st));
        QK_TRY(table_scatter(d, st, ids, vals, {}));
        d.layout = QK_ATTR_TABLE;
    } else {
        free_table(d);
        d.h_ids.swap(ids);
        d.h_vals.swap(vals);
        QK_TRY(upload_sorted(d, st));
        d.layout = QK_ATTR_SORTED;
    }
    d.n_ids = n;
    d.max_id = max_id;
    return QK_OK;
}

// (ids, vals) <- its union with (uids, uvals), both ascending and distinct; the update wins
void merge_pairs(std::vector<int64_t> &ids, std::vector<int64_t> &vals, const std::vector<int64_t> &uids, const std::vector<int64_t> &uvals) {
    std::vector<int64_t> oi, ov;
    oi.reserve(ids.size() + uids.size());
    ov.reserve(ids.size() + uids.size());
    size_t i = 0, j = 0;
    while (i < ids.size() || j < uids.size()) {
        if (j == uids.size() || (i < ids.size() && ids[i] < uids[j])) {
            oi.push_back(ids[i]);
            ov.push_back(vals[i]);
            i++;
        } else {
            if (i < ids.size() && ids[i] == uids[j]) i++;
            oi.push_back(uids[j]);
            ov.push_back(uvals[j]);
            j++;
        }
    }
    ids.swap(oi);
    vals.swap(ov);
}

// (ids, vals) without the ids of `gone` (ascending, distinct)
void remove_pairs(std::vector<int64_t> &ids, std::vector<int64_t> &vals, const std::vector<int64_t> &gone) {
    size_t o = 0, j = 0;
    for (size_t i = 0; i < ids.size(); i++) {
        while (j < gone.size() && gone[j] < ids[i]) j++;
        if (j < gone.size() && gone[j] == ids[i]) continue;
        ids[o] = ids[i];
        vals[o] = vals[i];
        o++;
    }
    ids.resize(o);
    vals.resize(o);
}

int finish_update(qk_attr *a) {
    qk_attr_data &d = *a->d;
    d.version++;
    d.upd_stream = a->ctx->stream;
    d.updated = true;
    QK_HIP(hipEventRecord(d.upd_ev, a->ctx->stream));
    return QK_OK;
}

}  // namespace

bool qk_filter_where_current(const qk_filter *f) {
    for (const qk_filter_clause &c : f->clauses)
        if (c.col->version != c.col_version) return false;
    return true;
}

int qk_launch_filter_build_where(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    hipStream_t st = ctx->stream;
    WhereBuildParams F;
    F.nc = (int)f->clauses.size();
    for (int i = 0; i < F.nc; i++) {
        qk_filter_clause &c = f->clauses[(size_t)i];
        // a column updated on another stream: behind its last update
        if (c.col->updated && c.col->upd_stream != st) QK_HIP(hipStreamWaitEvent(st, c.col->upd_ev, 0));
        F.c[i].col = col_of(*c.col);
        if (!col_usable(F.c[i].col)) QK_FAIL(QK_ERR_HIP, "filtered search: the column of clause %d lost its device data in a failed update", i);
        F.c[i].op = c.op;
        F.c[i].a = c.a;
        F.c[i].b = c.b;
        c.col_version = c.col->version;
    }
    for (int i = F.nc; i < QK_MAX_CLAUSES; i++) F.c[i] = F.c[0];
    const int64_t npids = (int64_t)s->parts.size();
    if (npids > 0 && s->ntotal > 0) {
        F.ids = s->ids;
        F.pt_off = s->d_off;
        F.pt_size = s->d_size;
        F.mask = f->mask;
        F.mask_words = f->mask_words;
        F.allowed = f->d_allowed;
        const int64_t max_tiles = (std::max<int64_t>(1, s->max_size) + 15) / 16;
        const unsigned gy = (unsigned)std::min<int64_t>(65535, (max_tiles + 16 * WB_U - 1) / (16 * WB_U));
        hipLaunchKernelGGL(k_filter_build_where, dim3((unsigned)npids, gy), dim3(256), 0, st, F);
        QK_HIP(hipGetLastError());
    }
    return QK_OK;
}

int qk_launch_filter_build_expr(qk_ctx *ctx, qk_store *s, qk_filter *f) {
    hipStream_t st = ctx->stream;
    ExprBuildParams F;
    const int nc = (int)f->clauses.size();
    F.nt = (int)f->term_end.size();
    for (int t = 0; t < QK_MAX_TERMS; t++) F.term_end[t] = t < F.nt ? f->term_end[(size_t)t] : nc;
    for (int i = 0; i < nc; i++) {
        qk_filter_clause &c = f->clauses[(size_t)i];
        // a column updated on another stream: behind its last update
        if (c.col->updated && c.col->upd_stream != st) QK_HIP(hipStreamWaitEvent(st, c.col->upd_ev, 0));
        F.c[i].col = col_of(*c.col);
        if (!col_usable(F.c[i].col)) QK_FAIL(QK_ERR_HIP, "filtered search: the column of clause %d lost its device data in a failed update", i);
        F.c[i].op = c.op;
        F.c[i].a = c.a;
        F.c[i].b = c.b;
        F.c[i].set = f->d_sets + c.set_off;
        F.c[i].n_set = c.set_n;
        c.col_version = c.col->version;
    }
    for (int i = nc; i < QK_MAX_EXPR_CLAUSES; i++) F.c[i] = F.c[0];
    const int64_t npids = (int64_t)s->parts.size();
    if (npids > 0 && s->ntotal > 0) {
        F.ids = s->ids;
        F.pt_off = s->d_off;
        F.pt_size = s->d_size;
        F.mask = f->mask;
        F.mask_words = f->mask_words;
        F.allowed = f->d_allowed;
        const int64_t max_tiles = (std::max<int64_t>(1, s->max_size) + 15) / 16;
        const unsigned gy = (unsigned)std::min<int64_t>(65535, (max_tiles + 16 * WB_U - 1) / (16 * WB_U));
        hipLaunchKernelGGL(k_filter_build_expr, dim3((unsigned)npids, gy), dim3(256), 0, st, F);
        QK_HIP(hipGetLastError());
    }
    return QK_OK;
}

extern "C" {

int qk_attr_create(qk_store *s, qk_attr **out) {
    if (!s || !out) QK_FAIL(QK_ERR_INVALID, "qk_attr_create: null argument");
    qk_ctx *c = s->ctx;
    QK_HIP(hipSetDevice(c->device));
    static std::atomic<uint64_t> next_serial{1};
    auto d = std::make_shared<qk_attr_data>();
    d->serial = next_serial.fetch_add(1);
    d->store_uid = s->uid;
    d->device = c->device;
    QK_HIP(hipEventCreateWithFlags(&d->upd_ev, hipEventDisableTiming));
    // an empty column is a table (max_id = -1 < 65536) without a bit set
    bool grown = false;
    QK_TRY(table_reserve(*d, c->stream, TABLE_MIN, &grown));
    QK_TRY(upload_bits(*d, c->stream));
    qk_attr *a = new qk_attr();
    a->d = d;
    a->ctx = c;
    const int rc = finish_update(a);
    if (rc != QK_OK) {
        delete a;
        return rc;
    }
    d->version = 0;
    *out = a;
    return QK_OK;
}

int qk_attr_destroy(qk_attr *a) {
    if (!a) return QK_OK;
    delete a;  // (the device data goes with its last owner: filters that name the column keep it)
    return QK_OK;
}

int qk_attr_set(qk_attr *a, const int64_t *ids, const int64_t *values, int64_t n, int mem) {
    if (!a || n < 0 || (n > 0 && (!ids || !values))) QK_FAIL(QK_ERR_INVALID, "qk_attr_set: bad argument");
    qk_attr_data &d = *a->d;
    qk_ctx *c = a->ctx;
    QK_HIP(hipSetDevice(d.device));
    hipStream_t st = c->stream;
    std::vector<int64_t> hi, hv;
    QK_TRY(fetch_i64(c, ids, n, mem, hi));
    QK_TRY(fetch_i64(c, values, n, mem, hv));
    for (int64_t i = 0; i < n; i++)
        if (hi[(size_t)i] < 0) QK_FAIL(QK_ERR_INVALID, "qk_attr_set: ids[%lld] = %lld is negative", (long long)i, (long long)hi[(size_t)i]);
    // the request de-duplicated on the host: ascending ids, of an id given twice the last value
    std::vector<int64_t> order((size_t)n);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return hi[(size_t)x] < hi[(size_t)y]; });
    std::vector<int64_t> uids, uvals;
    uids.reserve((size_t)n);
    uvals.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t o = order[(size_t)i];
        if (!uids.empty() && uids.back() == hi[(size_t)o]) uvals.back() = hv[(size_t)o];
        else {
            uids.push_back(hi[(size_t)o]);
            uvals.push_back(hv[(size_t)o]);
        }
    }
    if (!uids.empty()) {
        int64_t n_new = 0;
        if (d.layout == QK_ATTR_TABLE) {
            for (int64_t id : uids) n_new += bit_of(d.h_bits, id) ? 0 : 1;
        } else {
            size_t j = 0;
            for (int64_t id : uids) {
                while (j < d.h_ids.size() && d.h_ids[j] < id) j++;
                n_new += (j < d.h_ids.size() && d.h_ids[j] == id) ? 0 : 1;
            }
        }
        const int64_t new_n = d.n_ids + n_new, new_max = std::max(d.max_id, uids.back());
        const bool table = want_table(new_max, new_n);
        if (table && d.layout == QK_ATTR_TABLE) {
            bool grown = false;
            QK_TRY(table_reserve(d, st, new_max + 1, &grown));
            std::vector<int64_t> words;
            for (int64_t id : uids) {
                d.h_bits[(size_t)(id >> 5)] |= 1u << (id & 31);
                if (words.empty() || words.back() != (id >> 5)) words.push_back(id >> 5);
            }
            if (grown) {
                QK_TRY(upload_bits(d, st));
                words.clear();
            }
            QK_TRY(table_scatter(d, st, uids, uvals, words));
            d.n_ids = new_n;
            d.max_id = new_max;
        } else if (!table && d.layout == QK_ATTR_SORTED) {
            merge_pairs(d.h_ids, d.h_vals, uids, uvals);
            QK_TRY(upload_sorted(d, st));
            d.n_ids = new_n;
            d.max_id = new_max;
        } else {  // the rule flipped: convert
            std::vector<int64_t> pi, pv;
            QK_TRY(to_pairs(d, st, pi, pv));
            merge_pairs(pi, pv, uids, uvals);
            QK_TRY(load_pairs(d, st, pi, pv));
        }
    }
    return finish_update(a);
}

int qk_attr_unset(qk_attr *a, const int64_t *ids, int64_t n, int mem) {
    if (!a || n < 0 || (n > 0 && !ids)) QK_FAIL(QK_ERR_INVALID, "qk_attr_unset: bad argument");
    qk_attr_data &d = *a->d;
    qk_ctx *c = a->ctx;
    QK_HIP(hipSetDevice(d.device));
    hipStream_t st = c->stream;
    std::vector<int64_t> gone;
    QK_TRY(fetch_i64(c, ids, n, mem, gone));
    std::sort(gone.begin(), gone.end());
    gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
    if (d.layout == QK_ATTR_TABLE) {
        std::vector<int64_t> words;
        int64_t removed = 0;
        for (int64_t id : gone) {
            if (id < 0 || !bit_of(d.h_bits, id)) continue;
            d.h_bits[(size_t)(id >> 5)] &= ~(1u << (id & 31));
            if (words.empty() || words.back() != (id >> 5)) words.push_back(id >> 5);
            removed++;
        }
        d.n_ids -= removed;
        while (d.max_id >= 0 && !bit_of(d.h_bits, d.max_id)) d.max_id--;
        if (want_table(d.max_id, d.n_ids)) {
            QK_TRY(table_scatter(d, st, {}, {}, words));
        } else {  // (the host bits are already those after the unset)
            std::vector<int64_t> pi, pv;
            QK_TRY(to_pairs(d, st, pi, pv));
            QK_TRY(load_pairs(d, st, pi, pv));
        }
    } else {
        remove_pairs(d.h_ids, d.h_vals, gone);
        const int64_t nn = (int64_t)d.h_ids.size();
        const int64_t mx = nn ? d.h_ids.back() : -1;
        if (!want_table(mx, nn)) {
            QK_TRY(upload_sorted(d, st));
            d.n_ids = nn;
            d.max_id = mx;
        } else {
            std::vector<int64_t> pi, pv;
            pi.swap(d.h_ids);
            pv.swap(d.h_vals);
            QK_TRY(load_pairs(d, st, pi, pv));
        }
    }
    return finish_update(a);
}

int qk_attr_get(qk_attr *a, const int64_t *ids_host, int64_t n, int64_t *values_out_host, int *found) {
    if (!a || n < 0 || (n > 0 && !ids_host)) QK_FAIL(QK_ERR_INVALID, "qk_attr_get: bad argument");
    if (n == 0) return QK_OK;
    qk_attr_data &d = *a->d;
    QK_HIP(hipSetDevice(d.device));
    hipStream_t st = a->ctx->stream;
    if (!col_usable(col_of(d))) QK_FAIL(QK_ERR_HIP, "qk_attr_get: the column lost its device data in a failed update");
    int64_t *g_ids = nullptr, *g_vals = nullptr;
    int32_t *g_found = nullptr;
    int rc = dev_alloc(&g_ids, n, "qk_attr_get");
    if (rc == QK_OK) rc = dev_alloc(&g_vals, n, "qk_attr_get");
    if (rc == QK_OK) rc = dev_alloc(&g_found, n, "qk_attr_get");
    std::vector<int64_t> hv((size_t)n);
    std::vector<int32_t> hf((size_t)n);
    auto run = [&]() -> int {
        QK_HIP(hipMemcpyAsync(g_ids, ids_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_attr_get, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, col_of(d), (const int64_t *)g_ids, n, g_vals, g_found);
        QK_HIP(hipGetLastError());
        QK_HIP(hipMemcpyAsync(hv.data(), g_vals, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        QK_HIP(hipMemcpyAsync(hf.data(), g_found, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        QK_HIP(hipStreamSynchronize(st));
        return QK_OK;
    };
    if (rc == QK_OK) rc = run();
    if (g_ids) hipFree(g_ids);
    if (g_vals) hipFree(g_vals);
    if (g_found) hipFree(g_found);
    if (rc != QK_OK) return rc;
    for (int64_t i = 0; i < n; i++) {
        if (values_out_host) values_out_host[i] = hv[(size_t)i];
        if (found) found[i] = (int)hf[(size_t)i];
    }
    return QK_OK;
}

int qk_attr_info(qk_attr *a, int64_t *n_ids, uint64_t *version, int *layout, int64_t *device_bytes) {
    if (!a) QK_FAIL(QK_ERR_INVALID, "qk_attr_info: null column");
    const qk_attr_data &d = *a->d;
    if (n_ids) *n_ids = d.n_ids;
    if (version) *version = d.version;
    if (layout) *layout = d.layout;
    if (device_bytes)
        *device_bytes = (int64_t)((size_t)d.t_cap * sizeof(int64_t) + (size_t)(d.t_cap / 32) * sizeof(uint32_t) +
                                  (size_t)d.s_cap * 2 * sizeof(int64_t) + d.stage_cap);
    return QK_OK;
}

int qk_filter_create_where(qk_store *s, const qk_clause *clauses, int n_clauses, qk_filter **out) {
    if (!s || !out) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_where: null argument");
    if (n_clauses < 1 || !clauses) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_where: at least one clause is required (n_clauses=%d)", n_clauses);
    if (n_clauses > QK_MAX_CLAUSES)
        QK_FAIL(QK_ERR_UNSUPPORTED, "qk_filter_create_where: n_clauses=%d exceeds QK_MAX_CLAUSES=%d", n_clauses, QK_MAX_CLAUSES);
    for (int i = 0; i < n_clauses; i++) {
        const qk_clause &c = clauses[i];
        if (!c.attr) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_where: clause %d names a null column", i);
        if (c.attr->d->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_where: the column of clause %d belongs to another store", i);
        if (c.op < QK_OP_RANGE || c.op > QK_OP_NO_BITS) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_where: clause %d has the unknown op %d", i, c.op);
    }
    qk_ctx *ctx = s->ctx;
    QK_HIP(hipSetDevice(ctx->device));
    qk_filter *f = new qk_filter();
    f->serial = qk_filter_next_serial();
    f->store_uid = s->uid;
    f->device = ctx->device;
    f->kind = QK_FILTER_KIND_WHERE;
    f->n_ids = 0;
    for (int i = 0; i < n_clauses; i++) {
        qk_filter_clause c;
        c.col = clauses[i].attr->d;
        c.op = clauses[i].op;
        c.a = clauses[i].a;
        c.b = clauses[i].b;
        f->clauses.push_back(std::move(c));
    }
    const bool ok = hipMalloc((void **)&f->d_allowed, sizeof(unsigned long long)) == hipSuccess &&
                    hipEventCreateWithFlags(&f->built_ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        qk_filter_destroy(f);
        QK_FAIL(QK_ERR_OOM, "qk_filter_create_where: no device memory");
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

int qk_filter_create_expr(qk_store *s, const qk_expr_clause *clauses, const int *term_sizes, int n_terms, qk_filter **out) {
    if (!s || !out) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: null argument");
    if (n_terms < 1 || !clauses || !term_sizes) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: at least one term is required (n_terms=%d)", n_terms);
    if (n_terms > QK_MAX_TERMS) QK_FAIL(QK_ERR_UNSUPPORTED, "qk_filter_create_expr: n_terms=%d exceeds QK_MAX_TERMS=%d", n_terms, QK_MAX_TERMS);
    int64_t nc = 0;
    for (int t = 0; t < n_terms; t++) {
        if (term_sizes[t] < 1) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: term %d needs at least one clause (term_sizes[%d]=%d)", t, t, term_sizes[t]);
        nc += term_sizes[t];
    }
    if (nc > QK_MAX_EXPR_CLAUSES)
        QK_FAIL(QK_ERR_UNSUPPORTED, "qk_filter_create_expr: %lld clauses in total exceed QK_MAX_EXPR_CLAUSES=%d", (long long)nc, QK_MAX_EXPR_CLAUSES);
    for (int i = 0; i < (int)nc; i++) {
        const qk_expr_clause &c = clauses[i];
        if (!c.attr) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: clause %d names a null column", i);
        if (c.attr->d->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: the column of clause %d belongs to another store", i);
        if (c.op < QK_OP_RANGE || c.op > QK_OP_NOT_IN_SET) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: clause %d has the unknown op %d", i, c.op);
        if (c.op < QK_OP_IN_SET) continue;  // (set / n_set are read by the two set ops only)
        if (c.n_set < 0) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: clause %d has a negative n_set (%lld)", i, (long long)c.n_set);
        if (c.n_set > 0 && !c.set) QK_FAIL(QK_ERR_INVALID, "qk_filter_create_expr: clause %d has n_set=%lld and a null set", i, (long long)c.n_set);
        if (c.n_set > QK_MAX_SET_VALUES)
            QK_FAIL(QK_ERR_UNSUPPORTED, "qk_filter_create_expr: n_set=%lld of clause %d exceeds QK_MAX_SET_VALUES=%d", (long long)c.n_set, i,
                    QK_MAX_SET_VALUES);
    }
    qk_ctx *ctx = s->ctx;
    QK_HIP(hipSetDevice(ctx->device));
    qk_filter *f = new qk_filter();
    f->serial = qk_filter_next_serial();
    f->store_uid = s->uid;
    f->device = ctx->device;
    f->kind = QK_FILTER_KIND_EXPR;
    f->n_ids = 0;
    // the sets sorted and de-duplicated on the host, one after the other in one buffer: every set clause has its own slice, a set
    // given to several clauses is held once per clause (at worst 32 x 2^20 values = 256 MB, on the host here and on the device)
    std::vector<int64_t> sets;
    try {
        int i = 0;
        for (int t = 0; t < n_terms; t++) {
            for (int e = i + term_sizes[t]; i < e; i++) {
                qk_filter_clause c;
                c.col = clauses[i].attr->d;
                c.op = clauses[i].op;
                c.a = clauses[i].a;
                c.b = clauses[i].b;
                if (c.op >= QK_OP_IN_SET && clauses[i].n_set > 0) {
                    std::vector<int64_t> h(clauses[i].set, clauses[i].set + clauses[i].n_set);
                    std::sort(h.begin(), h.end());
                    h.erase(std::unique(h.begin(), h.end()), h.end());
                    c.set_off = (int64_t)sets.size();
                    c.set_n = (int64_t)h.size();
                    sets.insert(sets.end(), h.begin(), h.end());
                }
                f->clauses.push_back(std::move(c));
            }
            f->term_end.push_back(i);
        }
    } catch (const std::bad_alloc &) {  // (no exception crosses the C ABI)
        qk_filter_destroy(f);
        QK_FAIL(QK_ERR_OOM, "qk_filter_create_expr: no host memory for the value sets");
    }
    f->sets_len = (int64_t)sets.size();
    bool ok = hipMalloc((void **)&f->d_sets, std::max<size_t>(sets.size(), 1) * sizeof(int64_t)) == hipSuccess &&
              hipMalloc((void **)&f->d_allowed, sizeof(unsigned long long)) == hipSuccess &&
              hipEventCreateWithFlags(&f->built_ev, hipEventDisableTiming) == hipSuccess;
    if (ok && !sets.empty()) ok = hipMemcpy(f->d_sets, sets.data(), sets.size() * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        qk_filter_destroy(f);
        QK_FAIL(QK_ERR_OOM, "qk_filter_create_expr: no device memory");
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

}  // extern "C"
