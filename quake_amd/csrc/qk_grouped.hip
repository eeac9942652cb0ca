// qk_grouped.hip -- grouped search: the k best GROUPS of an attribute column, every group represented by its best row
// (include/quake_hip.h, "grouped search").
//
// The expensive half is the key-emission scan, run pass by pass by qk_emit_passes (qk_dense.hip): keys[pair_base[pair] + row] holds
// the canonical key of every (query, probed row), pairs in (query, rank) order.  Between emission and the exact selection of the
// wide-k path (qk_launch_select_pairs, qk_dense.hip) the keys of every row that is not the (min key, min id) of its group are
// overwritten with 0xFFFFFFFF -- the key that is never a candidate -- so the selection sees one row per group.  This file's device work:
//   k_grouped_rowvals   once per (store version, column version): the column's value of every arena row and a has-value mask in
//                       the filter's layout (one 16-bit word per 16-row tile); a call that finds both stamps unchanged does nothing
//   per pass of queries, an open-addressing table per query (value, min key, min id), cleared by one memset of 0xFF:
//   k_grouped_claim     every candidate finds or claims the slot of its value (atomicCAS on the value word), remembers the slot
//                       and folds its key into the slot's minimum (atomicMin)
//   k_grouped_minid     every candidate whose key is its slot's minimum folds its id into the slot (64-bit atomicMin)
//   k_grouped_rewrite   every emitted key that is not its slot's (min key, min id) becomes 0xFFFFFFFF
//   k_grouped_values    groups[q][j] of the selected ids, through the column's lookup
// group_size = m > 1 (qk_*_grouped_n; DESIGN.md 5.10, "members"): the rewrite leaves the emitted keys alone and fills a second key
// array for the selection; behind the selection
//   k_grouped_mark      per (query, j): the value of the selected row finds its slot again, the slot learns j, member 0 goes to
//                       [q][j][0] of the strided outputs
//   k_grouped_renumber  every key's slot number becomes the j of its group, or -1 where the group was not selected
//   per member r = 1 .. m - 1, the floor being member r - 1 of the key's group:
//   k_grouped_next_key  the smallest key of the group's candidates above the floor (atomicMin)
//   k_grouped_next_id   the smallest id among those with that key (64-bit atomicMin, straight into out_ids)
//   k_grouped_member_dist  distances of members 1 .. m - 1 from their keys, by the selection's epilogue rule
// No thread waits for another: a slot's key and id words hold "nothing yet" (all ones) from the memset on, so whoever finds a value
// claimed proceeds at once, and the phases are separated by kernel boundaries.  Only commutative minima decide a slot, so the result
// does not depend on who came first.  The value whose bits are all ones (-1) is the table's empty marker: it owns slot T of every query.
// The host side is this file's kernels plus one description: grouped_call states the call for qk_emit_run (qk_emit.hip), the host
// body of every entry point on the emission scan -- no radius, one column -- and grouped_device hangs the launches above into
// qk_emit_device's skeleton.
#include "qk_attr.h"

#include <cstring>
#include "qk_device.h"

namespace {

constexpr unsigned long long GR_EMPTY = ~0ull;
constexpr int GR_SLICE = 1024;  // keys per workgroup step: 256 threads x 4

struct GroupedParams {
    uint32_t *keys;
    int32_t *slot;             // per emitted key: the slot of its value inside its query's table, -1 = no candidate
    const int64_t *pair_base;  // [npairs + 1]
    const int64_t *pids;       // [nq][P] or nullptr (pair r -> list r)
    const int64_t *pt_off;
    const int64_t *ids;        // arena ids
    const uint16_t *mask;      // row mask of a filter, or nullptr
    const uint16_t *has;       // has-value mask of the column
    const int64_t *rowval;     // the column's value per arena row
    unsigned long long *tvals; // [nq][T + 1]
    unsigned long long *tids;  // [nq][T + 1]
    uint32_t *tkeys;           // [nq][T + 1]
    int P, Sg;
    uint32_t tmask;            // T - 1
    // group_size > 1 only
    uint32_t *sel_keys;        // the keys the selection reads: keys with every non-representative set to 0xFFFFFFFF (nullptr: in place)
    int32_t *tsel;             // [nq][T + 1] the j of a selected group, -1 elsewhere
    uint32_t *mkeys;           // [nq][k][m] key of every member, 0xFFFFFFFF = none
    int64_t *mids;             // [nq][k][m] out_ids of the pass
    int k, m, r;               // r: the member a round decides
};

__device__ __forceinline__ uint32_t grouped_hash(unsigned long long v) {  // (the 64-bit finaliser of MurmurHash3)
    v ^= v >> 33;
    v *= 0xff51afd7ed558ccdull;
    v ^= v >> 33;
    v *= 0xc4ceb9fe1a85ec53ull;
    v ^= v >> 33;
    return (uint32_t)v;
}

// blockIdx.x = query * Sg + g: the workgroup takes slices g, g + Sg, ... of its query's segment (the decomposition of k_range_count)
#define GROUPED_FOR_EACH_KEY(G)                                                                          \
    const int64_t q = blockIdx.x / (G).Sg;                                                               \
    const int64_t *pbase = (G).pair_base + q * (G).P;                                                    \
    const int64_t *qpids = (G).pids ? (G).pids + q * (G).P : nullptr;                                    \
    const int64_t beg = pbase[0], end = pbase[(G).P];                                                    \
    const int64_t tbase = q * ((int64_t)(G).tmask + 2);                                                  \
    for (int64_t s0 = beg + (int64_t)(blockIdx.x - q * (G).Sg) * GR_SLICE; s0 < end; s0 += (int64_t)(G).Sg * GR_SLICE) \
        for (int64_t pos = s0 + threadIdx.x; pos < min(end, s0 + GR_SLICE); pos += 256)

__global__ __launch_bounds__(256) void k_grouped_claim(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const uint32_t key = G.keys[pos];
        int32_t sl = -1;
        if (key != 0xFFFFFFFFu) {
            const int64_t row = emit_key_row(pbase, qpids, G.P, G.pt_off, pos);
            bool ok = (G.has[row >> 4] >> (row & 15)) & 1;
            if (ok && G.mask) ok = (G.mask[row >> 4] >> (row & 15)) & 1;
            if (ok) {
                const unsigned long long v = (unsigned long long)G.rowval[row];
                if (v == GR_EMPTY) {
                    sl = (int32_t)G.tmask + 1;  // the value that looks like an empty slot has a slot of its own
                } else {
                    // linear probing; the table holds at least twice the values a query can meet, so an empty slot ends every chain.
                    // At most T probes whatever happens: this loop cannot spin.
                    uint32_t h = grouped_hash(v) & G.tmask;
                    for (uint32_t n = 0; n <= G.tmask; n++) {
                        unsigned long long cur = __hip_atomic_load(&G.tvals[tbase + h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (cur == GR_EMPTY) {
                            cur = atomicCAS(&G.tvals[tbase + h], GR_EMPTY, v);
                            if (cur == GR_EMPTY) cur = v;
                        }
                        if (cur == v) {
                            sl = (int32_t)h;
                            break;
                        }
                        h = (h + 1) & G.tmask;
                    }
                }
                if (sl >= 0) atomicMin(&G.tkeys[tbase + sl], key);
            }
        }
        G.slot[pos] = sl;
    }
}

__global__ __launch_bounds__(256) void k_grouped_minid(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const int32_t sl = G.slot[pos];
        if (sl < 0) continue;
        if (G.keys[pos] != G.tkeys[tbase + sl]) continue;
        const int64_t row = emit_key_row(pbase, qpids, G.P, G.pt_off, pos);
        atomicMin(&G.tids[tbase + sl], (unsigned long long)G.ids[row]);  // (attribute ids are non-negative)
    }
}

__global__ __launch_bounds__(256) void k_grouped_rewrite(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const int32_t sl = G.slot[pos];
        const uint32_t key = G.keys[pos];
        bool win = false;
        if (sl >= 0 && key == G.tkeys[tbase + sl]) {
            const int64_t row = emit_key_row(pbase, qpids, G.P, G.pt_off, pos);
            win = (unsigned long long)G.ids[row] == G.tids[tbase + sl];
        }
        if (G.sel_keys) G.sel_keys[pos] = win ? key : 0xFFFFFFFFu;
        else if (!win && key != 0xFFFFFFFFu) G.keys[pos] = 0xFFFFFFFFu;
    }
}

// ---- group_size > 1: members 1 .. m - 1 of the k selected groups ------------------------------------------------------------------
struct MarkParams {
    AttrCol col;
    const int64_t *sel_ids;             // [nq][k] the selection's result
    const float *sel_dist;              // [nq][k] or nullptr
    const unsigned long long *tvals;    // [nq][T + 1]
    const uint32_t *tkeys;              // [nq][T + 1]
    int32_t *tsel;                      // [nq][T + 1], cleared to -1
    uint32_t *mkeys;                    // [nq][k][m], cleared to 0xFFFFFFFF
    int64_t *out_ids;                   // [nq][k][m], cleared to -1
    float *out_dist;                    // [nq][k][m] or nullptr
    int64_t *out_groups;                // [nq][k] or nullptr
    int64_t n;                          // nq * k
    int k, m;
    uint32_t tmask;
};

// one thread per (query, j).  The slot of the selected row's value is found the way k_grouped_claim found it -- same hash, same
// bounded walk, read only: the value is in the table because its row claimed it.
__global__ __launch_bounds__(256) void k_grouped_mark(MarkParams M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t raw = i < M.n ? M.sel_ids[i] : -1;
    const bool live[1] = {raw >= 0};
    const int64_t id[1] = {live[0] ? raw : 0};
    int64_t v[1];
    bool has[1];
    attr_lookup<1>(M.col, id, live, v, has);
    if (i >= M.n) return;
    const int64_t q = i / M.k;
    const int j = (int)(i - q * M.k);
    const int64_t tbase = q * ((int64_t)M.tmask + 2);
    if (M.out_groups) M.out_groups[i] = has[0] ? v[0] : 0;
    if (M.out_dist) M.out_dist[i * M.m] = M.sel_dist[i];
    if (!has[0]) return;  // padding: every member keeps the cleared words
    const unsigned long long val = (unsigned long long)v[0];
    int32_t sl = -1;
    if (val == GR_EMPTY) {
        sl = (int32_t)M.tmask + 1;
    } else {
        uint32_t h = grouped_hash(val) & M.tmask;
        for (uint32_t n = 0; n <= M.tmask; n++) {
            const unsigned long long cur = M.tvals[tbase + h];
            if (cur == val) {
                sl = (int32_t)h;
                break;
            }
            if (cur == GR_EMPTY) break;
            h = (h + 1) & M.tmask;
        }
    }
    M.out_ids[i * M.m] = raw;
    if (sl >= 0) {
        M.tsel[tbase + sl] = j;
        M.mkeys[i * M.m] = M.tkeys[tbase + sl];
    }
}

// slot[pos]: the slot of the key's value -> the j of its group among the k selected, -1 for every other key.  The rounds below then
// drop a key of a group that was not selected after one load.
__global__ __launch_bounds__(256) void k_grouped_renumber(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const int32_t sl = G.slot[pos];
        if (sl >= 0) G.slot[pos] = G.tsel[tbase + sl];
    }
}

// a key of group j qualifies for member r when its (key, id) lies strictly above member r - 1's: the smallest such key
__global__ __launch_bounds__(256) void k_grouped_next_key(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const int32_t j = G.slot[pos];
        if (j < 0) continue;
        const int64_t w = ((q * G.k + j) * G.m) + G.r;
        const uint32_t fkey = G.mkeys[w - 1];
        if (fkey == 0xFFFFFFFFu) continue;  // the group ran out of rows in an earlier round
        const uint32_t key = G.keys[pos];
        if (key < fkey) continue;
        if (key == fkey) {
            const int64_t row = emit_key_row(pbase, qpids, G.P, G.pt_off, pos);
            if ((unsigned long long)G.ids[row] <= (unsigned long long)G.mids[w - 1]) continue;
        }
        atomicMin(&G.mkeys[w], key);
    }
}

// ... and the smallest id among the qualifying keys that equal it
__global__ __launch_bounds__(256) void k_grouped_next_id(GroupedParams G) {
    GROUPED_FOR_EACH_KEY(G) {
        const int32_t j = G.slot[pos];
        if (j < 0) continue;
        const int64_t w = ((q * G.k + j) * G.m) + G.r;
        const uint32_t key = G.keys[pos];
        if (key != G.mkeys[w]) continue;
        const int64_t row = emit_key_row(pbase, qpids, G.P, G.pt_off, pos);
        const unsigned long long id = (unsigned long long)G.ids[row];
        if (key == G.mkeys[w - 1] && id <= (unsigned long long)G.mids[w - 1]) continue;
        atomicMin((unsigned long long *)&G.mids[w], id);
    }
}

// distances of members 1 .. m - 1 (the epilogue rule of k_select_pairs_large); member 0 carries the selection's own bits
__global__ __launch_bounds__(256) void k_grouped_member_dist(const uint32_t *mkeys, int64_t n, int m, int metric, int sqrt_l2, float *out_dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || i % m == 0) return;
    const uint32_t o = mkeys[i];
    float od = metric == QK_METRIC_IP ? -INFINITY : INFINITY;
    if (o != 0xFFFFFFFFu) {
        if (metric == QK_METRIC_L2) {
            const float d2 = __uint_as_float(o);
            od = sqrt_l2 ? sqrtf(d2) : d2;
        } else {
            od = ip_from_ord(o);
        }
    }
    out_dist[i] = od;
}

// the value of every selected id; the padding id (negative) and -- it cannot happen -- an id without a value give 0
__global__ __launch_bounds__(256) void k_grouped_values(AttrCol c, const int64_t *out_ids, int64_t n, int64_t *groups) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t raw = i < n ? out_ids[i] : -1;
    const bool live[1] = {raw >= 0};
    const int64_t id[1] = {live[0] ? raw : 0};
    int64_t v[1];
    bool has[1];
    attr_lookup<1>(c, id, live, v, has);
    if (i < n) groups[i] = has[0] ? v[0] : 0;
}

// an all-padding result (no list to scan)
__global__ __launch_bounds__(256) void k_grouped_pad(int64_t n, float worst, int64_t *out_ids, float *out_dist, int64_t *groups) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out_ids[i] = -1;
    if (out_dist) out_dist[i] = worst;
    if (groups) groups[i] = 0;
}

// ---- the column's value of every arena row ------------------------------------------------------------------------------------
struct RowvalParams {
    const int64_t *ids;      // arena ids
    const int64_t *pt_off;   // [npids] first arena row of every list
    const int32_t *pt_size;  // [npids] rows, -1 = absent
    AttrCol col;
    int64_t *vals;           // [cap_rows]
    uint16_t *has;           // [has_words]
    int64_t cap_rows, has_words;
};

constexpr int RV_U = 4;  // rows in flight per lane (k_filter_build_where's choice)

// k_filter_build_where's grid and writer rule: blockIdx.x = list, blockIdx.y strides over its chunks of RV_U x 16 tiles; the word of
// a tile is the ballot of the 16 lanes that looked at its rows, stored by the first of them; rows behind a list's size keep 0
__global__ __launch_bounds__(256) void k_grouped_rowvals(RowvalParams R) {
    const int p = blockIdx.x;
    const int size = R.pt_size[p];
    if (size <= 0) return;
    const int64_t row_off = R.pt_off[p];
    const int ntl = (size + 15) >> 4;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int sub = threadIdx.x >> 4;  // tile of a 16-tile chunk
    for (int t0 = blockIdx.y * 16 * RV_U; t0 < ntl; t0 += gridDim.y * 16 * RV_U) {
        int64_t id[RV_U], v[RV_U];
        bool ok[RV_U], has[RV_U];
#pragma unroll
        for (int u = 0; u < RV_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const int row = tile * 16 + j;
            ok[u] = tile < ntl && row < size && row_off + row < R.cap_rows;
            id[u] = R.ids[row_off + (ok[u] ? row : 0)];
        }
        attr_lookup<RV_U>(R.col, id, ok, v, has);
#pragma unroll
        for (int u = 0; u < RV_U; u++) {
            const int tile = t0 + u * 16 + sub;
            const int row = tile * 16 + j;
            if (ok[u]) R.vals[row_off + row] = has[u] ? v[u] : 0;
            const uint64_t b = __ballot(ok[u] && has[u]);
            const uint32_t word = (uint32_t)((b >> (16 * (lane >> 4))) & 0xFFFFull);
            const int64_t w = (row_off >> 4) + tile;
            if (j == 0 && tile < ntl && w < R.has_words) R.has[w] = (uint16_t)word;
        }
    }
}

}  // namespace

// rv_vals / rv_has of the column brought up to date for the store as it is (the table has been synced) on ctx's stream
// (shared with qk_facet.hip: declared in qk_attr.h)
int qk_rowvals_ensure(qk_ctx *ctx, qk_store *s, qk_attr_data &d) {
    hipStream_t st = ctx->stream;
    const bool current = d.rv_built && d.rv_store_version == s->version && d.rv_cap_rows == s->cap_rows && d.rv_col_version == d.version;
    if (current) {
        if (d.rv_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, d.rv_ev, 0));  // derived on another context's stream
        return QK_OK;
    }
    const AttrCol col = col_of(d);
    if (!col_usable(col)) QK_FAIL(QK_ERR_HIP, "grouped search: the column lost its device data in a failed update");
    if (!d.rv_ev) QK_HIP(hipEventCreateWithFlags(&d.rv_ev, hipEventDisableTiming));
    const int64_t rows = std::max<int64_t>(16, qk_round_up64(s->cap_rows, 16));
    if (rows > d.rv_cap || !d.rv_vals) {
        // (hipFree waits for the device: nothing still reads the old arrays)
        if (d.rv_vals) hipFree(d.rv_vals);
        if (d.rv_has) hipFree(d.rv_has);
        d.rv_vals = nullptr;
        d.rv_has = nullptr;
        d.rv_cap = 0;
        d.rv_built = false;
        if (hipMalloc((void **)&d.rv_vals, (size_t)rows * 8) != hipSuccess || hipMalloc((void **)&d.rv_has, (size_t)(rows / 16) * 2) != hipSuccess) {
            (void)hipGetLastError();
            if (d.rv_vals) hipFree(d.rv_vals);
            d.rv_vals = nullptr;
            d.rv_has = nullptr;
            QK_FAIL(QK_ERR_OOM, "grouped search: no device memory for the values of %lld rows", (long long)rows);
        }
        d.rv_cap = rows;
    }
    // behind the column's last update and behind the readers of the previous derivation
    if (d.updated && d.upd_stream != st) QK_HIP(hipStreamWaitEvent(st, d.upd_ev, 0));
    if (d.rv_built && d.rv_ctx != ctx) QK_HIP(hipStreamWaitEvent(st, d.rv_ev, 0));
    const int64_t has_words = d.rv_cap / 16;
    QK_HIP(hipMemsetAsync(d.rv_has, 0, (size_t)has_words * 2, st));
    const int64_t npids = (int64_t)s->parts.size();
    if (npids > 0 && s->ntotal > 0) {
        RowvalParams R;
        R.ids = s->ids;
        R.pt_off = s->d_off;
        R.pt_size = s->d_size;
        R.col = col;
        R.vals = d.rv_vals;
        R.has = d.rv_has;
        R.cap_rows = std::min(s->cap_rows, d.rv_cap);
        R.has_words = has_words;
        const int64_t max_tiles = (std::max<int64_t>(1, s->max_size) + 15) / 16;
        const unsigned gy = (unsigned)std::min<int64_t>(65535, (max_tiles + 16 * RV_U - 1) / (16 * RV_U));
        hipLaunchKernelGGL(k_grouped_rowvals, dim3((unsigned)npids, gy), dim3(256), 0, st, R);
        QK_HIP(hipGetLastError());
    }
    QK_HIP(hipEventRecord(d.rv_ev, st));
    d.rv_built = true;
    d.rv_ctx = ctx;
    d.rv_store_version = s->version;
    d.rv_cap_rows = s->cap_rows;
    d.rv_col_version = d.version;
    d.rv_builds++;
    return QK_OK;
}

// slots of a query's table: a power of two, at least twice the distinct values a query can meet -- no more than the keys it can
// have, no more than the ids that have a value
int64_t qk_grouped_table_slots(int64_t per_query_ub, int64_t n_ids) {
    const int64_t distinct = std::max<int64_t>(1, std::min(per_query_ub, n_ids));
    int64_t T = 16;
    while (T < 2 * distinct) T <<= 1;
    return T;
}

// bytes of a pass that one query accounts for (include/quake_hip.h, QK_GROUPED_PASS_BYTES): 8 per key it has room for -- the key and
// its slot number -- and 20 per table slot; with group_size = m > 1, 12 per key (the selection's copy), 24 per slot (the j of a
// selected group), 12 per result of the one-row selection and 4 per member word
static inline int64_t grouped_query_bytes(int64_t per_query_ub, int64_t T, int k, int m) {
    if (m == 1) return per_query_ub * 8 + (T + 1) * 20;
    return per_query_ub * 12 + (T + 1) * 24 + (int64_t)k * 12 + (int64_t)k * m * 4;
}

namespace {

// the device half: the k best groups of `col` per query over the probed lists, m rows of each; a.k, a.out_ids [Q][k][m] and
// a.out_dist (or nullptr) set, out_groups [Q][k] or nullptr, all on the device; m == 1 is the one-row call, launch for launch
int grouped_device(const qk_emit_call &c, qk_emit_env &e, qk_attr_data &col, int m, int64_t *out_groups) {
    qk_ctx *ctx = c.ctx;
    qk_store *s = c.s;
    const qk_scan_args &a = e.a;
    const uint16_t *mask = e.mask;
    const int64_t Q = a.Q;
    const int k = a.k;
    hipStream_t st = ctx->stream;
    const int P = e.P;
    qk_emit_stages g;
    g.pad = [&]() -> int {
        const int64_t nw = Q * k * m;  // (m > 1: the groups, [Q][k], are cleared apart)
        hipLaunchKernelGGL(k_grouped_pad, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, nw,
                           a.metric == QK_METRIC_IP ? -INFINITY : INFINITY, a.out_ids, a.out_dist, m == 1 ? out_groups : nullptr);
        QK_HIP(hipGetLastError());
        if (m > 1 && out_groups) QK_HIP(hipMemsetAsync(out_groups, 0, (size_t)Q * k * 8, st));
        return QK_OK;
    };
    int kp = 2;  // (k_select_pairs_large keeps kp keys and kp ids in LDS, the ids behind the keys: kp >= 2 keeps them 8-byte aligned)
    while (kp < k) kp <<= 1;
    // this pipeline's bytes of the call's buffer, sized for the largest pass: [slots] [table values] [table ids] [table keys], and
    // for m > 1 [selected j per slot] [the selection's keys] [the selection's ids] [its distances] [member keys]
    int64_t T = 0, S = 0;
    size_t o_tvals = 0, o_tids = 0, o_tkeys = 0, o_tsel = 0, o_skeys = 0, o_sids = 0, o_sdist = 0, o_mkeys = 0;
    g.h.plan = [&](int64_t per_query_ub, int64_t *qc, size_t *extra_bytes) -> int {
        T = qk_grouped_table_slots(per_query_ub, col.n_ids);
        const int64_t qbytes = grouped_query_bytes(per_query_ub, T, k, m);
        if (qbytes > QK_GROUPED_PASS_BYTES)
            QK_FAIL(QK_ERR_UNSUPPORTED, "grouped search: one query needs %lld bytes of workspace, more than QK_GROUPED_PASS_BYTES", (long long)qbytes);
        *qc = std::max<int64_t>(1, std::min<int64_t>(*qc, QK_GROUPED_PASS_BYTES / qbytes));
        S = (per_query_ub + GR_SLICE - 1) / GR_SLICE;
        if (*qc * S > 0x7FFFFFF0LL) QK_FAIL(QK_ERR_UNSUPPORTED, "grouped search: Q too large");
        const int64_t nslots = *qc * (T + 1);
        o_tvals = qk_al256((size_t)*qc * per_query_ub * 4 + 256);
        o_tids = o_tvals + (size_t)nslots * 8;
        o_tkeys = o_tids + (size_t)nslots * 8;
        *extra_bytes = o_tkeys + (size_t)nslots * 4;
        if (m > 1) {
            o_tsel = qk_al256(*extra_bytes);
            o_skeys = qk_al256(o_tsel + (size_t)nslots * 4);
            o_sids = qk_al256(o_skeys + (size_t)*qc * per_query_ub * 4 + 256);
            o_sdist = qk_al256(o_sids + (size_t)*qc * k * 8);
            o_mkeys = qk_al256(o_sdist + (size_t)*qc * k * 4);
            *extra_bytes = o_mkeys + (size_t)*qc * k * m * 4;
        }
        return QK_OK;
    };
    g.h.before_scan = [&](const qk_emit_pass &p) -> int {
        // every slot of the pass: value = empty, min key = min id = "nothing yet"
        QK_HIP(hipMemsetAsync(p.extra + o_tvals, 0xFF, (size_t)p.nq * (T + 1) * 8, st));
        QK_HIP(hipMemsetAsync(p.extra + o_tids, 0xFF, (size_t)p.nq * (T + 1) * 8, st));
        QK_HIP(hipMemsetAsync(p.extra + o_tkeys, 0xFF, (size_t)p.nq * (T + 1) * 4, st));
        return QK_OK;
    };
    g.h.consume = [&](const qk_emit_pass &p) -> int {
        GroupedParams G;
        G.keys = p.keys;
        G.slot = (int32_t *)p.extra;
        G.pair_base = p.pair_base;
        G.pids = p.pids;
        G.pt_off = s->d_off;
        G.ids = s->ids;
        G.mask = mask;
        G.has = col.rv_has;
        G.rowval = col.rv_vals;
        G.tvals = (unsigned long long *)(p.extra + o_tvals);
        G.tids = (unsigned long long *)(p.extra + o_tids);
        G.tkeys = (uint32_t *)(p.extra + o_tkeys);
        G.P = P;
        G.tmask = (uint32_t)(T - 1);
        G.sel_keys = m > 1 ? (uint32_t *)(p.extra + o_skeys) : nullptr;
        G.tsel = (int32_t *)(p.extra + o_tsel);
        G.mkeys = (uint32_t *)(p.extra + o_mkeys);
        G.mids = a.out_ids + p.q0 * k * m;
        G.k = k;
        G.m = m;
        G.r = 0;
        G.Sg = qk_emit_sg(S, p.nq);
        const unsigned grid = (unsigned)(p.nq * G.Sg);
        hipLaunchKernelGGL(k_grouped_claim, dim3(grid), dim3(256), 0, st, G);
        hipLaunchKernelGGL(k_grouped_minid, dim3(grid), dim3(256), 0, st, G);
        hipLaunchKernelGGL(k_grouped_rewrite, dim3(grid), dim3(256), 0, st, G);
        QK_HIP(hipGetLastError());
        if (m == 1)
            return qk_launch_select_pairs(ctx, s, p.keys, p.pair_base, p.pids, p.nq, P, k, kp, a.metric, a.sqrt_l2, a.out_ids + p.q0 * k,
                                          a.out_dist ? a.out_dist + p.q0 * k : nullptr);
        // ---- members: the one-row selection into the workspace, then member 0 into place and a round per further member ----------
        int64_t *sids = (int64_t *)(p.extra + o_sids);
        float *sdist = a.out_dist ? (float *)(p.extra + o_sdist) : nullptr;
        QK_TRY(qk_launch_select_pairs(ctx, s, G.sel_keys, p.pair_base, p.pids, p.nq, P, k, kp, a.metric, a.sqrt_l2, sids, sdist));
        const int64_t nw = p.nq * k * m;  // member words of the pass
        float *mdist = a.out_dist ? a.out_dist + p.q0 * k * m : nullptr;
        QK_HIP(hipMemsetAsync(G.tsel, 0xFF, (size_t)p.nq * (T + 1) * 4, st));
        QK_HIP(hipMemsetAsync(G.mkeys, 0xFF, (size_t)nw * 4, st));
        QK_HIP(hipMemsetAsync(G.mids, 0xFF, (size_t)nw * 8, st));
        MarkParams M;
        M.col = col_of(col);
        M.sel_ids = sids;
        M.sel_dist = sdist;
        M.tvals = G.tvals;
        M.tkeys = G.tkeys;
        M.tsel = G.tsel;
        M.mkeys = G.mkeys;
        M.out_ids = G.mids;
        M.out_dist = mdist;
        M.out_groups = out_groups ? out_groups + p.q0 * k : nullptr;
        M.n = p.nq * k;
        M.k = k;
        M.m = m;
        M.tmask = G.tmask;
        hipLaunchKernelGGL(k_grouped_mark, dim3((unsigned)((M.n + 255) / 256)), dim3(256), 0, st, M);
        hipLaunchKernelGGL(k_grouped_renumber, dim3(grid), dim3(256), 0, st, G);
        for (G.r = 1; G.r < m; G.r++) {
            hipLaunchKernelGGL(k_grouped_next_key, dim3(grid), dim3(256), 0, st, G);
            hipLaunchKernelGGL(k_grouped_next_id, dim3(grid), dim3(256), 0, st, G);
        }
        if (mdist)
            hipLaunchKernelGGL(k_grouped_member_dist, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, (const uint32_t *)G.mkeys, nw, m,
                               a.metric, a.sqrt_l2 ? 1 : 0, mdist);
        QK_HIP(hipGetLastError());
        return QK_OK;
    };
    g.tail = [&]() -> int {
        if (out_groups && m == 1) {
            hipLaunchKernelGGL(k_grouped_values, dim3((unsigned)((Q * k + 255) / 256)), dim3(256), 0, st, col_of(col),
                               (const int64_t *)a.out_ids, Q * k, out_groups);
            QK_HIP(hipGetLastError());
        }
        return QK_OK;
    };
    return qk_emit_device(c, e, g);
}

// both entry points behind their first two checks: the description of the call for qk_emit_run (qk_emit.hip)
int grouped_call(const char *who, qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int nprobe,
                 int k, int m, int metric, qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem,
                 qk_timing *timing) {
    // [ids] [groups] [distances]
    qk_emit_out outs[3] = {{out_ids, (size_t)Q * k * m * 8, true}, {out_groups, (size_t)Q * k * 8, false}, {out_dist, (size_t)Q * k * m * 4, false}};
    qk_emit_call c;
    c.who = who;
    c.pipeline = "grouped search";
    c.label = "k_scan (grouped)";
    c.label_wide = "k_scan_wide (grouped)";
    c.ctx = ctx, c.parent = parent, c.s = s, c.x = x, c.Q = Q, c.pids = pids, c.P = P, c.nprobe = nprobe, c.metric = metric, c.mem = mem;
    c.has_radius = false, c.filter = filter, c.timing = timing;
    c.outs = outs, c.n_outs = 3;
    c.check = [&]() -> int {
        if (!group_by) QK_FAIL(QK_ERR_INVALID, "%s: the group-by column is null", who);
        c.cols[0] = group_by->d.get();
        c.n_cols = 1;
        if (c.cols[0]->store_uid != s->uid) QK_FAIL(QK_ERR_INVALID, "%s: the group-by column belongs to another store", who);
        if (k < 1) QK_FAIL(QK_ERR_INVALID, "%s: k=%d must be at least 1", who, k);
        if (k > QK_MAX_WIDE_K) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: k=%d exceeds %d", who, k, QK_MAX_WIDE_K);
        if (m < 1) QK_FAIL(QK_ERR_INVALID, "%s: group_size=%d must be at least 1", who, m);
        if (m > QK_MAX_GROUP_SIZE) QK_FAIL(QK_ERR_UNSUPPORTED, "%s: group_size=%d exceeds QK_MAX_GROUP_SIZE=%d", who, m, QK_MAX_GROUP_SIZE);
        return QK_OK;
    };
    c.device = [&](qk_emit_env &e) -> int {
        e.a.k = k;
        e.a.out_ids = (int64_t *)outs[0].dev;
        e.a.out_dist = (float *)outs[2].dev;
        return grouped_device(c, e, *c.cols[0], m, (int64_t *)outs[1].dev);
    };
    return qk_emit_run(c);
}

}  // namespace

extern "C" {

int qk_search_grouped_n(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int group_size, int metric,
                        qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_search_grouped: null argument");
    if (parent && nprobe <= 0) QK_FAIL(QK_ERR_INVALID, "qk_search_grouped: nprobe must be positive");
    return grouped_call("qk_search_grouped", ctx, parent, s, x, Q, nullptr, 0, nprobe, k, group_size, metric, group_by, filter, out_ids, out_dist,
                        out_groups, mem, timing);
}

int qk_scan_grouped_n(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int group_size, int metric,
                      qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem, qk_timing *timing) {
    if (!ctx || !s) QK_FAIL(QK_ERR_INVALID, "qk_scan_grouped: null argument");
    if (P <= 0 || (Q > 0 && !pids)) QK_FAIL(QK_ERR_INVALID, "qk_scan_grouped: bad partition id list");
    return grouped_call("qk_scan_grouped", ctx, nullptr, s, x, Q, pids, P, 0, k, group_size, metric, group_by, filter, out_ids, out_dist,
                        out_groups, mem, timing);
}

int qk_search_grouped(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric, qk_attr *group_by,
                      qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem, qk_timing *timing) {
    return qk_search_grouped_n(ctx, parent, s, x, Q, nprobe, k, 1, metric, group_by, filter, out_ids, out_dist, out_groups, mem, timing);
}

int qk_scan_grouped(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric, qk_attr *group_by,
                    qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem, qk_timing *timing) {
    return qk_scan_grouped_n(ctx, s, x, Q, pids, P, k, 1, metric, group_by, filter, out_ids, out_dist, out_groups, mem, timing);
}

int qk_attr_group_info(qk_attr *a, int64_t *builds, int64_t *device_bytes) {
    if (!a) QK_FAIL(QK_ERR_INVALID, "qk_attr_group_info: null column");
    const qk_attr_data &d = *a->d;
    if (builds) *builds = d.rv_builds;
    if (device_bytes) *device_bytes = d.rv_vals ? d.rv_cap * 8 + d.rv_cap / 16 * 2 : 0;
    return QK_OK;
}

}  // extern "C"
