// qk_scan_body.inc -- the body of k_scan (qk_scan.hip), included once per kernel: QK_SCAN_FILT 0 = k_scan as it always was (the
// preprocessed text is the one the kernel had before the filtered sibling existed, so its code does not move), QK_SCAN_FILT 1 =
// k_scan_filt.  The filtered body reads ScanParams::mask -- one 16-bit word per 16-row arena tile, bit r = "row r of the tile is a
// candidate" (qk_filter.hip): a wave walks only the tiles of its share whose word is not 0 -- the loads of the others are never
// issued -- and a row passes the epilogue only with its bit set.  Which tiles are skipped depends on the tile index alone, and the
// barriers of the multi-wave forms sit at the query staging, once per segment, outside the tile loop: every wave reaches them.
// QK_SCAN_FILT 2 = k_scan_filtq, one filter per QUERY: ScanParams::mask is the OR of the call's F masks and drives the walk alone
// (which tiles are read); the word that reaches the epilogue is the lane's own, qmasks[qfilter[myq]][tile] -- lane (j, g) holds
// rows 4g..4g+3 of the tile for query j, so the 16 queries of a tile are answered under 16 different filters in one pass.  The
// four g groups of a query read the same word: at most 16 distinct 2-byte addresses per tile.
// QK_SCAN_AFTER (with QK_SCAN_FILT 1) = k_scan_after, paged search: the filtered body plus one more test in the epilogue -- the
// row's (key, id) must lie behind the lane's own query's cursor (ScanParams::after_key / after_id).  Everything it adds sits
// behind #ifdef QK_SCAN_AFTER: the preprocessed text of the three kernels above does not change.
// QK_SCAN_SHADOW (with QK_SCAN_FILT 0) = k_scan_shadow (qk_shadow.hip), the fp16 shadow form: P.vecs is the fp16 mirror of the arena
// (P.nblk blocks of 32 columns per tile, 16 B per lane as before), P.xq4 the fp16 copy of the queries in the same lane order, one
// v_mfma_f32_16x16x32_f16 per block; no ids are loaded -- a candidate's "id" is its arena row --, the start bound is the seed's
// widened by the query's error bound P.sh_E, P.k is the k' of the form.  Everything it changes sits behind #ifdef QK_SCAN_SHADOW.
// Expects: template parameters DB, MAXCH, MODE, L2 and the kernel argument `ScanParams P` in scope.
    extern __shared__ __align__(16) unsigned char smem[];
    // nw waves per workgroup (1, 2 or 4) share ONE LDS query tile and split every segment's tiles between them; each
    // wave keeps its own pools and emits its own records.  nw > 1 is chosen by the host for wide rows, where a
    // wave-private query tile (1 KiB per 16 columns) would leave room for only 2-3 waves per CU.
    const int lane = threadIdx.x & 63;
    // P.pack > 1: the hardware workgroup is a bundle of `pack` INDEPENDENT one-wave workgroups of the cut (own query tile, own
    // pools, own range; no barrier anywhere on that path).  The dispatcher spreads the waves of one workgroup over the SIMDs
    // of a CU, which it does not do for single-wave workgroups: QK_SCAN_WAVE_CLOCK showed 57 SIMDs holding two of the 1024
    // waves (and 57 none) on some launches, and those 114 waves set the kernel time (0.26 -> 0.31 ms).
    const int wv_phys = threadIdx.x >> 6;
    const int pack = P.pack;
    const int wv = pack > 1 ? 0 : wv_phys, nw = pack > 1 ? 1 : (int)(blockDim.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int nblk = P.nblk, C = P.C, k = P.k;
    constexpr bool l2 = L2;
    constexpr bool qshare = MODE == 3;
    constexpr bool PRODUCT = MODE == 0 || MODE == 3;
    constexpr bool EMIT = MODE == 4;  // wide-k path: keys out, selection happens in k_select_rows_large afterwards
    const size_t per_wave = (size_t)nblk * 1024 + (size_t)16 * C * 12;  // qshare: every wave owns a query tile + pools
    unsigned char *smem_w = smem + (pack > 1 ? (size_t)wv_phys * P.pack_lds : 0);
    float4 *qs = (float4 *)(smem_w + (qshare ? wv * per_wave : 0));           // [nblk*64] (shared by the workgroup unless qshare)
    unsigned char *pool_base = qshare ? smem_w + wv * per_wave + (size_t)nblk * 1024
                                      : smem_w + (size_t)nblk * 1024 + (size_t)wv * 16 * C * 12;
    int64_t *pool_id = (int64_t *)pool_base;                                   // [16][C]
    uint32_t *pool_ord = (uint32_t *)(pool_base + (size_t)16 * C * 8);         // [16][C]
    uint32_t *my_ord = pool_ord + j * C;
    int64_t *my_id = pool_id + j * C;
    const int ncd = nblk / DB;  // d-chunks per tile

    // ---- this wave's contiguous share of the global tile sequence ------------------------------------------
    const long long T = *P.n_tiles;
    const long long W = pack > 1 ? (long long)gridDim.x * pack : (long long)gridDim.x;
    const long long vblock = pack > 1 ? (long long)blockIdx.x * pack + wv_phys : (long long)blockIdx.x;
    const bool dyn = P.dyn_counter != nullptr && nw == 1;
    // static share: an equal cut of the first Ts tiles; the rest is claimed chunk by chunk by whoever finishes first
    // (waves do not finish together: HBM channel and XCD placement make equal tile counts take unequal time)
    const long long Ts = dyn ? T - (T * P.dyn_pct) / 100 : T;
    long long T0 = (Ts * vblock) / W, T1 = (Ts * (vblock + 1)) / W;
    if (P.xcd_on && !dyn) {
        // weighted cut: the split points are f(a) = T a / total for cumulative weights a; a wave's end is its successor's start
        const int np = pack > 1 ? pack : 1;
        long long pre[9];
        pre[0] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) pre[i + 1] = pre[i] + P.xcd_w[i];
        const long long u = blockIdx.x, gu = gridDim.x;
        const long long total = ((gu >> 3) * pre[8] + pre[gu & 7]) * np;
        const long long a0 = ((u >> 3) * pre[8] + pre[u & 7]) * np + (long long)P.xcd_w[u & 7] * (pack > 1 ? wv_phys : 0);
        const long long a1 = a0 + P.xcd_w[u & 7];
        T0 = a0 <= 0 ? 0 : (long long)((double)T * (double)a0 / (double)total);
        T1 = a1 >= total ? T : (long long)((double)T * (double)a1 / (double)total);
    }
    if (!dyn && T1 <= T0) return;
    const long long wc0 = (P.wave_clock || P.xcd_stat) ? wall_clock64() : 0;
    const int n_active = *P.n_active;
    int pend_rec = -1, pend_old = -1, pend_cnt = 0;  // deferred header store of this lane's previous record
    int dbg_comp = 0, dbg_app = 0, dbg_seg = 0;       // probe counters (QK_SCAN_WAVE_CLOCK)
    long long dbg_t_end = 0, dbg_t_stage = 0;         // probe: ticks spent in segment ends / query staging
    for (;;) {
    if (T1 > T0) {
    // 64-ary search for the partition containing tile T0: active[lo].toff <= T0 < active[lo+1].toff
    int lo = 0, hi = n_active;
    while (hi - lo > 1) {
        const int span = hi - lo;
        const int step = (span + 63) >> 6;
        const int probe = min(lo + (lane + 1) * step, hi);          // lanes probe lo+step, lo+2step, ..., hi
        const bool gt = (probe >= hi) || (P.active[probe].toff > T0);  // active[hi].toff > T0 by the invariant
        const uint64_t m = __ballot(gt);
        const int first = __ffsll((unsigned long long)m) - 1;      // first lane whose probe is beyond T0 (always exists)
        const int nlo = min(lo + first * step, hi - 1);
        const int nhi = min(lo + (first + 1) * step, hi);
        lo = nlo;
        hi = nhi;
    }
    int ai = lo;
    long long cur = T0;

    while (cur < T1) {
        // ---- segment = tiles [tl, tend) of item (p, qt) ---------------------------------------------------------
        const ActiveInfo inf = P.active[ai];
        const long long base = inf.toff;
        const int size_p = inf.size;
        const int64_t row_off = inf.row_off;
        const int ntl = (size_p + 15) >> 4;
        const int cnt_p = inf.cnt;
        const int nqt = (cnt_p + 15) >> 4;
        const int G = qshare ? nw : 1;           // query tiles per pass over the partition
        const int ngrp = (nqt + G - 1) / G;      // passes (items) of this partition
        const long long local = cur - base;
        // position inside the partition's weighted sequence (seq_weight): full passes weigh G units per row tile, the last
        // pass q' = 1, 2 or 4; a row tile belongs to the range that holds its first unit
        const int nfull = nqt / G;
        const int ovh = P.seg_ovh;  // units in front of every pass that stand for the cost of starting it (no row tiles)
        const long long wfull = (long long)ntl * G + ovh;
        int grp, wq;
        long long off;
        if (local < nfull * wfull) {
            grp = (int)(local / wfull);
            off = local - grp * wfull;
            wq = G;
        } else {
            grp = nfull;
            off = local - nfull * wfull;
            const int rem = nqt - nfull * G;
            wq = rem <= 1 ? 1 : rem <= 2 ? 2 : 4;
        }
        const long long pass_len = (long long)ntl * wq + ovh;
        const long long off_end = min(pass_len, off + (T1 - cur));
        const int tl_wg = (int)((max(0ll, off - ovh) + wq - 1) / wq);
        const int tend_wg = (int)((max(0ll, off_end - ovh) + wq - 1) / wq);
        cur += off_end - off;
        if (tend_wg <= tl_wg) {  // a range boundary inside one row tile's units or inside the start charge: nothing here
            if (grp == ngrp - 1 && off_end == pass_len) ai++;
            continue;
        }
        // this wave's query tile and its contiguous share of the segment's tiles:
        //   split mode (wide rows) / nw == 1: one query tile, the tiles are cut nw ways;
        //   qshare: the nq_g query tiles of the pass go to waves 0..nq_g-1 (rounded up to a power of two); when the pass
        //   has fewer query tiles than waves, the spare waves take a second / third / fourth cut of the tiles
        int qt = grp, part = wv, parts = nw;
        bool idle = false;
        if (qshare) {
            const int nq_g = min(G, nqt - grp * G);
            const int nq_p = nq_g <= 1 ? 1 : nq_g <= 2 ? 2 : 4;
            parts = max(1, nw / nq_p);
            const int ql = wv % nq_p;
            part = wv / nq_p;
            idle = ql >= nq_g || part >= parts;
            qt = grp * G + min(ql, nq_g - 1);
        }
        const int tl = idle ? tend_wg : tl_wg + (int)(((long long)(tend_wg - tl_wg) * part) / parts);
        const int tend = idle ? tend_wg : tl_wg + (int)(((long long)(tend_wg - tl_wg) * (part + 1)) / parts);
        if (grp == ngrp - 1 && off_end == pass_len) ai++;  // item sequence of this partition exhausted
        const int nq = idle ? 0 : min(16, cnt_p - 16 * qt);
        const int gidx = inf.qoff + 16 * qt + j;
        // grouped entry of this lane's query + record slots for the segment: issued FIRST so that they return first
        // (loads complete in order); the first tile's loads go out right behind them and fly under the query staging
        const int myq = (j < nq) ? P.grouped_q[gidx] : -1;
        const int mypair = (j < nq) ? P.grouped_pair[gidx] : -1;
        int base_rec = 0;
        if (QK_OPT_EARLY_REC && PRODUCT && lane == 0) base_rec = atomicAdd(P.rec_counter, nq);
        uint32_t tau = 0xFFFFFFFFu;
        int cnt = 0;
        dbg_seg++;
        float xnj = 0.0f;
#ifdef QK_SCAN_SHADOW
        bool sh_dead = false;  // this lane's query takes no part (its bound is negative: the finish answers it exactly)
#endif
        {
            // (a wave whose share is empty still issues the static loads: keep them inside the segment)
            const int64_t tile_abs0 = (row_off >> 4) + min(tl, tend_wg - 1);
            const float4 *src = P.vecs + tile_abs0 * nblk * 64 + lane;
            const float4 *nsrc = (const float4 *)(P.norms + (tile_abs0 << 4)) + g;  // +4 float4 per tile
            // ids of this lane's 4 rows travel with the tile (static prefetch): an id load inside the append path
            // would force s_waitcnt vmcnt(0) and drain the prefetched tile every time a candidate passes
            const longlong2 *isrc = (const longlong2 *)(P.ids + (tile_abs0 << 4)) + 2 * g;  // +8 longlong2 per tile
            // norms + ids are double-buffered with the tile data (y0/i0* with a0, y1/i1* with a1): no register copies,
            // so the only wait on a buffer is its first use -- after the following step's loads have been issued
            longlong2 i00 = {0, 0}, i01 = {0, 0}, i10 = {0, 0}, i11 = {0, 0};
#if QK_SCAN_FILT
            // The load stream walks the non-zero words of [tl, tend): fl_bits = those of the 64 tiles from fl_base on that it has
            // not reached yet, lt = the tile (of the list) the next load reads, lt_issued = the tile of the last load issued
            const float4 *srcL = P.vecs + (row_off >> 4) * nblk * 64 + lane;
            const float4 *nsrcL = (const float4 *)(P.norms + row_off) + g;
            const longlong2 *isrcL = (const longlong2 *)(P.ids + row_off) + 2 * g;
            const uint16_t *mrow = P.mask + (row_off >> 4);
#if QK_SCAN_FILT == 2
            // this lane's own mask row, resolved once per segment.  A lane without a query, or whose filter number is outside
            // [0, F) (a device qfilter is not validated by the host), reads the union's word and drops it: qm_keep = 0
            const uint16_t *qmrow = mrow;
            uint32_t qm_keep = 0u;
            if (myq >= 0) {
                const int fi_ = P.qfilter[myq];
                if ((unsigned)fi_ < (unsigned)P.F) {
                    qmrow = P.qmasks[fi_] + (row_off >> 4);
                    qm_keep = 0xFFFFu;
                }
            }
#define QK_MASK_WORD(T) ((uint32_t)qmrow[T] & qm_keep)
#else
#define QK_MASK_WORD(T) (uint32_t)mrow[T]
#endif
#ifdef QK_SCAN_AFTER
            // this lane's own query's cursor, resolved once per segment like qm_keep above.  A lane without a query keeps the
            // exhausted cursor: nothing lies behind it
            uint32_t cur_key = 0xFFFFFFFFu;
            int64_t cur_id = INT64_MAX;
            if (myq >= 0) {
                cur_key = P.after_key[myq];
                cur_id = P.after_id[myq];
            }
#endif
            int fl_base = tl, lt = min(tl, tend_wg - 1), lt_issued = lt;
            uint64_t fl_bits = 0;
            uint32_t y0_m = 0, y1_m = 0;  // the tile's word, double-buffered with its norms (y0 / y1) and ids
            auto nz_next = [&]() -> int {
                while (fl_bits == 0) {
                    fl_base += 64;
                    if (fl_base >= tend) return tend - 1;  // (not reached: nsteps counts the non-zero words)
                    const int t_ = fl_base + lane;
                    const uint32_t w_ = t_ < tend ? (uint32_t)mrow[t_] : 0u;
                    fl_bits = __ballot(w_ != 0u);
                }
                const int t_ = fl_base + __ffsll((unsigned long long)fl_bits) - 1;
                fl_bits &= fl_bits - 1;
                return t_;
            };
            int nnz = 0;
            for (int b_ = tl; b_ < tend; b_ += 64) {
                const int t_ = b_ + lane;
                const uint32_t w_ = t_ < tend ? (uint32_t)mrow[t_] : 0u;
                const uint64_t mm_ = __ballot(w_ != 0u);
                if (b_ == tl) fl_bits = mm_;
                nnz += __popcll(mm_);
            }
            const int nsteps = nnz * ncd;
            if (nnz > 0) lt = nz_next();
            lt_issued = lt;
#else
            const int nsteps = (tend - tl) * ncd;
#endif
            float4 a0[DB], a1[DB];
            float4 y0 = make_float4(0.f, 0.f, 0.f, 0.f), y1 = y0;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            float probe_sink = 0.f;
            int dch = 0;    // d-chunk of the step being computed
#if QK_SCAN_FILT
            int tile = lt;  // tile of the step being computed
#else
            int tile = tl;  // tile of the step being computed
#endif
            int ldch = 0;   // d-chunk of the step being loaded
            int ltile = 0;  // tiles loaded so far (relative)

            // The load stream is STATIC (same loads every iteration, clamped at the end of the segment) so that the
            // compiler can place counted s_waitcnt vmcnt(N) and keep the next step's loads in flight under the MFMAs.
            int lS = 0;  // next step to load (clamped to nsteps-1)
#if QK_SCAN_FILT
#define QK_EPI_M(Y) , Y##_m
#define QK_NEXT_TILE tile = lt_issued /* the tile of the step loaded last is the tile of the step computed next */
#define QK_LOAD(A, Y, I0, I1)                                         \
    {                                                                 \
        const float4 *pp_ = srcL + ((int64_t)lt * ncd + ldch) * (DB * 64); \
        _Pragma("unroll") for (int b_ = 0; b_ < DB; b_++)             \
            A[b_] = qk_ld_stream(pp_ + b_ * 64);                      \
        Y = nsrcL[(int64_t)lt * 4];                                   \
        I0 = isrcL[(int64_t)lt * 8];                                  \
        I1 = isrcL[(int64_t)lt * 8 + 1];                              \
        Y##_m = QK_MASK_WORD(lt);                                     \
        lt_issued = lt;                                               \
        if (lS < nsteps - 1) {                                        \
            lS++;                                                     \
            if (++ldch == ncd) {                                      \
                ldch = 0;                                             \
                lt = nz_next();                                       \
            }                                                         \
        }                                                             \
    }
#elif defined(QK_SCAN_SHADOW)
#define QK_EPI_M(Y)
#define QK_NEXT_TILE tile++
#define QK_LOAD(A, Y, I0, I1)                                         \
    {                                                                 \
        const float4 *pp_ = src + (int64_t)lS * (DB * 64);            \
        _Pragma("unroll") for (int b_ = 0; b_ < DB; b_++)             \
            A[b_] = qk_ld_stream(pp_ + b_ * 64);                      \
        Y = nsrc[(int64_t)ltile * 4];                                 \
        if (lS < nsteps - 1) {                                        \
            lS++;                                                     \
            if (++ldch == ncd) {                                      \
                ldch = 0;                                             \
                ltile++;                                              \
            }                                                         \
        }                                                             \
    }
#else
#define QK_EPI_M(Y)
#define QK_NEXT_TILE tile++
#define QK_LOAD(A, Y, I0, I1)                                         \
    {                                                                 \
        const float4 *pp_ = src + (int64_t)lS * (DB * 64);            \
        if (qshare) { /* the other waves of the workgroup read the same tile: keep it cacheable */ \
            _Pragma("unroll") for (int b_ = 0; b_ < DB; b_++) A[b_] = pp_[b_ * 64];      \
        } else {                                                      \
            _Pragma("unroll") for (int b_ = 0; b_ < DB; b_++)         \
                A[b_] = qk_ld_stream(pp_ + b_ * 64);                  \
        }                                                             \
        Y = nsrc[(int64_t)ltile * 4];                                 \
        I0 = isrc[(int64_t)ltile * 8];                                \
        I1 = isrc[(int64_t)ltile * 8 + 1];                            \
        if (lS < nsteps - 1) {                                        \
            lS++;                                                     \
            if (++ldch == ncd) {                                      \
                ldch = 0;                                             \
                ltile++;                                              \
            }                                                         \
        }                                                             \
    }
#endif

#ifdef QK_SCAN_SHADOW
#define QK_DOT(A_, B_) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qk_as_h8(A_), qk_as_h8(B_), acc, 0, 0, 0);
#else
#define QK_DOT(A_, B_)                                                        \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A_.x, B_.x, acc, 0, 0, 0);     \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A_.y, B_.y, acc, 0, 0, 0);     \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A_.z, B_.z, acc, 0, 0, 0);     \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A_.w, B_.w, acc, 0, 0, 0);
#endif
#define QK_STEP(A, Y, I0, I1, LIVE)                                                                                    \
    {                                                                                                      \
        if (dch == 0) acc = (f32x4){0.f, 0.f, 0.f, 0.f};                                                   \
        _Pragma("unroll") for (int b_ = 0; b_ < DB; b_++) {                                                \
            if (MODE == 2) {                                                                               \
                acc[0] += A[b_].x;                                                                         \
                acc[1] += A[b_].y;                                                                         \
                acc[2] += A[b_].z;                                                                         \
                acc[3] += A[b_].w;                                                                         \
            } else {                                                                                       \
                const float4 bq_ = qs[(dch * DB + b_) * 64 + lane];                                        \
                QK_DOT(A[b_], bq_)                                                                         \
            }                                                                                              \
        }                                                                                                  \
        if (++dch == ncd) {                                                                                \
            dch = 0;                                                                                       \
            if (PRODUCT || EMIT) {                                                                         \
                epilogue(tile, LIVE, Y, I0, I1 QK_EPI_M(Y));                                               \
            } else {                                                                                       \
                probe_sink += acc[0] + acc[1] + acc[2] + acc[3] + Y.x + (float)I0.x + (float)I1.x;         \
            }                                                                                              \
            QK_NEXT_TILE;                                                                                  \
        }                                                                                                  \
    }

#if QK_SCAN_FILT
            auto epilogue = [&](int tl_, bool live, const float4 yn, const longlong2 ia, const longlong2 ib, const uint32_t mw) {
#else
            auto epilogue = [&](int tl_, bool live, const float4 yn, const longlong2 ia, const longlong2 ib) {
#endif
                const int row0 = tl_ << 4;
                const float yv[4] = {yn.x, yn.y, yn.z, yn.w};
#ifdef QK_SCAN_SHADOW
                const int64_t row_abs_ = row_off + row0 + 4 * g;
                const int64_t idv[4] = {row_abs_, row_abs_ + 1, row_abs_ + 2, row_abs_ + 3};
#else
                const int64_t idv[4] = {ia.x, ia.y, ib.x, ib.y};
#endif
                if (EMIT) {
                    if (live && myq >= 0) {
                        uint32_t *dst = P.key_out + P.pair_base[mypair] + row0 + 4 * g;
#pragma unroll
                        for (int reg = 0; reg < 4; reg++) {
                            const float v = acc[reg];
                            if (row0 + 4 * g + reg < size_p)
                                dst[reg] = l2 ? ord_from_l2(l2_expanded(xnj, yv[reg], v)) : ord_from_ip(v);
                        }
                    }
                    return;
                }
                // every 8 tiles pick up bounds published by other waves working on the same query (only when queries
                // probe more than one partition: gtau is null otherwise).  Measured (scan_probe.py, 10M x 128, P=32)
                // against a per-tile plain (L1-stale) load, a per-tile sc1 load in the prefetch stream and an
                // exchange at compaction time: this variant is 5-25 % faster although consuming the load drains
                // the prefetched tile.
                if (P.gtau && P.tau_refresh && (tl_ & 7) == 7 && myq >= 0)
                    tau = min(tau, ~__hip_atomic_load(&P.gtau[myq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                uint32_t ordv[4];
                bool anyp = false;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = row0 + 4 * g + reg;
#if QK_SCAN_FILT
                    const bool valid = live && (myq >= 0) && (row < size_p) && ((mw >> (4 * g + reg)) & 1u);
#elif defined(QK_SCAN_SHADOW)
                    const bool valid = live && (myq >= 0) && (row < size_p) && !sh_dead;
#else
                    const bool valid = live && (myq >= 0) && (row < size_p);
#endif
                    const float v = acc[reg];
                    const uint32_t o = l2 ? ord_from_l2(l2_expanded(xnj, yv[reg], v)) : ord_from_ip(v);
#ifdef QK_SCAN_AFTER
                    // a row at or before the cursor is no candidate: it never reaches a pool, so it never sets a bound either
                    const bool cand = valid && qk_behind_cursor(o, idv[reg], cur_key, cur_id);
                    ordv[reg] = cand ? o : 0xFFFFFFFFu;
                    anyp |= cand && o <= tau;
#else
                    ordv[reg] = valid ? o : 0xFFFFFFFFu;  // an invalid row can never pass (tau < 0xFFFFFFFF once set; see below)
                    anyp |= valid && o <= tau;
#endif
                }
                // steady state: nothing beats the running k-th best -> one ballot, one branch per tile
                if (!QK_OPT_ONE_BALLOT || __ballot(anyp)) {
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const uint32_t ord = ordv[reg];
                        const bool pass = ord != 0xFFFFFFFFu && ord <= tau;
                        const uint64_t m = __ballot(pass);
                        if (m) {
                            const uint64_t gm = m & (0x0001000100010001ull << j);
                            if (pass) {
                                const int slot = cnt + __popcll(gm & ((1ull << lane) - 1ull));
                                my_ord[slot] = ord;
                                my_id[slot] = idv[reg];
                            }
                            cnt += __popcll(gm);
                            dbg_app += __popcll(m);
                            uint64_t need = __ballot(cnt > C - 4) & 0xFFFFull;
                            while (need) {
                                dbg_comp++;
                                const int jq = __ffsll((unsigned long long)need) - 1;
                                need &= need - 1;
                                const int n = __builtin_amdgcn_readlane(cnt, jq);
                                uint32_t kth;
                                int nn;
                                if (MAXCH > 1 || QK_OPT_SELECT1) {
                                    nn = select_pool<MAXCH>(pool_ord + jq * C, pool_id + jq * C, n, k, lane, kth);
                                } else {
                                    nn = compact_pool<MAXCH>(pool_ord + jq * C, pool_id + jq * C, n, k, lane);
                                    kth = nn >= k ? pool_ord[jq * C + k - 1] : 0xFFFFFFFFu;
                                }
                                if (j == jq) {
                                    cnt = nn;
                                    if (nn >= k) {
                                        tau = min(tau, kth);
                                        // publish (fire and forget: no returned value, no wait)
                                        if (P.gtau && P.tau_publish && lane < 16) atomicMax(&P.gtau[myq], ~tau);
                                    }
                                }
                            }
                        }
                    }
                }
            };

            if (QK_OPT_EARLY_LOAD) QK_LOAD(a0, y0, i00, i01);
            // ---- query tile -> LDS in B-operand lane order (wave-private), while the first tile is in flight --------
            const long long dbg_s0 = P.wave_clock ? wall_clock64() : 0;
            {
                const int qsafe = myq >= 0 ? myq : 0;
                const float4 *qsrc = P.xq4 + (int64_t)qsafe * nblk * 4 + g;
                if (P.gtau) tau = ~__hip_atomic_load(&P.gtau[qsafe], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (l2) xnj = P.xn[qsafe];
#ifdef QK_SCAN_SHADOW
                {  // the seed's exact bound, widened by what an approximate key may lie above its exact one
                    const float she_ = P.sh_E[qsafe];
                    sh_dead = !(she_ >= 0.0f);
                    tau = qk_ord_widen(tau, sh_dead ? 0.0f : she_, l2);
                }
#endif
                // LDS only (no vmcnt wait: the first tile stays in flight): every wave has left the previous tile
                const bool coop = nw > 1 && !qshare;  // split mode: one query tile staged by all waves, fenced by barriers
                if (coop) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                for (int cb0 = coop ? wv * DB : 0; cb0 < nblk; cb0 += coop ? nw * DB : DB) {
                    float4 qv[DB];
#pragma unroll
                    for (int b = 0; b < DB; b++) qv[b] = qsrc[(cb0 + b) * 4];
#pragma unroll
                    for (int b = 0; b < DB; b++) {
                        if (myq < 0) qv[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                        qs[(cb0 + b) * 64 + lane] = qv[b];
                    }
                }
                if (myq < 0) {
                    tau = 0xFFFFFFFFu;
                    xnj = 0.0f;
                }
                if (coop) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            if (P.wave_clock) dbg_t_stage += wall_clock64() - dbg_s0;
            if (!QK_OPT_EARLY_LOAD) QK_LOAD(a0, y0, i00, i01);
            // (a third tile buffer was measured twice at 4 waves per CU: 0.265 -> 0.296 ms, slower, with counted vmcnt waits in
            //  the ISA; at 3 waves per CU it makes no difference.  Probe modes on the bench configuration: loads only 0.229 ms,
            //  + MFMA 0.236 ms, + top-k 0.265 ms at any of 4 / 6 / 8 waves per CU -- the gap to the stream is the top-k path
            //  (cold starts after the seed bound, segment-end compaction and record emission), not latency hiding.)
            for (int s = 0; s < nsteps; s += 2) {
                QK_LOAD(a1, y1, i10, i11);
                QK_STEP(a0, y0, i00, i01, true);
                if (QK_OPT_STEP_DRAIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                QK_LOAD(a0, y0, i00, i01);
                QK_STEP(a1, y1, i10, i11, s + 1 < nsteps);
                if (QK_OPT_STEP_DRAIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
#undef QK_LOAD
#undef QK_STEP
#undef QK_DOT
#undef QK_EPI_M
#undef QK_NEXT_TILE
#if QK_SCAN_FILT
#undef QK_MASK_WORD
#endif
            if (!PRODUCT && probe_sink == 12345.678f) my_ord[0] = 1;  // keep the probe's loads alive
        }
        // ---- segment end: final compaction (sorts, caps at k), publish bound, emit records ---------------------------
        const long long dbg_e0 = P.wave_clock ? wall_clock64() : 0;
        {
            uint64_t need = __ballot(cnt > 0) & 0xFFFFull;
            while (need) {
                const int jq = __ffsll((unsigned long long)need) - 1;
                need &= need - 1;
                const int n = __builtin_amdgcn_readlane(cnt, jq);
                const int nn = compact_pool<MAXCH>(pool_ord + jq * C, pool_id + jq * C, n, k, lane);
                if (j == jq) cnt = nn;
            }
            const uint64_t have = __ballot(cnt > 0) & 0xFFFFull;
            if (have) {
                // the two atomics of an emission -- a slot in the pair's line, record numbers for the segment -- do not depend
                // on each other: both are issued before either result is awaited (one round trip instead of two)
                int slot = -1;
                if (lane < 16 && cnt > 0) slot = atomicAdd(&P.pair_slots[(int64_t)mypair * QK_SLOTS], 1);
                if (!QK_OPT_EARLY_REC && lane == 0) base_rec = atomicAdd(P.rec_counter, nq);
                const int rec0 = __builtin_amdgcn_readfirstlane(base_rec);
                int myrec = -1;
                if (lane < 16 && cnt > 0) {
                    myrec = rec0 + lane;
                    // the first 31 records of a pair are listed in its slot line (the merge fetches them together, no
                    // pointer chase); further ones are chained through pair_head.  (max_recs is an upper bound of the
                    // records a launch can emit; a slot taken for a record beyond it reads as "none")
                    if (slot < QK_SLOTS - 1) P.pair_slots[(int64_t)mypair * QK_SLOTS + 1 + slot] = myrec < P.max_recs ? myrec : -1;
                    if (myrec >= P.max_recs) *P.overflow = 1;  // never, if the host bound holds: the context reports it
                    if (myrec < P.max_recs) {
                        // the store of the previous head is deferred to the next emit (or kernel end) so that the
                        // wave does not stall on the exchange's round trip
                        if (pend_rec >= 0) P.rec_hdr[pend_rec] = make_int2(pend_old, pend_cnt);
                        pend_old = -1;
                        if (slot >= QK_SLOTS - 1) pend_old = atomicExch(&P.pair_head[mypair], myrec);
                        pend_rec = myrec;
                        pend_cnt = cnt;
                        if (!QK_OPT_EARLY_REC) {
                            P.rec_hdr[pend_rec] = make_int2(pend_old, pend_cnt);
                            pend_rec = -1;
                        }
                        if (P.gtau && P.tau_publish && cnt >= k) atomicMax(&P.gtau[myq], ~my_ord[k - 1]);
                    }
                }
                uint64_t todo = have;
                while (todo) {
                    const int jq = __ffsll((unsigned long long)todo) - 1;
                    todo &= todo - 1;
                    const int n = __builtin_amdgcn_readlane(cnt, jq);
                    const int rec = __builtin_amdgcn_readlane(myrec, jq);
                    if (rec < P.max_recs)
                        for (int e = lane; e < n; e += 64) {
                            P.rec_ord[(int64_t)rec * k + e] = pool_ord[jq * C + e];
                            P.rec_id[(int64_t)rec * k + e] = pool_id[jq * C + e];
                        }
                }
            }
        }
        if (P.wave_clock) dbg_t_end += wall_clock64() - dbg_e0;
    }
    }  // range
        if (!dyn) break;
        unsigned long long c = 0;
        if (lane == 0) c = atomicAdd(P.dyn_counter, (unsigned long long)P.dyn_chunk);
        c = __shfl(c, 0);
        T0 = Ts + (long long)c;
        if (T0 >= T) break;
        T1 = min(T, T0 + P.dyn_chunk);
    }
    if (pend_rec >= 0) P.rec_hdr[pend_rec] = make_int2(pend_old, pend_cnt);
    if (P.xcd_stat && lane == 0 && (nw == 1 || wv == 0)) {
        atomicAdd(&P.xcd_stat[blockIdx.x & 7], (unsigned long long)(wall_clock64() - wc0));
        atomicAdd(&P.xcd_stat[8 + (blockIdx.x & 7)], 1ull);
    }
    if (P.wave_clock && lane == 0) {
        long long *wcp = P.wave_clock + 8 * (pack > 1 ? vblock : (long long)blockIdx.x * nw + wv);
        wcp[0] = wc0;
        wcp[1] = wall_clock64();
        wcp[2] = dbg_comp;
        wcp[3] = dbg_app;
        wcp[4] = dbg_seg;
        wcp[5] = dbg_t_end;
        wcp[6] = dbg_t_stage;
        // where the wave ran: HW_ID (simd [5:4], cu [11:8], sh [12], se [15:13]) and XCC_ID [3:0]
        const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | ((32 - 1) << 11));
        const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11));
        wcp[7] = ((long long)xcc << 32) | hw;
    }
