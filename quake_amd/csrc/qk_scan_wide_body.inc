// qk_scan_wide_body.inc -- the body of k_scan_wide (qk_scan_wide.hip), included once per kernel: QK_SCAN_FILT 0 = k_scan_wide as it
// always was (same preprocessed text, so its code does not move), QK_SCAN_FILT 1 = k_scan_wide_filt, which reads ScanParams::mask
// (one 16-bit word per arena tile, qk_filter.hip): a row passes the epilogue only with its bit set, and the walk jumps over tiles
// whose word is 0 (a tile of a wide row is 16 x d x 4 bytes: 192 KB at d = 3072).  QK_SCAN_FILT 2 = k_scan_wide_filtq, one filter
// per query: the walk jumps by ScanParams::mask, the OR of the call's masks; the epilogue's word is the lane's own query's
// (qmasks[qfilter[myq]], see qk_scan_body.inc).  QK_SCAN_AFTER (with QK_SCAN_FILT 1) = k_scan_wide_after: the filtered body plus
// the cursor test of paged search in the epilogue (see qk_scan_body.inc); its lines sit behind #ifdef QK_SCAN_AFTER.
// Expects: template parameters L2, MAXCH, EMIT and the kernel argument `ScanParams P` in scope.
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int R = QK_WIDE_R;
    constexpr bool l2 = L2;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    const int nblk = P.nblk, C = P.C, k = P.k;
    int64_t *pool_id = (int64_t *)smem;                            // [16][C]
    uint32_t *pool_ord = (uint32_t *)(smem + (size_t)16 * C * 8);  // [16][C]
    uint32_t *my_ord = pool_ord + j * C;
    int64_t *my_id = pool_id + j * C;

    const long long T = *P.n_tiles;
    const long long W = gridDim.x, vb = blockIdx.x;
    const long long T0 = (T * vb) / W, T1 = (T * (vb + 1)) / W;
    if (T1 <= T0) return;
    const int n_active = *P.n_active;
    // 64-ary search for the partition containing tile T0: active[lo].toff <= T0 < active[lo+1].toff
    int lo = 0, hi = n_active;
    while (hi - lo > 1) {
        const int span = hi - lo;
        const int step = (span + 63) >> 6;
        const int probe = min(lo + (lane + 1) * step, hi);
        const bool gt = (probe >= hi) || (P.active[probe].toff > T0);
        const uint64_t m = __ballot(gt);
        const int first = __ffsll((unsigned long long)m) - 1;
        const int nlo = min(lo + first * step, hi - 1);
        const int nhi = min(lo + (first + 1) * step, hi);
        lo = nlo;
        hi = nhi;
    }
    int ai = lo;
    long long cur = T0;
    while (cur < T1) {
        // ---- segment = tiles [tl, tend) of item (p, qt): k_scan's walk with one query tile per pass ----------------------------
        const ActiveInfo inf = P.active[ai];
        const long long local = cur - inf.toff;
        const int size_p = inf.size;
        const int ntl = (size_p + 15) >> 4;
        const int nqt = (inf.cnt + 15) >> 4;
        const int ovh = P.seg_ovh;
        const long long pass_len = (long long)ntl + ovh;
        const int qt = (int)(local / pass_len);
        const long long off = local - qt * pass_len;
        const long long off_end = min(pass_len, off + (T1 - cur));
        const int tl = (int)max(0ll, off - ovh);
        const int tend = (int)max(0ll, off_end - ovh);
        cur += off_end - off;
        if (qt == nqt - 1 && off_end == pass_len) ai++;  // item sequence of this partition exhausted
        if (tend <= tl) continue;
        const int nq = min(16, inf.cnt - 16 * qt);
        const int gidx = inf.qoff + 16 * qt + j;
        const int myq = (j < nq) ? P.grouped_q[gidx] : -1;
        const int mypair = (j < nq) ? P.grouped_pair[gidx] : -1;
        const int qsafe = myq >= 0 ? myq : 0;
        uint32_t tau = 0xFFFFFFFFu;
        float xnj = 0.0f;
        if (myq >= 0) {
            if (P.gtau) tau = ~__hip_atomic_load(&P.gtau[myq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (l2) xnj = P.xn[myq];
        }
        int cnt = 0;
#if QK_SCAN_FILT == 2
        // this lane's own mask, resolved once per segment; no query / a filter number outside [0, F): the union's word, dropped
        const uint16_t *qmask = P.mask;
        uint32_t qm_keep = 0u;
        if (myq >= 0) {
            const int fi_ = P.qfilter[myq];
            if ((unsigned)fi_ < (unsigned)P.F) {
                qmask = P.qmasks[fi_];
                qm_keep = 0xFFFFu;
            }
        }
#endif
#ifdef QK_SCAN_AFTER
        // this lane's own query's cursor, resolved once per segment; no query: the exhausted cursor, nothing lies behind it
        uint32_t cur_key = 0xFFFFFFFFu;
        int64_t cur_id = INT64_MAX;
        if (myq >= 0) {
            cur_key = P.after_key[myq];
            cur_id = P.after_id[myq];
        }
#endif
        const float4 *qsrc = P.xq4 + (int64_t)qsafe * nblk * 4 + g;
        auto bload = [&](int c) { return qsrc[c * 4]; };

        // one tile's keys -> the pools (k_scan's epilogue), or -> key_out
        auto epilogue = [&](int tile, const f32x4 &acc) {
            const int64_t tile_abs = (inf.row_off >> 4) + tile;
            const int row0 = tile << 4;
            const float4 yn = l2 ? ((const float4 *)(P.norms + (tile_abs << 4)))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float yv[4] = {yn.x, yn.y, yn.z, yn.w};
            if (EMIT) {
                if (myq >= 0) {
                    uint32_t *dst = P.key_out + P.pair_base[mypair] + row0 + 4 * g;
#pragma unroll
                    for (int reg = 0; reg < 4; reg++)
                        if (row0 + 4 * g + reg < size_p) dst[reg] = l2 ? ord_from_l2(l2_expanded(xnj, yv[reg], acc[reg])) : ord_from_ip(acc[reg]);
                }
                return;
            }
            const longlong2 ia = ((const longlong2 *)(P.ids + (tile_abs << 4)))[2 * g];
            const longlong2 ib = ((const longlong2 *)(P.ids + (tile_abs << 4)))[2 * g + 1];
            const int64_t idv[4] = {ia.x, ia.y, ib.x, ib.y};
#if QK_SCAN_FILT == 2
            const uint32_t mw = (uint32_t)qmask[tile_abs] & qm_keep;  // this tile's word under this lane's query's filter
#elif QK_SCAN_FILT
            const uint32_t mw = (uint32_t)P.mask[tile_abs];  // this tile's word: bit r = row r is a candidate
#endif
            if (P.gtau && P.tau_refresh && (tile & 7) == 7 && myq >= 0)
                tau = min(tau, ~__hip_atomic_load(&P.gtau[myq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            uint32_t ordv[4];
            bool anyp = false;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
#if QK_SCAN_FILT
                const bool valid = (myq >= 0) && (row0 + 4 * g + reg < size_p) && ((mw >> (4 * g + reg)) & 1u);
#else
                const bool valid = (myq >= 0) && (row0 + 4 * g + reg < size_p);
#endif
                const uint32_t o = l2 ? ord_from_l2(l2_expanded(xnj, yv[reg], acc[reg])) : ord_from_ip(acc[reg]);
#ifdef QK_SCAN_AFTER
                const bool cand = valid && qk_behind_cursor(o, idv[reg], cur_key, cur_id);
                ordv[reg] = cand ? o : 0xFFFFFFFFu;
                anyp |= cand && o <= tau;
#else
                ordv[reg] = valid ? o : 0xFFFFFFFFu;
                anyp |= valid && o <= tau;
#endif
            }
            if (!__ballot(anyp)) return;
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
                    uint64_t need = __ballot(cnt > C - 4) & 0xFFFFull;
                    while (need) {
                        const int jq = __ffsll((unsigned long long)need) - 1;
                        need &= need - 1;
                        const int n = __builtin_amdgcn_readlane(cnt, jq);
                        uint32_t kth;
                        const int nn = select_pool<MAXCH>(pool_ord + jq * C, pool_id + jq * C, n, k, lane, kth);
                        if (j == jq) {
                            cnt = nn;
                            if (nn >= k) {
                                tau = min(tau, kth);
                                if (P.gtau && P.tau_publish && lane < 16) atomicMax(&P.gtau[myq], ~tau);
                            }
                        }
                    }
                }
            }
        };

        const float4 *src = P.vecs + ((inf.row_off >> 4) + tl) * (int64_t)nblk * 64 + lane;
        for (int t0 = tl; t0 < tend; t0 += R) {
#if QK_SCAN_FILT
            {  // on to the next tile of [t0, tend) that has a candidate: the group of R tiles starts there
                const uint16_t *mrow = P.mask + (inf.row_off >> 4);
                while (t0 < tend) {
                    const int t_ = t0 + lane;
                    const uint32_t w_ = t_ < tend ? (uint32_t)mrow[t_] : 0u;
                    const uint64_t nz = __ballot(w_ != 0u);
                    if (nz) {
                        t0 += __ffsll((unsigned long long)nz) - 1;
                        break;
                    }
                    t0 += 64;
                }
                if (t0 >= tend) break;
            }
#endif
            const int nr = min(R, tend - t0);
            f32x4 acc[R];
            wide_tiles<true>(acc, src + (int64_t)(t0 - tl) * nblk * 64, (int64_t)nblk * 64, nr, nblk, bload);
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < nr) epilogue(t0 + r, acc[r]);
        }
        if (EMIT) continue;
        // ---- segment end: final compaction (sorts, caps at k), publish bound, emit records (as k_scan) ---------------------------
        uint64_t need = __ballot(cnt > 0) & 0xFFFFull;
        while (need) {
            const int jq = __ffsll((unsigned long long)need) - 1;
            need &= need - 1;
            const int n = __builtin_amdgcn_readlane(cnt, jq);
            const int nn = compact_pool<MAXCH>(pool_ord + jq * C, pool_id + jq * C, n, k, lane);
            if (j == jq) cnt = nn;
        }
        const uint64_t have = __ballot(cnt > 0) & 0xFFFFull;
        if (!have) continue;
        int slot = -1, base_rec = 0;
        if (lane < 16 && cnt > 0) slot = atomicAdd(&P.pair_slots[(int64_t)mypair * QK_SLOTS], 1);
        if (lane == 0) base_rec = atomicAdd(P.rec_counter, nq);
        const int rec0 = __builtin_amdgcn_readfirstlane(base_rec);
        int myrec = -1;
        if (lane < 16 && cnt > 0) {
            myrec = rec0 + lane;
            if (slot < QK_SLOTS - 1) P.pair_slots[(int64_t)mypair * QK_SLOTS + 1 + slot] = myrec < P.max_recs ? myrec : -1;
            if (myrec >= P.max_recs) *P.overflow = 1;
            if (myrec < P.max_recs) {
                const int old = slot >= QK_SLOTS - 1 ? atomicExch(&P.pair_head[mypair], myrec) : -1;
                P.rec_hdr[myrec] = make_int2(old, cnt);
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
