// qk_emit.hip -- the host side every entry point on the key-emission scan shares: range search (qk_range.hip), grouped search
// (qk_grouped.hip), facet counts and facet statistics (qk_facet.hip), ordered search (qk_order.hip).  No kernels.
//
// qk_emit_run is the body of all of them.  An entry point checks its handles and its list arguments, describes the call in a
// qk_emit_call (qk_internal.h) -- names, the common arguments, its own checks, the columns it reads, its outputs as a table, its
// device half -- and calls it.  The refusals keep one order: metric, NaN radius, the pipeline's own, null argument, an overflow
// left behind by an earlier call, then the front end's, the filter's and the pass plan's.
// qk_emit_device is the bracket of every device half: the phase events, the answer of a call without lists, qk_emit_passes
// (qk_dense.hip, next to its pair-offset kernels), the name of the scan kernel as ctx->last_scan_kernel reports it.
#include "qk_attr.h"

#include <cstring>

int qk_emit_run(qk_emit_call &c) {
    qk_ctx *ctx = c.ctx;
    qk_store *s = c.s;
    const int64_t Q = c.Q;
    qk_timing *timing = c.timing;
    const bool host = c.mem == QK_MEM_HOST;
    if (c.metric != QK_METRIC_L2 && c.metric != QK_METRIC_IP) QK_FAIL(QK_ERR_INVALID, "Metric type not supported");
    if (c.has_radius && c.radius != c.radius) QK_FAIL(QK_ERR_INVALID, "%s: the radius is NaN", c.who);
    if (c.check) QK_TRY(c.check());
    bool missing = !c.x;
    for (int i = 0; i < c.n_outs; i++) missing = missing || (c.outs[i].required && !c.outs[i].host);
    if (Q < 0 || (Q > 0 && missing)) QK_FAIL(QK_ERR_INVALID, "%s: null argument", c.who);
    QK_TRY(qk_check_overflow(ctx));
    QK_HIP(hipSetDevice(ctx->device));
    if (timing) memset(timing, 0, sizeof(*timing));
    if (Q == 0) return c.on_empty ? c.on_empty() : QK_OK;
    hipStream_t st = ctx->stream;
    // ---- staging, query preparation, coarse; a host caller's outputs on the device, in the table's order ----------------------------
    size_t out_bytes = 0;
    for (int i = 0; i < c.n_outs; i++) out_bytes += qk_al256(c.outs[i].bytes);
    qk_emit_env e;
    char *stage = nullptr;
    bool have_coarse = false;
    QK_TRY(qk_emit_front_end(ctx, c.parent, s, c.x, Q, c.pids, c.P, c.nprobe, c.metric, c.mem, out_bytes, timing != nullptr, &e.a, &stage,
                             &have_coarse));
    for (int i = 0; i < c.n_outs; i++) {
        qk_emit_out &o = c.outs[i];
        o.dev = !host ? o.host : o.host ? stage : nullptr;
        if (host) stage += qk_al256(o.bytes);
    }
    if (c.has_radius && !qk_range_key_bounds(c.metric, e.a.sqrt_l2, c.radius, &e.key_lo, &e.key_hi)) {
        e.key_lo = 1;  // (empty interval)
        e.key_hi = 0;
    }
    // ---- mask and row values, then the pipeline: emission and what it does with the keys ------------------------------------------
    if (c.filter) QK_TRY(qk_filter_ensure(ctx, s, c.filter, &e.mask));
    QK_TRY(qk_store_sync_table(s));
    for (int i = 0; i < c.n_cols; i++) {
        bool seen = false;  // (the same column twice: derived once)
        for (int j = 0; j < i; j++) seen = seen || c.cols[j] == c.cols[i];
        if (!seen) QK_TRY(qk_rowvals_ensure(ctx, s, *c.cols[i]));
    }
    e.npids = (int)s->parts.size();
    e.P = e.a.all_lists ? e.npids : e.a.P;
    QK_TRY(c.device(e));
    // ---- results back ------------------------------------------------------------------------------------------------------------
    if (host && c.copy_back) {
        QK_TRY(c.copy_back());
    } else if (host) {
        for (int i = 0; i < c.n_outs; i++) {
            const qk_emit_out &o = c.outs[i];
            if (o.host) QK_HIP(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, st));
        }
        QK_HIP(hipStreamSynchronize(st));
    }
    if (timing) {
        // the scalars of the wide-k path: no list statistics (but range search's, fill_timing); n_items = the query passes of the call
        QK_HIP(hipStreamSynchronize(st));
        timing->n_items = e.n_passes;
        if (c.fill_timing) QK_TRY(c.fill_timing());
        QK_TRY(qk_read_phase_ms(ctx, timing, have_coarse, 4));
    }
    if (timing || host) QK_TRY(qk_check_overflow(ctx));
    return QK_OK;
}

int qk_emit_device(const qk_emit_call &c, qk_emit_env &e, const qk_emit_stages &st) {
    qk_ctx *ctx = c.ctx;
    e.n_passes = 0;
    qk_phase_events pe;
    pe.ctx = ctx;
    pe.tm = ctx->timing && c.timing;
    pe.dtm = false;
    pe.ev_base = 4;
    if (e.P <= 0 || e.npids <= 0) {  // no lists: no candidates
        QK_TRY(pe.mark(0));
        QK_TRY(qk_prep_flush(ctx));
        QK_TRY(st.pad());
        for (int i = 1; i <= 3; i++) QK_TRY(pe.mark(i));
        return QK_OK;
    }
    QK_TRY(qk_emit_passes(ctx, c.s, e.a, e.P, c.pipeline, pe, st.h, &e.n_passes));
    if (st.tail) QK_TRY(st.tail());
    const bool wide = strcmp(ctx->last_scan_kernel, "k_scan_wide") == 0;
    ctx->last_scan_kernel = wide ? c.label_wide : c.label;
    QK_TRY(pe.mark(3));
    return QK_OK;
}
