// query_coordinator.cpp -- see query_coordinator.h.  No arithmetic here: tensors are marshalled to the C ABI.
#include "query_coordinator.h"

#include <c10/hip/HIPStream.h>

#include <chrono>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "maintenance_policies.h"
#include "partition_manager.h"
#include "quake_index.h"

namespace quake_amd {

namespace {
using clk = std::chrono::high_resolution_clock;
inline int64_t ns_since(clk::time_point t0) { return std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t0).count(); }

// Device tensors in: the library works on torch's CURRENT stream for the length of the call (the newly bound stream waits for
// the previous one through an event, qk_ctx_set_stream), so it is ordered behind whatever produced the inputs and the outputs are
// ordered in front of whatever torch enqueues next -- no device-wide synchronisation.  The context is shared (one per device):
// the binding it had on entry -- its private stream, the NULL stream, or a stream a caller bound it to -- comes back on every
// way out.
struct BoundToTorchStream {
    qk_ctx *c = nullptr;
    void *prev = nullptr;
    int prev_kind = 0;
    BoundToTorchStream(qk_ctx *ctx, const Tensor &t) {
        if (!ctx || !t.is_cuda()) return;
        qk_check(qk_ctx_get_stream(ctx, &prev, &prev_kind));
        c = ctx;
        hipStream_t st = c10::hip::getCurrentHIPStream(t.device().index()).stream();
        qk_check(st ? qk_ctx_set_stream(c, (void *)st) : qk_ctx_set_null_stream(c));
    }
    ~BoundToTorchStream() {
        if (!c) return;
        if (prev_kind == 1) (void)qk_ctx_set_null_stream(c);
        else (void)qk_ctx_set_stream(c, prev_kind == 2 ? prev : nullptr);
    }
};
}  // namespace

QueryCoordinator::QueryCoordinator(shared_ptr<QuakeIndex> parent, shared_ptr<PartitionManager> partition_manager,
                                   shared_ptr<MaintenancePolicy> maintenance_policy, MetricType metric, int num_workers)
    : partition_manager_(partition_manager), maintenance_policy_(maintenance_policy), parent_(parent), metric_(metric) {
    if (num_workers > 0) initialize_workers(num_workers);
}

QueryCoordinator::~QueryCoordinator() { shutdown_workers(); }

void QueryCoordinator::initialize_workers(int num_workers) {  // query_coordinator.cpp:50-74
    if (workers_initialized_) return;
    num_workers_ = num_workers;
    workers_initialized_ = num_workers > 0;
    // the reference starts one thread per worker and pins partition i to core i % num_workers; here the partitions move into a
    // device group (one member per worker, member j on GPU j % #GPUs) unless the manager was told the count before it was filled
    if (partition_manager_ && workers_initialized_) partition_manager_->distribute_partitions(num_workers);
}

void QueryCoordinator::shutdown_workers() {  // :77-95
    // the reference joins its threads and keeps serving scans serially; the partitions of a device group stay where they are
    // (they ARE the index) -- only the flag the reference's tests read goes down
    workers_initialized_ = false;
}

shared_ptr<SearchResult> QueryCoordinator::empty_result(shared_ptr<SearchParams> sp) const {  // :251-257, 476-482
    auto res = std::make_shared<SearchResult>();
    res->ids = torch::empty({0}, torch::kInt64);
    res->distances = torch::empty({0}, torch::kFloat32);
    res->timing_info = std::make_shared<SearchTimingInfo>();
    res->timing_info->search_params = sp;
    return res;
}

shared_ptr<SearchResult> QueryCoordinator::search(Tensor x, shared_ptr<SearchParams> sp) {  // :612-657
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::search] partition_manager_ is null.");
    if (!x.defined() || x.size(0) == 0) return empty_result(sp);
    auto t0 = clk::now();
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    qk_group *group = partition_manager_->group();  // partitions distributed over workers (GPUs)
    if (!store && !group) throw std::runtime_error("[QueryCoordinator::search] partitions are not initialized.");
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    // (workers: the parent search of the hit-tracking path runs on the shared context, the scan on the group's lead -- both are
    //  ordered on torch's stream)
    BoundToTorchStream bound(ctx, xq), bound_lead(group ? partition_manager_->search_ctx() : nullptr, xq);
    const int64_t Q = xq.size(0);
    const int k = sp->k > 0 ? sp->k : 1;  // :490
    const int nprobe = std::max(sp->nprobe, 1);
    auto res = std::make_shared<SearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_queries = Q;
    ti->n_clusters = partition_manager_->nlist();
    res->ids = torch::empty({Q, k}, torch::TensorOptions().dtype(torch::kInt64).device(xq.device()));
    res->distances = torch::empty({Q, k}, torch::TensorOptions().dtype(torch::kFloat32).device(xq.device()));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    const bool track = maintenance_policy_ && maintenance_policy_->track_hits_ && parent_;
    // per-call phase timing for SearchTimingInfo (mode 1: the library reads its events behind a synchronisation of the stream -- which
    // a call that asks for the counters of SearchTimingInfo performs anyway), for host and device tensors alike: the reference always
    // fills the phase fields (query_coordinator.cpp:612-657).  The caller's mode on the (shared, one per device) context is put back
    // on every way out.
    struct TimingMode {
        qk_ctx *c = nullptr;
        int was = 0;
        TimingMode(qk_ctx *ctx, bool want) {
            if (!want || qk_ctx_get_timing(ctx, &was) != QK_OK || was == 1) return;
            if (qk_ctx_set_timing(ctx, 1) == QK_OK) c = ctx;
        }
        ~TimingMode() {
            if (c) (void)qk_ctx_set_timing(c, was);
        }
    } timing_mode(ctx, !on_dev || device_timing_);
    qk_timing *tmp = (!on_dev || device_timing_) ? &tm : nullptr;  // device tensors: asynchronous unless the caller opted in
    if (sp->filters_exact_rows < 0 || sp->filters_exact_pool_rows < 0)
        throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters_exact_rows / filters_exact_pool_rows must not be "
                                 "negative (0 turns exact per-query filtered search off / leaves the pool unbounded)");
    if (sp->filters_exact_rows > 0) {
        // exact search with one filter per query (extension): the queries whose filter has at most filters_exact_rows candidates go
        // to qk_search_filtered_exact_batch with only those filters -- the others never enter the pool --, the rest go through
        // search() as they do today, and the two answers are scattered into one result
        if (sp->filter)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters_exact_rows is not supported with filter (one filter "
                                     "for every query: that is filter_exact_rows)");
        if (sp->filters.empty() || !sp->query_filter.defined())
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters_exact_rows needs filters and query_filter: without "
                                     "them every vector is a candidate");
        if (sp->recall_target > 0.0f)
            throw std::runtime_error("[QuakeIndex::search()] filters_exact_rows cannot be combined with recall_target > 0: "
                                     "not supported");
        if (group) throw std::runtime_error("[QuakeIndex::search()] filters_exact_rows is not supported with num_workers > 0");
        for (const auto &f : sp->filters)
            if (!f || !f->h) throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters must come from make_filter()");
        for (const auto &f : sp->filters)
            if (f->owner != store) throw std::runtime_error("[QuakeIndex::search()] the filter was made for another index");
        const Tensor &qf = sp->query_filter;
        const int64_t F = (int64_t)sp->filters.size();
        if (qf.dim() != 1 || qf.size(0) != Q)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.query_filter must have one entry per query (" +
                                     std::to_string(qf.dim() >= 1 ? qf.size(0) : 0) + " != " + std::to_string(Q) + ")");
        if (!qf.is_cuda() && qf.numel() > 0 && (qf.min().item<int64_t>() < 0 || qf.max().item<int64_t>() >= F))
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.query_filter holds a value outside [0, " + std::to_string(F) + ")");
        std::vector<qk_filter *> small;
        Tensor remap = torch::full({F}, -1, torch::kInt64);
        for (int64_t i = 0; i < F; i++) {
            int64_t rows = 0;  // (the count is cached per mask build)
            qk_check(qk_filter_candidate_rows(ctx, store, sp->filters[i]->h, &rows));
            if (rows <= sp->filters_exact_rows) {
                remap[i] = (int64_t)small.size();
                small.push_back(sp->filters[i]->h);
            }
        }
        // split where query_filter lives: a host tensor on the host, a device tensor with torch ops on the device (a device value
        // outside [0, F) stays with the probed call, which pads that row)
        Tensor ql = qf.to(torch::kInt64);
        Tensor slot = torch::where((ql >= 0) & (ql < F), remap.to(ql.device()).index_select(0, ql.clamp(0, F - 1)), torch::full_like(ql, -1));
        Tensor mask = slot >= 0;
        Tensor ie = torch::nonzero(mask).reshape({-1}), ip = torch::nonzero(~mask).reshape({-1});
        const auto xdev = xq.device();
        if (ie.numel() > 0) {
            // one enqueue, no partition probed: no hits for the policy
            Tensor xe = xq.index_select(0, ie.to(xdev)).contiguous();
            Tensor qe = slot.index_select(0, ie).to(xdev, torch::kInt32).contiguous();
            const int64_t Qe = xe.size(0);
            Tensor gi = torch::empty({Qe, k}, res->ids.options()), gd = torch::empty({Qe, k}, res->distances.options());
            qk_check(qk_search_filtered_exact_batch(ctx, store, xe.data_ptr<float>(), Qe, k, (int)metric_, small.data(), (int)small.size(),
                                                    qe.data_ptr<int32_t>(), sp->filters_exact_rows, sp->filters_exact_pool_rows,
                                                    gi.data_ptr<int64_t>(), gd.data_ptr<float>(), mem, nullptr));
            res->ids.index_copy_(0, ie.to(xdev), gi);
            res->distances.index_copy_(0, ie.to(xdev), gd);
        }
        if (ip.numel() > 0) {
            auto sp2 = std::make_shared<SearchParams>(*sp);
            sp2->filters_exact_rows = 0;
            sp2->query_filter = qf.index_select(0, ip);
            auto r2 = search(xq.index_select(0, ip.to(xdev)).contiguous(), sp2);
            res->ids.index_copy_(0, ip.to(xdev), r2->ids);
            res->distances.index_copy_(0, ip.to(xdev), r2->distances);
            ti->partitions_scanned = r2->timing_info->partitions_scanned;
            ti->parent_info = r2->timing_info->parent_info;
            if (r2->nprobed.defined()) {  // (adaptive probing: an exact query probed no partition)
                res->nprobed = torch::zeros({Q}, r2->nprobed.options());
                res->nprobed.index_copy_(0, ip.to(r2->nprobed.device()), r2->nprobed);
            }
        }
        res->exact = 0;  // (its meaning is the single-filter call's: this was not one)
        res->exact_mask = mask.to(xdev);
        ti->total_time_ns = ns_since(t0);
        return res;
    }
    if (sp->filter_exact_rows < 0)
        throw std::runtime_error("[QuakeIndex::search()] SearchParams.filter_exact_rows must not be negative (0 turns exact "
                                 "filtered search off)");
    if (sp->filter_exact_rows > 0) {
        // exact filtered search (extension): one filter, one device, no recall target; the rest is refused, not approximated
        if (!sp->filters.empty() || sp->query_filter.defined())
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.filter_exact_rows is not supported with filters / "
                                     "query_filter (one filter per query)");
        if (!sp->filter)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.filter_exact_rows needs a filter: without one every "
                                     "vector is a candidate");
        if (sp->recall_target > 0.0f)
            throw std::runtime_error("[QuakeIndex::search()] filter_exact_rows cannot be combined with recall_target > 0: "
                                     "not supported");
        if (group) throw std::runtime_error("[QuakeIndex::search()] filter_exact_rows is not supported with num_workers > 0");
    }
    qk_filter *flt = nullptr;
    if (sp->filter) {
        // filtered search (extension): the fixed-nprobe branch of one device; the rest is refused, not approximated
        if (sp->recall_target > 0.0f)
            throw std::runtime_error("[QuakeIndex::search()] a filter cannot be combined with recall_target > 0 "
                                     "(the recall model counts volume, not allowed rows): not supported");
        if (group) throw std::runtime_error("[QuakeIndex::search()] filtered search is not supported with num_workers > 0");
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::search()] SearchParams.filter must come from make_filter()");
        flt = sp->filter->h;
    }
    // one filter per query (extension): the same branch, the same refusals
    std::vector<qk_filter *> flts;
    Tensor qflt;
    if (!sp->filters.empty() || sp->query_filter.defined()) {
        if (sp->filter) throw std::runtime_error("[QuakeIndex::search()] SearchParams.filter and SearchParams.filters are exclusive");
        if (sp->filters.empty() || !sp->query_filter.defined())
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters and SearchParams.query_filter must be given together");
        for (const auto &f : sp->filters)
            if (!f || !f->h) throw std::runtime_error("[QuakeIndex::search()] SearchParams.filters must come from make_filter()");
        if (sp->recall_target > 0.0f)
            throw std::runtime_error("[QuakeIndex::search()] a filter cannot be combined with recall_target > 0 "
                                     "(the recall model counts volume, not allowed rows): not supported");
        if (group) throw std::runtime_error("[QuakeIndex::search()] filtered search is not supported with num_workers > 0");
        for (const auto &f : sp->filters)
            if (f->owner != store) throw std::runtime_error("[QuakeIndex::search()] the filter was made for another index");
        const Tensor &qf = sp->query_filter;
        if (qf.dim() != 1 || qf.size(0) != Q)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.query_filter must have one entry per query (" +
                                     std::to_string(qf.dim() >= 1 ? qf.size(0) : 0) + " != " + std::to_string(Q) + ")");
        if (!qf.is_cuda() && qf.numel() > 0 &&
            (qf.min().item<int64_t>() < 0 || qf.max().item<int64_t>() >= (int64_t)sp->filters.size()))
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.query_filter holds a value outside [0, " +
                                     std::to_string(sp->filters.size()) + ")");
        for (const auto &f : sp->filters) flts.push_back(f->h);
        qflt = qf.to(xq.device(), torch::kInt32).contiguous();
    }
    const int F = (int)flts.size();
    if (sp->max_nprobe > 0) {
        // adaptive probing under a filter (extension): the same branch, the same refusals
        if (!flt && !F)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.max_nprobe needs a filter (filter, or filters and "
                                     "query_filter): without one every probed row is a candidate");
        if (sp->recall_target > 0.0f)
            throw std::runtime_error("[QuakeIndex::search()] max_nprobe cannot be combined with recall_target > 0 "
                                     "(the recall model counts volume, not allowed rows): not supported");
        if (group) throw std::runtime_error("[QuakeIndex::search()] max_nprobe is not supported with num_workers > 0");
        if (sp->max_nprobe < nprobe)
            throw std::runtime_error("[QuakeIndex::search()] SearchParams.max_nprobe=" + std::to_string(sp->max_nprobe) +
                                     " is below nprobe=" + std::to_string(nprobe) + " (0 turns adaptive probing off)");
    }
    const bool adaptive = sp->max_nprobe > nprobe && parent_;  // (a flat index scans everything: nothing to adapt)
    if (sp->filter_exact_rows > 0) {
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::search()] the filter was made for another index");
        int64_t rows = 0;
        qk_check(qk_filter_candidate_rows(ctx, store, flt, &rows));
        res->exact = rows <= sp->filter_exact_rows ? 1 : 0;
    }
    if (res->exact == 1) {
        // the flat search of the filter's candidate rows: no parent, no nprobe, no hits for the policy
        qk_check(qk_search_filtered_exact(ctx, store, xq.data_ptr<float>(), Q, k, (int)metric_, flt, sp->filter_exact_rows,
                                          res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, tmp));
        ti->partitions_scanned = (int)tm.partitions_scanned;  // (as this mirror's search of a flat index reports it: one per query)
        ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
        ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
        ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
        ti->total_time_ns = ns_since(t0);
        return res;
    }
    if (adaptive) {
        // one enqueue: coarse step at max_nprobe, the cut of every query's row on the device, the filtered scan
        const int M = (int)std::min<int64_t>(sp->max_nprobe, parent_->ntotal());
        const auto dev = torch::TensorOptions().device(xq.device());
        res->nprobed = torch::empty({Q}, dev.dtype(torch::kInt32));
        Tensor pids;
        if (track) pids = torch::empty({Q, std::max(M, 1)}, dev.dtype(torch::kInt64));
        qk_filter *one[1] = {flt};
        qk_check(qk_search_filtered_adaptive(ctx, parent_->store(), store, xq.data_ptr<float>(), Q, nprobe, sp->max_nprobe,
                                             sp->filter_min_candidates > 0 ? sp->filter_min_candidates : (int64_t)k, k, (int)metric_,
                                             F ? flts.data() : one, F ? F : 1, F ? qflt.data_ptr<int32_t>() : nullptr,
                                             res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(),
                                             res->nprobed.data_ptr<int32_t>(), track ? pids.data_ptr<int64_t>() : nullptr, mem, tmp));
        if (track) {  // (the rows end in -1: record_query_batch skips those)
            if (M < 1) pids = pids.slice(1, 0, 0);
            maintenance_policy_->record_query_batch_later(pids);
        }
        ti->partitions_scanned = (int)tm.partitions_scanned;
        ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
        ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
        ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    } else if (sp->recall_target > 0.0f && parent_ && !sp->batched_scan) {
        // adaptive partition scanning (:502,637-641): candidates = nlist * initial_search_fraction; with workers the rounds run on
        // the group's lead and every member scans the pairs whose partitions it holds (the APS hook of worker_scan, :364-428)
        Tensor nscan = torch::empty({Q}, torch::TensorOptions().dtype(torch::kInt32).device(xq.device()));
        if (group)
            qk_check(qk_group_search_aps(group, parent_->store(), xq.data_ptr<float>(), Q, k, (int)metric_, sp->recall_target,
                                         sp->recompute_threshold, sp->use_precomputed ? 1 : 0, sp->initial_search_fraction,
                                         res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), nscan.data_ptr<int32_t>(), mem, &tm));
        else
            qk_check(qk_search_aps(ctx, parent_->store(), store, xq.data_ptr<float>(), Q, k, (int)metric_, sp->recall_target,
                                   sp->recompute_threshold, sp->use_precomputed ? 1 : 0, sp->initial_search_fraction,
                                   res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), nscan.data_ptr<int32_t>(), mem, &tm));
        ti->partitions_scanned = (int)nscan.sum().item<int64_t>();
        ti->job_wait_time_ns = (int64_t)(tm.total_ms * 1e6);
    } else if (track) {
        // hit tracking on: the probed lists go to the policy.  One store: qk_search_tracked (the nearest-centroid step writes `pids`, the
        // scan reads it, one enqueue); a group: the coarse step on the shared context, then the members' scan
        const int kk = (int)std::min<int64_t>(nprobe, parent_->ntotal());
        Tensor pids = torch::empty({Q, std::max(kk, 1)}, torch::TensorOptions().dtype(torch::kInt64).device(xq.device()));
        if (group) {
            qk_check(qk_coarse(ctx, parent_->store(), xq.data_ptr<float>(), Q, nprobe, (int)metric_, pids.data_ptr<int64_t>(), nullptr, mem));
            qk_check(qk_group_scan(group, xq.data_ptr<float>(), Q, pids.data_ptr<int64_t>(), kk, k, (int)metric_,
                                   res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, &tm));
        } else if (F) {
            qk_check(qk_search_filtered_batch_tracked(ctx, parent_->store(), store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                                                      flts.data(), F, qflt.data_ptr<int32_t>(), res->ids.data_ptr<int64_t>(),
                                                      res->distances.data_ptr<float>(), pids.data_ptr<int64_t>(), mem, &tm));
        } else if (flt) {  // (the probed lists are the unfiltered search's: the policy sees the same hits)
            qk_check(qk_search_filtered_tracked(ctx, parent_->store(), store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_, flt,
                                                res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), pids.data_ptr<int64_t>(), mem, &tm));
        } else {
            qk_check(qk_search_tracked(ctx, parent_->store(), store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                                       res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), pids.data_ptr<int64_t>(), mem, &tm));
        }
        if (kk < 1) pids = pids.slice(1, 0, 0);
        maintenance_policy_->record_query_batch_later(pids);  // (recorded before the next modification / maintenance: flush_hits)
        ti->partitions_scanned = (int)tm.partitions_scanned;
        ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
        ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
        ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    } else if (group) {  // workers: every member scans the partitions it holds (worker_scan, :243-469), the lead merges
        qk_check(qk_group_search(group, parent_->store(), xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                                 res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, tmp));
        ti->partitions_scanned = (int)tm.partitions_scanned;
        ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
        ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    } else {
        if (F)
            qk_check(qk_search_filtered_batch(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k,
                                              (int)metric_, flts.data(), F, qflt.data_ptr<int32_t>(), res->ids.data_ptr<int64_t>(),
                                              res->distances.data_ptr<float>(), mem, tmp));
        else if (flt)
            qk_check(qk_search_filtered(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                                        flt, res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, tmp));
        else
            qk_check(qk_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                               res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, tmp));
        ti->partitions_scanned = (int)tm.partitions_scanned;
        ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
        ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
        ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    }
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<SearchResult> QueryCoordinator::search_after(Tensor x, shared_ptr<SearchParams> sp, shared_ptr<SearchCursor> cursor) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::search_after] partition_manager_ is null.");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::search_after()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by search_after");
    if (sp->max_nprobe > 0)
        throw std::runtime_error("[QuakeIndex::search_after()] SearchParams.max_nprobe (adaptive probing) is not supported by "
                                 "search_after: a page is defined over a fixed set of probed partitions");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::search_after()] SearchParams.filters_exact_rows (exact per-query filtered search) is not "
                                 "supported by search_after");
    if (sp->filter_exact_rows > 0)
        throw std::runtime_error("[QuakeIndex::search_after()] SearchParams.filter_exact_rows (exact filtered search) is not supported by "
                                 "search_after");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::search_after()] search_after is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::search_after()] search_after is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::search_after] partitions are not initialized.");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::search_after()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::search_after()] the filter was made for another index");
        flt = sp->filter->h;
    }
    const int k = sp->k > 0 ? sp->k : 1;
    if (k > QK_MAX_K)
        throw std::runtime_error("[QuakeIndex::search_after()] k=" + std::to_string(k) + " exceeds the page limit of " + std::to_string(QK_MAX_K) +
                                 ": ask for the rest with the next cursor");
    const int64_t Q = x.defined() ? x.size(0) : 0;
    if (cursor) {
        if (!cursor->keys.defined() || !cursor->ids.defined())
            throw std::runtime_error("[QuakeIndex::search_after()] cursor must be the SearchCursor of an earlier page (keys and ids)");
        if (cursor->keys.numel() != Q || cursor->ids.numel() != Q)
            throw std::runtime_error("[QuakeIndex::search_after()] the cursor has " + std::to_string(cursor->keys.numel()) + " / " +
                                     std::to_string(cursor->ids.numel()) + " entries for " + std::to_string(Q) + " queries");
    }
    auto res = std::make_shared<SearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    res->cursor = std::make_shared<SearchCursor>();
    if (Q == 0) {
        res->ids = torch::empty({0}, torch::kInt64);
        res->distances = torch::empty({0}, torch::kFloat32);
        res->cursor->keys = torch::empty({0}, torch::kInt32);
        res->cursor->ids = torch::empty({0}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto opt = [&](torch::ScalarType t) { return torch::TensorOptions().dtype(t).device(xq.device()); };
    res->ids = torch::empty({Q, (int64_t)k}, opt(torch::kInt64));
    res->distances = torch::empty({Q, (int64_t)k}, opt(torch::kFloat32));
    res->cursor->keys = torch::empty({Q}, opt(torch::kInt32));
    res->cursor->ids = torch::empty({Q}, opt(torch::kInt64));
    Tensor ak, ai;  // the caller's cursor in the queries' memory space
    if (cursor) {
        ak = cursor->keys.reshape({Q}).to(opt(torch::kInt32)).contiguous();
        ai = cursor->ids.reshape({Q}).to(opt(torch::kInt64)).contiguous();
    }
    qk_check(qk_search_after(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_,
                             cursor ? (const uint32_t *)ak.data_ptr<int32_t>() : nullptr, cursor ? ai.data_ptr<int64_t>() : nullptr, flt,
                             res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), (uint32_t *)res->cursor->keys.data_ptr<int32_t>(),
                             res->cursor->ids.data_ptr<int64_t>(), mem, &tm));
    ti->partitions_scanned = (int)tm.partitions_scanned;
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<RangeSearchResult> QueryCoordinator::range_search(Tensor x, float radius, shared_ptr<SearchParams> sp) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::range_search] partition_manager_ is null.");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::range_search()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by range_search");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::range_search()] SearchParams.filters_exact_rows (exact per-query filtered search) is not "
                                 "supported by range_search");
    if (sp->filter_exact_rows > 0)
        throw std::runtime_error("[QuakeIndex::range_search()] SearchParams.filter_exact_rows (exact filtered search) is not supported by "
                                 "range_search");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::range_search()] range_search is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::range_search()] range_search is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::range_search] partitions are not initialized.");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::range_search()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::range_search()] the filter was made for another index");
        flt = sp->filter->h;
    }
    auto res = std::make_shared<RangeSearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        res->lims = torch::zeros({1}, torch::kInt64);
        res->ids = torch::empty({0}, torch::kInt64);
        res->distances = torch::empty({0}, torch::kFloat32);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(xq.device());
    res->lims = torch::empty({Q + 1}, i64);
    // the capacity protocol: a guess, then one more call only if lims[Q] says it was short (lims is exact either way)
    int64_t cap = std::max<int64_t>(4096, 64 * Q), total = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        res->ids = torch::empty({cap}, i64);
        res->distances = torch::empty({cap}, f32);
        qk_check(qk_range_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, (int)metric_, radius, flt,
                                 cap, res->lims.data_ptr<int64_t>(), res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), mem, &tm));
        total = res->lims[Q].item<int64_t>();  // (a timed call has synchronised the stream)
        if (total <= cap) break;
        cap = total;
    }
    res->ids = res->ids.slice(0, 0, total);
    res->distances = res->distances.slice(0, 0, total);
    ti->partitions_scanned = (int)tm.partitions_scanned;
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<GroupedSearchResult> QueryCoordinator::grouped_search(Tensor x, qk_attr *group_by, const std::string &name, shared_ptr<SearchParams> sp,
                                                                 std::optional<int> group_size) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::grouped_search] partition_manager_ is null.");
    if (group_size && (*group_size < 1 || *group_size > QK_MAX_GROUP_SIZE))
        throw std::runtime_error("[QuakeIndex::grouped_search()] group_size must be between 1 and " + std::to_string(QK_MAX_GROUP_SIZE));
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::grouped_search()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by grouped_search");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::grouped_search()] SearchParams.filters_exact_rows (exact per-query filtered search) is not "
                                 "supported by grouped_search");
    if (sp->filter_exact_rows > 0)
        throw std::runtime_error("[QuakeIndex::grouped_search()] SearchParams.filter_exact_rows (exact filtered search) is not supported by "
                                 "grouped_search");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::grouped_search()] grouped_search is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::grouped_search()] grouped_search is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::grouped_search] partitions are not initialized.");
    if (!group_by) throw std::runtime_error("[QuakeIndex::grouped_search()] unknown attribute column '" + name + "'");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::grouped_search()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::grouped_search()] the filter was made for another index");
        flt = sp->filter->h;
    }
    const int k = sp->k > 0 ? sp->k : 1;
    // group_size unset: the one-row shapes [Q, k]; m: ids / distances [Q, k, m]
    auto shape = [&](int64_t q) { return group_size ? std::vector<int64_t>{q, k, *group_size} : std::vector<int64_t>{q, k}; };
    auto res = std::make_shared<GroupedSearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        res->ids = torch::empty(shape(0), torch::kInt64);
        res->distances = torch::empty(shape(0), torch::kFloat32);
        res->groups = torch::empty({0, k}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(xq.device());
    res->ids = torch::empty(shape(Q), i64);
    res->distances = torch::empty(shape(Q), f32);
    res->groups = torch::empty({Q, k}, i64);
    if (group_size)
        qk_check(qk_search_grouped_n(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k, *group_size, (int)metric_,
                                     group_by, flt, res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), res->groups.data_ptr<int64_t>(),
                                     mem, &tm));
    else
        qk_check(qk_search_grouped(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, k, (int)metric_, group_by, flt,
                                   res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), res->groups.data_ptr<int64_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<FacetResult> QueryCoordinator::facet_counts(Tensor x, const std::vector<qk_attr *> &cols, const std::vector<std::string> &names,
                                                       shared_ptr<SearchParams> sp, std::optional<float> radius_opt, int n_values) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::facet_counts] partition_manager_ is null.");
    if (names.size() < 1 || names.size() > QK_MAX_FACET_COLS)
        throw std::runtime_error("[QuakeIndex::facet_counts()] facet_by must name between 1 and " + std::to_string(QK_MAX_FACET_COLS) + " columns");
    if (n_values < 1 || n_values > QK_MAX_FACET_VALUES)
        throw std::runtime_error("[QuakeIndex::facet_counts()] n_values must be between 1 and " + std::to_string(QK_MAX_FACET_VALUES));
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::facet_counts()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by facet_counts");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::facet_counts()] SearchParams.filters_exact_rows (exact per-query filtered search) is not "
                                 "supported by facet_counts");
    if (sp->filter_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::facet_counts()] SearchParams.filter_exact_rows (exact filtered search) is not supported by "
                                 "facet_counts");
    if (sp->max_nprobe > 0)
        throw std::runtime_error("[QuakeIndex::facet_counts()] SearchParams.max_nprobe (adaptive probing) is not supported by facet_counts");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::facet_counts()] facet_counts is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::facet_counts()] facet_counts is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::facet_counts] partitions are not initialized.");
    for (size_t c = 0; c < names.size(); c++)
        if (!cols[c]) throw std::runtime_error("[QuakeIndex::facet_counts()] unknown attribute column '" + names[c] + "'");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::facet_counts()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::facet_counts()] the filter was made for another index");
        flt = sp->filter->h;
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float radius = radius_opt ? *radius_opt : ((int)metric_ == QK_METRIC_IP ? -inf : inf);
    if (radius != radius) throw std::runtime_error("[QuakeIndex::facet_counts()] the radius is NaN");
    const int64_t C = (int64_t)names.size();
    auto res = std::make_shared<FacetResult>();
    res->columns = names;
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        res->values = torch::zeros({C, 0, n_values}, torch::kInt64);
        res->counts = torch::zeros({C, 0, n_values}, torch::kInt64);
        res->distinct = torch::zeros({C, 0}, torch::kInt64);
        res->missing = torch::zeros({C, 0}, torch::kInt64);
        res->totals = torch::zeros({0}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    res->values = torch::empty({C, Q, n_values}, i64);
    res->counts = torch::empty({C, Q, n_values}, i64);
    res->distinct = torch::empty({C, Q}, i64);
    res->missing = torch::empty({C, Q}, i64);
    res->totals = torch::empty({Q}, i64);
    qk_check(qk_facet_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, (int)metric_, radius, flt,
                             cols.data(), (int)C, n_values, res->values.data_ptr<int64_t>(), res->counts.data_ptr<int64_t>(),
                             res->distinct.data_ptr<int64_t>(), res->missing.data_ptr<int64_t>(), res->totals.data_ptr<int64_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<FacetStatsResult> QueryCoordinator::facet_stats(Tensor x, const std::vector<qk_attr *> &cols, const std::vector<std::string> &names,
                                                          shared_ptr<SearchParams> sp, std::optional<float> radius_opt,
                                                          const FacetEdgesFn &edges_fn) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::facet_stats] partition_manager_ is null.");
    if (names.size() < 1 || names.size() > QK_MAX_FACET_COLS)
        throw std::runtime_error("[QuakeIndex::facet_stats()] facet_by must name between 1 and " + std::to_string(QK_MAX_FACET_COLS) + " columns");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::facet_stats()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by facet_stats");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::facet_stats()] SearchParams.filters_exact_rows (exact per-query filtered search) is not "
                                 "supported by facet_stats");
    if (sp->filter_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::facet_stats()] SearchParams.filter_exact_rows (exact filtered search) is not supported by "
                                 "facet_stats");
    if (sp->max_nprobe > 0)
        throw std::runtime_error("[QuakeIndex::facet_stats()] SearchParams.max_nprobe (adaptive probing) is not supported by facet_stats");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::facet_stats()] facet_stats is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::facet_stats()] facet_stats is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::facet_stats] partitions are not initialized.");
    for (size_t c = 0; c < names.size(); c++)
        if (!cols[c]) throw std::runtime_error("[QuakeIndex::facet_stats()] unknown attribute column '" + names[c] + "'");
    const std::vector<std::vector<int64_t>> edges = edges_fn();  // (here, as in the Python mirror: an edge error comes behind these)
    if (edges.size() != names.size()) throw std::runtime_error("[QuakeIndex::facet_stats()] edges needs one list per facet column");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::facet_stats()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::facet_stats()] the filter was made for another index");
        flt = sp->filter->h;
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float radius = radius_opt ? *radius_opt : ((int)metric_ == QK_METRIC_IP ? -inf : inf);
    if (radius != radius) throw std::runtime_error("[QuakeIndex::facet_stats()] the radius is NaN");
    const int64_t C = (int64_t)names.size();
    std::vector<int64_t> flat;
    std::vector<int> n_edges;
    int64_t hs = 1;
    for (int64_t c = 0; c < C; c++) {
        const std::vector<int64_t> &e = edges[c];
        flat.insert(flat.end(), e.begin(), e.end());
        n_edges.push_back((int)e.size());
        hs = std::max<int64_t>(hs, 1 + (int64_t)e.size());
    }
    auto res = std::make_shared<FacetStatsResult>();
    res->columns = names;
    res->edges = edges;
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        for (Tensor *t : {&res->count, &res->missing, &res->min, &res->max, &res->sum_lo, &res->sum_hi}) *t = torch::zeros({C, 0}, torch::kInt64);
        res->histogram = torch::zeros({C, 0, hs}, torch::kInt64);
        res->totals = torch::zeros({0}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    for (Tensor *t : {&res->count, &res->missing, &res->min, &res->max, &res->sum_lo, &res->sum_hi}) *t = torch::empty({C, Q}, i64);
    res->histogram = torch::empty({C, Q, hs}, i64);
    res->totals = torch::empty({Q}, i64);
    qk_check(qk_facet_stats_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, (int)metric_, radius, flt,
                                   cols.data(), (int)C, flat.data(), n_edges.data(), res->count.data_ptr<int64_t>(),
                                   res->missing.data_ptr<int64_t>(), res->min.data_ptr<int64_t>(), res->max.data_ptr<int64_t>(),
                                   res->sum_lo.data_ptr<int64_t>(), res->sum_hi.data_ptr<int64_t>(), res->histogram.data_ptr<int64_t>(),
                                   res->totals.data_ptr<int64_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<OrderedSearchResult> QueryCoordinator::ordered_search(Tensor x, qk_attr *col, const std::vector<std::string> &known,
                                                                const std::string &order_by, shared_ptr<SearchParams> sp,
                                                                std::optional<float> radius_opt, bool descending, const std::string &missing) {
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::ordered_search] partition_manager_ is null.");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error("[QuakeIndex::ordered_search()] SearchParams.filters / query_filter (one filter per query) are not "
                                 "supported by ordered_search");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::ordered_search()] SearchParams.filters_exact_rows (exact per-query filtered search) is "
                                 "not supported by ordered_search");
    if (sp->filter_exact_rows != 0)
        throw std::runtime_error("[QuakeIndex::ordered_search()] SearchParams.filter_exact_rows (exact filtered search) is not supported "
                                 "by ordered_search");
    if (sp->max_nprobe > 0)
        throw std::runtime_error("[QuakeIndex::ordered_search()] SearchParams.max_nprobe (adaptive probing) is not supported by "
                                 "ordered_search");
    if (sp->recall_target > 0.0f) throw std::runtime_error("[QuakeIndex::ordered_search()] ordered_search is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error("[QuakeIndex::ordered_search()] ordered_search is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::ordered_search] partitions are not initialized.");
    const int flags = lower_order(known, order_by, sp->k, descending, missing);
    const int64_t k = sp->k;
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error("[QuakeIndex::ordered_search()] SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error("[QuakeIndex::ordered_search()] the filter was made for another index");
        flt = sp->filter->h;
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float radius = radius_opt ? *radius_opt : ((int)metric_ == QK_METRIC_IP ? -inf : inf);
    if (radius != radius) throw std::runtime_error("[QuakeIndex::ordered_search()] the radius is NaN");
    auto res = std::make_shared<OrderedSearchResult>();
    res->column = order_by;
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        res->ids = torch::zeros({0, k}, torch::kInt64);
        res->distances = torch::zeros({0, k}, torch::kFloat32);
        res->values = torch::zeros({0, k}, torch::kInt64);
        for (Tensor *t : {&res->counts, &res->missing, &res->totals}) *t = torch::zeros({0}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    res->ids = torch::empty({Q, k}, i64);
    res->distances = torch::empty({Q, k}, i64.dtype(torch::kFloat32));
    res->values = torch::empty({Q, k}, i64);
    for (Tensor *t : {&res->counts, &res->missing, &res->totals}) *t = torch::empty({Q}, i64);
    qk_check(qk_order_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, (int)metric_, radius, flt, col,
                             flags, (int)k, res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), res->values.data_ptr<int64_t>(),
                             res->counts.data_ptr<int64_t>(), res->missing.data_ptr<int64_t>(), res->totals.data_ptr<int64_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<MultiVectorSearchResult> QueryCoordinator::multi_vector_search(Tensor x, qk_attr *col, const std::vector<std::string> &known,
                                                                          const std::string &group_by, shared_ptr<SearchParams> sp,
                                                                          std::optional<float> radius_opt,
                                                                          const std::optional<std::vector<int64_t>> &n_tokens,
                                                                          std::optional<double> missing_opt) {
    const std::string who = "[QuakeIndex::multi_vector_search()]";
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::multi_vector_search] partition_manager_ is null.");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error(who + " SearchParams.filters / query_filter (one filter per query) are not supported by "
                                       "multi_vector_search");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error(who + " SearchParams.filters_exact_rows (exact per-query filtered search) is not supported by "
                                       "multi_vector_search");
    if (sp->filter_exact_rows != 0)
        throw std::runtime_error(who + " SearchParams.filter_exact_rows (exact filtered search) is not supported by multi_vector_search");
    if (sp->max_nprobe > 0)
        throw std::runtime_error(who + " SearchParams.max_nprobe (adaptive probing) is not supported by multi_vector_search");
    if (sp->recall_target > 0.0f) throw std::runtime_error(who + " multi_vector_search is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error(who + " multi_vector_search is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::multi_vector_search] partitions are not initialized.");
    if (!x.defined() || x.dim() != 3) throw std::runtime_error(who + " x must be [L, T, d]");
    const int64_t L = x.size(0), T = x.size(1), k = sp->k;
    const float missing = (float)lower_maxsim(known, group_by, k, T, n_tokens, missing_opt, (int)metric_ == QK_METRIC_IP);
    if (n_tokens && (int64_t)n_tokens->size() != L)
        throw std::runtime_error(who + " n_tokens has " + std::to_string(n_tokens->size()) + " entries for " + std::to_string(L) + " queries");
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error(who + " SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error(who + " the filter was made for another index");
        flt = sp->filter->h;
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float radius = radius_opt ? *radius_opt : ((int)metric_ == QK_METRIC_IP ? -inf : inf);
    if (radius != radius) throw std::runtime_error(who + " the radius is NaN");
    auto res = std::make_shared<MultiVectorSearchResult>();
    res->column = group_by;
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (L == 0) {
        res->groups = torch::zeros({0, k}, torch::kInt64);
        res->scores = torch::zeros({0, k}, torch::kFloat32);
        res->matched = torch::zeros({0, k}, torch::kInt32);
        res->n_groups = torch::zeros({0}, torch::kInt64);
        res->hits = torch::zeros({0, T}, torch::kInt64);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = (on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x)).reshape({L * T, x.size(2)});
    BoundToTorchStream bound(ctx, xq);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = L;
    Tensor nt;  // int32 [L] in x's memory
    if (n_tokens) {
        nt = torch::empty({L}, torch::kInt32);
        for (int64_t l = 0; l < L; l++) nt.data_ptr<int32_t>()[l] = (int32_t)(*n_tokens)[l];
        if (on_dev) nt = nt.to(xq.device());
    }
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    res->groups = torch::empty({L, k}, i64);
    res->scores = torch::empty({L, k}, i64.dtype(torch::kFloat32));
    res->matched = torch::empty({L, k}, i64.dtype(torch::kInt32));
    res->n_groups = torch::empty({L}, i64);
    res->hits = torch::empty({L, T}, i64);
    qk_check(qk_maxsim_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), L, (int)T,
                              nt.defined() ? nt.data_ptr<int32_t>() : nullptr, nprobe, (int)metric_, radius, flt, col, missing, (int)k,
                              res->groups.data_ptr<int64_t>(), res->scores.data_ptr<float>(), res->matched.data_ptr<int32_t>(),
                              res->n_groups.data_ptr<int64_t>(), res->hits.data_ptr<int64_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = L;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<DiverseSearchResult> QueryCoordinator::diverse_search(Tensor x, shared_ptr<SearchParams> sp, int64_t fetch_k, double lambda_mult) {
    const std::string who = "[QuakeIndex::diverse_search()]";
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::diverse_search] partition_manager_ is null.");
    if (!sp->filters.empty() || sp->query_filter.defined())
        throw std::runtime_error(who + " SearchParams.filters / query_filter (one filter per query) are not supported by diverse_search");
    if (sp->filters_exact_rows != 0)
        throw std::runtime_error(who + " SearchParams.filters_exact_rows (exact per-query filtered search) is not supported by "
                                       "diverse_search");
    if (sp->filter_exact_rows != 0)
        throw std::runtime_error(who + " SearchParams.filter_exact_rows (exact filtered search) is not supported by diverse_search");
    if (sp->max_nprobe > 0) throw std::runtime_error(who + " SearchParams.max_nprobe (adaptive probing) is not supported by diverse_search");
    if (sp->recall_target > 0.0f) throw std::runtime_error(who + " diverse_search is not supported with recall_target > 0");
    qk_ctx *ctx = partition_manager_->ctx();
    qk_store *store = partition_manager_->store();
    if (partition_manager_->group()) throw std::runtime_error(who + " diverse_search is not supported with num_workers > 0");
    if (!store) throw std::runtime_error("[QueryCoordinator::diverse_search] partitions are not initialized.");
    const float lambda = lower_diverse(sp->k, fetch_k, lambda_mult);
    const int64_t k = sp->k;
    qk_filter *flt = nullptr;
    if (sp->filter) {
        if (!sp->filter->h) throw std::runtime_error(who + " SearchParams.filter must come from make_filter()");
        if (sp->filter->owner != store) throw std::runtime_error(who + " the filter was made for another index");
        flt = sp->filter->h;
    }
    auto res = std::make_shared<DiverseSearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_clusters = partition_manager_->nlist();
    if (!x.defined() || x.size(0) == 0) {
        res->ids = torch::zeros({0, k}, torch::kInt64);
        res->distances = torch::zeros({0, k}, torch::kFloat32);
        res->ranks = torch::zeros({0, k}, torch::kInt32);
        return res;
    }
    auto t0 = clk::now();
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(ctx, xq);
    const int64_t Q = xq.size(0);
    const int nprobe = std::max(sp->nprobe, 1);
    const int mem = on_dev ? QK_MEM_DEVICE : QK_MEM_HOST;
    ti->n_queries = Q;
    int was = 0;
    qk_check(qk_ctx_get_timing(ctx, &was));
    struct Restore {
        qk_ctx *c;
        int was;
        ~Restore() { (void)qk_ctx_set_timing(c, was); }
    } restore{ctx, was};
    qk_check(qk_ctx_set_timing(ctx, 1));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    auto i64 = torch::TensorOptions().dtype(torch::kInt64).device(xq.device());
    res->ids = torch::empty({Q, k}, i64);
    res->distances = torch::empty({Q, k}, i64.dtype(torch::kFloat32));
    res->ranks = torch::empty({Q, k}, i64.dtype(torch::kInt32));
    qk_check(qk_diverse_search(ctx, parent_ ? parent_->store() : nullptr, store, xq.data_ptr<float>(), Q, nprobe, (int)k, (int)fetch_k, lambda,
                               (int)metric_, flt, res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(),
                               res->ranks.data_ptr<int32_t>(), mem, &tm));
    ti->job_enqueue_time_ns = (int64_t)(tm.group_ms * 1e6);
    ti->job_wait_time_ns = (int64_t)(tm.scan_ms * 1e6);
    ti->result_aggregate_time_ns = (int64_t)(tm.merge_ms * 1e6);
    if (parent_) {
        ti->parent_info = std::make_shared<SearchTimingInfo>();
        ti->parent_info->n_queries = Q;
        ti->parent_info->n_clusters = 1;
        ti->parent_info->total_time_ns = (int64_t)(tm.coarse_ms * 1e6);
    }
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<SearchResult> QueryCoordinator::scan_partitions(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> sp) {  // :659-673
    if (!partition_manager_) throw std::runtime_error("[QueryCoordinator::scan_partitions] partition_manager_ is null.");
    if (!x.defined() || x.size(0) == 0) return empty_result(sp);
    auto t0 = clk::now();
    qk_store *store = partition_manager_->store();
    qk_group *group = partition_manager_->group();
    if (!store && !group) throw std::runtime_error("[QueryCoordinator::scan_partitions] partitions are not initialized.");
    // device queries stay on the device (the list numbers follow them there), host queries go through the staging buffers
    const bool on_dev = x.is_cuda();
    Tensor xq = on_dev ? x.to(torch::kFloat32).contiguous() : host_f32(x);
    BoundToTorchStream bound(partition_manager_->search_ctx(), xq);
    const int64_t Q = xq.size(0);
    const int k = sp->k > 0 ? sp->k : 1;
    Tensor pids = on_dev ? partition_ids.to(xq.device(), torch::kInt64).contiguous() : host_i64(partition_ids);
    if (pids.dim() == 1) pids = pids.unsqueeze(0).expand({Q, pids.size(0)}).contiguous();  // the same set for every query (:506-508)
    const int P = (int)pids.size(1);
    auto res = std::make_shared<SearchResult>();
    auto ti = res->timing_info = std::make_shared<SearchTimingInfo>();
    ti->search_params = sp;
    ti->n_queries = Q;
    ti->n_clusters = partition_manager_->nlist();
    res->ids = torch::empty({Q, k}, torch::TensorOptions().dtype(torch::kInt64).device(xq.device()));
    res->distances = torch::empty({Q, k}, torch::TensorOptions().dtype(torch::kFloat32).device(xq.device()));
    qk_timing tm;
    std::memset(&tm, 0, sizeof(tm));
    Tensor none = torch::full({Q, 1}, -1, torch::TensorOptions().dtype(torch::kInt64).device(xq.device()));  // zero partitions: padded output (:459-497)
    const Tensor &pp = P > 0 ? pids : none;
    qk_timing *tmp = (!on_dev || device_timing_) ? &tm : nullptr;  // (as in search: device tensors stay asynchronous)
    if (group)
        qk_check(qk_group_scan(group, xq.data_ptr<float>(), Q, pp.data_ptr<int64_t>(), (int)pp.size(1), k, (int)metric_,
                               res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), on_dev ? QK_MEM_DEVICE : QK_MEM_HOST, tmp));
    else
        qk_check(qk_scan(partition_manager_->ctx(), store, xq.data_ptr<float>(), Q, pp.data_ptr<int64_t>(), (int)pp.size(1), k, (int)metric_,
                         res->ids.data_ptr<int64_t>(), res->distances.data_ptr<float>(), on_dev ? QK_MEM_DEVICE : QK_MEM_HOST, tmp));
    ti->partitions_scanned = (int)tm.partitions_scanned;
    ti->total_time_ns = ns_since(t0);
    return res;
}

shared_ptr<SearchResult> QueryCoordinator::serial_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> sp) {
    return scan_partitions(x, partition_ids, sp);
}
shared_ptr<SearchResult> QueryCoordinator::batched_serial_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> sp) {
    return scan_partitions(x, partition_ids, sp);
}
shared_ptr<SearchResult> QueryCoordinator::worker_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> sp) {
    return scan_partitions(x, partition_ids, sp);
}

}  // namespace quake_amd
