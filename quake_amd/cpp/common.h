// common.h -- parameter / result records of the C++ host mirror: the names, fields and defaults of the reference's
// src/cpp/include/common.h:66-276 (IndexBuildParams, SearchParams, *TimingInfo, SearchResult, Clustering, str_to_metric_type),
// so that C++ callers and the pybind11 module see the records they know.  No arithmetic here.
#pragma once
#include <torch/torch.h>

#include <functional>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../../include/quake_hip.h"

using torch::Tensor;
using std::shared_ptr;

namespace quake_amd {

// faiss::MetricType's two values the reference uses (common.h:145-156); the numeric codes are the C ABI's
enum MetricType { METRIC_INNER_PRODUCT = QK_METRIC_IP, METRIC_L2 = QK_METRIC_L2 };

constexpr int DEFAULT_NLIST = 0, DEFAULT_NITER = 5, DEFAULT_NUM_WORKERS = 0, DEFAULT_K = 1, DEFAULT_NPROBE = 1;
constexpr const char *DEFAULT_METRIC = "l2";
constexpr float DEFAULT_RECALL_TARGET = -1.0f;

struct MaintenancePolicyParams {  // common.h:104-118
    std::string maintenance_policy = "query_cost";
    int window_size = 1000;
    int refinement_radius = 25;
    int refinement_iterations = 3;
    int min_partition_size = 32;
    float alpha = 0.9f;
    bool enable_split_rejection = true;
    bool enable_delete_rejection = true;
    float delete_threshold_ns = 10.0f;
    float split_threshold_ns = 10.0f;
    // EXTENSION (no reference field): a partition the delete branch examined and the rejection rule KEPT is then tested for a split
    // like every other kept partition.  The reference (maintenance_policies.cpp:68-131) never reaches its split test for such a
    // partition -- and its delete model is most negative for the partitions that are both larger and hotter than average, so the
    // lists a skewed insert stream grows are never split.  false = the reference's decisions.
    bool split_after_delete_rejection = false;
};

struct IndexBuildParams {  // common.h:123-143
    int dimension = 0;
    int nlist = DEFAULT_NLIST;
    int num_workers = DEFAULT_NUM_WORKERS;
    int code_size = -1;
    int num_codebooks = -1;
    std::string metric = DEFAULT_METRIC;
    int niter = DEFAULT_NITER;
    bool use_adaptive_nprobe = false;
    bool use_numa = false;
    bool use_gpu = true;  // GPU k-means is the only k-means here
    bool verify_numa = false;
    bool same_core = true;
    bool verbose = false;
    shared_ptr<IndexBuildParams> parent_params = nullptr;
};

// extension (no reference counterpart): a set of vector ids of ONE index and a mode, made by QuakeIndex::make_filter -- with
// exclude == false a stored vector is a candidate iff its id is in the set, with exclude == true iff it is not (qk_filter).
// Defined by ids: it stays valid while the index changes.  Not persisted by save().
struct SearchFilter {
    qk_filter *h = nullptr;
    bool exclude = false;
    const void *owner = nullptr;  // the store of the index that made it (compared, never dereferenced)
    SearchFilter() = default;
    SearchFilter(const SearchFilter &) = delete;
    SearchFilter &operator=(const SearchFilter &) = delete;
    ~SearchFilter() {
        if (h) (void)qk_filter_destroy(h);
    }
};

struct SearchParams {  // common.h:171-184
    int nprobe = DEFAULT_NPROBE;
    int k = DEFAULT_K;
    float recall_target = DEFAULT_RECALL_TARGET;
    int num_threads = 1;
    float k_factor = 1.0f;
    bool use_precomputed = true;
    bool batched_scan = false;
    float recompute_threshold = 0.001f;
    float initial_search_fraction = 0.02f;
    int aps_flush_period_us = 100;
    shared_ptr<SearchFilter> filter = nullptr;  // extension, not part of the summary: search only the filter's candidates
    // extension, not part of the summary: one filter per query of the batch -- query i sees the candidates of
    // filters[query_filter[i]] (query_filter: integer tensor [Q]).  Given together, exclusive with `filter`
    std::vector<shared_ptr<SearchFilter>> filters;
    Tensor query_filter;
    // extension, not part of the summary: adaptive probing under a filter -- with max_nprobe > nprobe every query probes the
    // shortest prefix of its max_nprobe nearest partitions, at least nprobe of them, that holds filter_min_candidates (0 = k)
    // candidates of its filter; 0 = off, max_nprobe == nprobe is the fixed call, a value below nprobe is refused.
    // SearchResult::nprobed says how many each query probed
    int max_nprobe = 0;
    int64_t filter_min_candidates = 0;
    // extension, not part of the summary: exact search under a selective filter -- with filter_exact_rows > 0 and `filter` set, a
    // filter that has at most that many candidate vectors in the index NOW is answered exactly: the k best of ALL its candidates,
    // no partition probed, k up to 8192 (SearchResult::exact = 1); a filter with more takes the path it takes today, fixed nprobe
    // or adaptive under max_nprobe (exact = 0).  0 = off.  An exact call probes no partition, so it records no hits for the
    // maintenance policy
    int64_t filter_exact_rows = 0;
    // extension, not part of the summary: the same with one filter per query -- with filters_exact_rows > 0 and `filters` /
    // `query_filter` set, the queries whose filter has at most that many candidates NOW are answered exactly in one call over the
    // index's candidate pool (SearchResult::exact_mask says which), the others take the path they take today.
    // filters_exact_pool_rows > 0 bounds the rows that pool holds (0 = no bound)
    int64_t filters_exact_rows = 0;
    int64_t filters_exact_pool_rows = 0;
};

struct BuildTimingInfo {  // common.h:189-198
    int64_t n_vectors = 0, n_clusters = 0;
    int d = 0, num_codebooks = -1, code_size = -1;
    int train_time_us = 0, assign_time_us = 0, total_time_us = 0;
};

struct ModifyTimingInfo {  // common.h:203-209
    int64_t n_vectors = 0;
    int input_validation_time_us = 0, find_partition_time_us = 0, modify_time_us = 0, maintenance_time_us = 0;
};

struct SearchTimingInfo {  // common.h:214-228
    int64_t n_queries = 0, n_clusters = 0;
    int partitions_scanned = 0;
    shared_ptr<SearchParams> search_params = nullptr;
    shared_ptr<SearchTimingInfo> parent_info = nullptr;
    int64_t buffer_init_time_ns = 0, job_enqueue_time_ns = 0, boundary_distance_time_ns = 0, job_wait_time_ns = 0,
            result_aggregate_time_ns = 0, total_time_ns = 0;
};

struct MaintenanceTimingInfo {  // common.h:233-241
    int64_t n_splits = 0, n_deletes = 0, delete_time_us = 0, delete_refine_time_us = 0, split_time_us = 0,
            split_refine_time_us = 0, total_time_us = 0;
};

// extension (QuakeIndex::search_after): one position per query in the total order (key, id) of its results -- keys int32 [Q] holding
// the uint32 bit pattern of the integer key the top-k compares, ids int64 [Q].  A position, not a snapshot: it stays valid across
// add / remove / maintenance.  (0, -1) is the start, (0xFFFFFFFF, INT64_MAX) an exhausted query
struct SearchCursor {
    Tensor keys;
    Tensor ids;
};

struct SearchResult {  // common.h:243-247
    Tensor ids;
    Tensor distances;
    shared_ptr<SearchTimingInfo> timing_info;
    Tensor nprobed;  // extension: int32 [Q] partitions probed per query under SearchParams::max_nprobe, else undefined
    int exact = -1;  // extension: 1 / 0 on a search that consulted SearchParams::filter_exact_rows, else -1 (None in Python)
    shared_ptr<SearchCursor> cursor = nullptr;  // extension: the cursor behind this page (QuakeIndex::search_after), else null
    Tensor exact_mask;  // extension: bool [Q], the queries answered exactly under SearchParams::filters_exact_rows, else undefined
};

// extension (QuakeIndex::range_search): query i's hits are ids / distances [lims[i], lims[i+1]), in scan order
struct RangeSearchResult {
    Tensor lims;
    Tensor ids;
    Tensor distances;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::grouped_search): the k best groups of a column per query -- ids / distances [Q, k] of each group's best vector,
// groups [Q, k] the group values (0 where ids is the padding id -1); with group_size = m, ids / distances [Q, k, m]
struct GroupedSearchResult {
    Tensor ids;
    Tensor distances;
    Tensor groups;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::facet_counts): per column and query the n_values most frequent values among the query's range hits --
// values / counts [C, Q, n] (count descending, then value ascending; padding is value 0, count 0), distinct / missing [C, Q],
// totals [Q] the hits of every query, columns the C column names
struct FacetResult {
    Tensor values;
    Tensor counts;
    Tensor distinct;
    Tensor missing;
    Tensor totals;
    std::vector<std::string> columns;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::facet_stats): per column and query, over the query's range hits: count / missing / min / max / sum_lo /
// sum_hi [C, Q] (min / max of a count of 0 are INT64_MAX / INT64_MIN; the exact sum is sum_hi * 2^64 + (sum_lo mod 2^64)),
// histogram [C, Q, 1 + the most edges of a column] (bucket b of a value v = the number of the column's edges <= v), totals [Q],
// columns the C column names, edges the C edge lists
// the edges of a facet_stats call, one checked list per column, produced when the call has passed its refusals and found its
// columns -- the point at which the Python mirror lowers them -- so that both mirrors raise the same error for the same call
using FacetEdgesFn = std::function<std::vector<std::vector<int64_t>>()>;

struct FacetStatsResult {
    Tensor count;
    Tensor missing;
    Tensor min;
    Tensor max;
    Tensor sum_lo;
    Tensor sum_hi;
    Tensor histogram;
    Tensor totals;
    std::vector<std::string> columns;
    std::vector<std::vector<int64_t>> edges;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::ordered_search): per query the k first range hits by an attribute column: ids [Q, k] (padding -1),
// distances [Q, k] (padding as search pads), values [Q, k] (0 without a value and at padding), counts / missing / totals [Q]
struct OrderedSearchResult {
    Tensor ids;
    Tensor distances;
    Tensor values;
    Tensor counts;
    Tensor missing;
    Tensor totals;
    std::string column;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::multi_vector_search): per logical query the k best values of an attribute column by the sum over the query's
// vectors of the best hit among the value's rows: groups [L, k] (padding 0), scores [L, k] (padding as search pads), matched [L, k]
// int32 (padding 0), n_groups [L], hits [L, T]
struct MultiVectorSearchResult {
    Tensor groups;
    Tensor scores;
    Tensor matched;
    Tensor n_groups;
    Tensor hits;
    std::string column;
    shared_ptr<SearchTimingInfo> timing_info;
};

// extension (QuakeIndex::diverse_search): per query k of its fetch_k nearest vectors chosen by maximal marginal relevance, in
// selection order: ids [Q, k] (padding -1), distances [Q, k] (padding as search pads), ranks [Q, k] int32 (padding -1)
struct DiverseSearchResult {
    Tensor ids;
    Tensor distances;
    Tensor ranks;
    shared_ptr<SearchTimingInfo> timing_info;
};

struct Clustering {  // common.h:249-276
    Tensor centroids;
    Tensor partition_ids;
    std::vector<Tensor> vectors;
    std::vector<Tensor> vector_ids;
    int64_t ntotal() const {
        int64_t n = 0;
        for (const auto &v : vectors)
            if (v.defined() && v.numel() > 0) n += v.size(0);
        return n;
    }
    int64_t nlist() const { return (int64_t)vectors.size(); }
    int64_t dim() const { return centroids.size(1); }
    int64_t cluster_size(int64_t i) const { return vectors[(size_t)i].size(0); }
};

int str_to_metric_type(std::string metric);  // common.h:145-156: "l2" -> 1, "ip" -> 0, else std::invalid_argument

// ---- plumbing shared by the mirror's translation units (not part of the reference surface) -------------------------------
void qk_check(int status);            // qk_status -> the exception type the reference throws (invalid_argument / runtime_error)
qk_ctx *qk_device_context(int device);  // one shared context per device
Tensor host_f32(const Tensor &t);
Tensor host_i64(const Tensor &t);

}  // namespace quake_amd
