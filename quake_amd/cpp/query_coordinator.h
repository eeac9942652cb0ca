// query_coordinator.h -- QueryCoordinator of the C++ host mirror: the public surface of the reference's
// src/cpp/include/query_coordinator.h:45-179.  search() = parent search for the nprobe nearest partitions, then
// scan_partitions(); on the device the three scan variants of the reference (serial_scan, batched_serial_scan, worker_scan:
// three ways of spreading the same work over CPU threads) are ONE pipeline -- qk_search / qk_scan of libquake_hip.so -- and
// return the same result, so all three names enqueue it.  A WORKER IS A GPU: initialize_workers(n) distributes the partitions
// over a device group of n members (PartitionManager::distribute_partitions -> qk_group, partition p on member p % n) and from
// then on search / scan_partitions / worker_scan run on all members at once (qk_group_search / qk_group_scan); results -- ids and
// distance bits -- equal the one-device pipeline's.
#pragma once
#include "common.h"

namespace quake_amd {

class QuakeIndex;
class PartitionManager;
class MaintenancePolicy;

class QueryCoordinator {
public:
    shared_ptr<PartitionManager> partition_manager_;
    shared_ptr<MaintenancePolicy> maintenance_policy_;
    shared_ptr<QuakeIndex> parent_;
    MetricType metric_;
    bool workers_initialized_ = false;
    int num_workers_ = 0;
    bool debug_ = false;
    // Device (CUDA) tensors in -> device tensors out, enqueued on torch's current stream with NO host synchronisation: the counters
    // and phase times of SearchTimingInfo need one (they are read back from the device), so for device tensors they are filled only
    // when this is set -- host-tensor searches synchronise anyway and always fill them (query_coordinator.cpp:612-657 always does: its
    // scan is host code).  Recall-target searches and hit tracking read their counters in either case.
    bool device_timing_ = false;

    QueryCoordinator(shared_ptr<QuakeIndex> parent, shared_ptr<PartitionManager> partition_manager,
                     shared_ptr<MaintenancePolicy> maintenance_policy, MetricType metric, int num_workers = 0);
    ~QueryCoordinator();

    shared_ptr<SearchResult> search(Tensor x, shared_ptr<SearchParams> search_params);
    // extension (qk_search_after): the page of sp->k results behind `cursor` (null: from the start) among the nprobe nearest partitions,
    // restricted to sp->filter if set; the result's cursor continues behind it.  Records no hits for maintenance
    shared_ptr<SearchResult> search_after(Tensor x, shared_ptr<SearchParams> search_params, shared_ptr<SearchCursor> cursor);
    // extension (qk_range_search): all vectors of the nprobe nearest partitions within `radius`, restricted to sp->filter if set
    shared_ptr<RangeSearchResult> range_search(Tensor x, float radius, shared_ptr<SearchParams> search_params);
    // extension (qk_search_grouped): the k best groups of `group_by` -- a column of this index's store, nullptr: unknown -- per query
    // group_size = m (qk_search_grouped_n): ids / distances [Q, k, m], the m best vectors of every group; unset: the one-row result [Q, k]
    shared_ptr<GroupedSearchResult> grouped_search(Tensor x, qk_attr *group_by, const std::string &name, shared_ptr<SearchParams> search_params,
                                                   std::optional<int> group_size = std::nullopt);
    // extension (qk_facet_search): value counts of `cols` -- columns of this index's store, nullptr: unknown -- over the range hits
    shared_ptr<FacetResult> facet_counts(Tensor x, const std::vector<qk_attr *> &cols, const std::vector<std::string> &names,
                                         shared_ptr<SearchParams> search_params, std::optional<float> radius, int n_values);
    // extension (qk_facet_stats_search): count / missing / min / max / exact sum / histogram of `cols` over the range hits; edges_fn:
    // one checked list per column (lower_edges), asked for behind the refusals and the column lookup
    shared_ptr<FacetStatsResult> facet_stats(Tensor x, const std::vector<qk_attr *> &cols, const std::vector<std::string> &names,
                                             shared_ptr<SearchParams> search_params, std::optional<float> radius,
                                             const FacetEdgesFn &edges_fn);
    // extension (qk_order_search): the search_params->k first range hits by `col` -- the column `order_by` of this index's store,
    // nullptr: unknown; `known`: the names of the store's columns (lower_order runs behind the refusals)
    shared_ptr<OrderedSearchResult> ordered_search(Tensor x, qk_attr *col, const std::vector<std::string> &known, const std::string &order_by,
                                                   shared_ptr<SearchParams> search_params, std::optional<float> radius, bool descending,
                                                   const std::string &missing);
    // extension (qk_maxsim_search): x [L, T, d], the search_params->k best values of `col` per logical query by the sum of the best
    // hits of its vectors -- the column `group_by` of this index's store, nullptr: unknown; `known`: the names of the store's columns
    // (lower_maxsim runs behind the refusals)
    shared_ptr<MultiVectorSearchResult> multi_vector_search(Tensor x, qk_attr *col, const std::vector<std::string> &known,
                                                            const std::string &group_by, shared_ptr<SearchParams> search_params,
                                                            std::optional<float> radius, const std::optional<std::vector<int64_t>> &n_tokens,
                                                            std::optional<double> missing);
    // extension (qk_diverse_search): search_params->k of the fetch_k nearest vectors of each query by maximal marginal relevance
    // (lower_diverse runs behind the refusals)
    shared_ptr<DiverseSearchResult> diverse_search(Tensor x, shared_ptr<SearchParams> search_params, int64_t fetch_k, double lambda_mult);
    shared_ptr<SearchResult> scan_partitions(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> search_params);
    shared_ptr<SearchResult> serial_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> search_params);
    shared_ptr<SearchResult> batched_serial_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> search_params);
    shared_ptr<SearchResult> worker_scan(Tensor x, Tensor partition_ids, shared_ptr<SearchParams> search_params);
    void initialize_workers(int num_workers);
    void shutdown_workers();

private:
    shared_ptr<SearchResult> empty_result(shared_ptr<SearchParams> sp) const;
};

}  // namespace quake_amd
