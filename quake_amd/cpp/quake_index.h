// quake_index.h -- QuakeIndex of the C++ host mirror: the public surface of the reference's
// src/cpp/include/quake_index.h:18-142 (same member and method names) on top of the C ABI (include/quake_hip.h).  Like the
// reference it is a facade over three collaborators it owns and exposes: partition_manager_ (the device partition store
// + its bookkeeping), query_coordinator_ (search) and maintenance_policy_.  Every method body is new: it marshals torch
// tensors to libquake_hip.so, where all arithmetic happens.
#pragma once
#include "common.h"
#include "list_scanning.h"
#include "maintenance_policies.h"
#include "partition_manager.h"
#include "query_coordinator.h"

#include <map>

namespace quake_amd {

// extension: one clause of make_filter_where -- (name, op, a[, b]) with op one of "==" "!=" "<" "<=" ">" ">=" "between" "any_bits"
// "all_bits" "no_bits".  An operand is an integer of any size: `over` says it lies below (-1) / above (+1) int64 (v is then
// unused, except that a bit mask in [2^63, 2^64) arrives as its two's complement with over == 0); lowering saturates, never wraps.
struct WhereOperand {
    int64_t v = 0;
    int over = 0;
};
struct WhereTerm {
    std::string name, op;
    WhereOperand a, b;
    int n_operands = 1;
    // the set ops "in" / "not_in" (lower_expr only): the operand is a value list
    std::vector<WhereOperand> values;
    bool has_values = false;
};
struct LoweredClause {
    std::string name;
    int op = QK_OP_RANGE;
    int64_t a = 0, b = 0;
    std::vector<int64_t> values;  // QK_OP_IN_SET / QK_OP_NOT_IN_SET: ascending, distinct
};
// the C clauses of a predicate (the Python mirror's quake_amd/where.py: same rules, same errors as std::runtime_error)
std::vector<LoweredClause> lower_where(const std::vector<WhereTerm> &where);
// an OR of conjunctions with the set ops (where.py's lower_expr): every term is lowered like a `where`, ("in" | "not_in", values)
// becomes a set clause, a value outside int64 is dropped
std::vector<std::vector<LoweredClause>> lower_expr(const std::vector<std::vector<WhereTerm>> &any_of);

// the histogram edges of facet_stats (where.py's lower_edges: same rules, same errors as std::runtime_error): one operand list per
// column of `names` (empty: no edges) -> the lists inside int64; refuses more than QK_MAX_FACET_EDGES edges, an edge outside int64,
// edges that are not strictly ascending
std::vector<std::vector<int64_t>> lower_edges(const std::vector<std::string> &names, const std::vector<std::vector<WhereOperand>> &edges);

// the arguments of ordered_search (where.py's lower_order: same rules, same errors as std::runtime_error, in the same order): an
// unknown column, k outside 1 .. QK_MAX_ORDER_K, a `missing` that is neither "exclude" nor "last" -> the flags of qk_order_search
int lower_order(const std::vector<std::string> &columns, const std::string &order_by, int64_t k, bool descending, const std::string &missing);

// the arguments of multi_vector_search (where.py's lower_maxsim: same rules, same errors as std::runtime_error, in the same order):
// an unknown column, k outside 1 .. QK_MAXSIM_MAX_K, T outside 1 .. QK_MAXSIM_MAX_TOKENS, an n_tokens entry outside [0, T], no
// `missing` under l2, a NaN `missing` -> missing (0.0 for the inner product when none is given)
double lower_maxsim(const std::vector<std::string> &columns, const std::string &group_by, int64_t k, int64_t T,
                    const std::optional<std::vector<int64_t>> &n_tokens, std::optional<double> missing, bool is_ip);

// the arguments of diverse_search (where.py's lower_diverse: same rules, same errors as std::runtime_error, in the same order):
// k < 1, fetch_k < k, fetch_k > QK_MAX_FETCH_K, a lambda_mult that is NaN or outside [0, 1] -> lambda_mult rounded to float32
float lower_diverse(int64_t k, int64_t fetch_k, double lambda_mult);

class QuakeIndex : public std::enable_shared_from_this<QuakeIndex> {
public:
    shared_ptr<QuakeIndex> parent_;
    shared_ptr<PartitionManager> partition_manager_;
    shared_ptr<QueryCoordinator> query_coordinator_;
    shared_ptr<MaintenancePolicy> maintenance_policy_;
    int metric_ = QK_METRIC_L2;
    shared_ptr<IndexBuildParams> build_params_;
    shared_ptr<MaintenancePolicyParams> maintenance_policy_params_;
    int current_level_ = 0;
    bool debug_ = false;

    explicit QuakeIndex(int current_level = 0);
    ~QuakeIndex();
    QuakeIndex(const QuakeIndex &) = delete;
    QuakeIndex &operator=(const QuakeIndex &) = delete;

    shared_ptr<BuildTimingInfo> build(Tensor x, Tensor ids, shared_ptr<IndexBuildParams> build_params);
    shared_ptr<SearchResult> search(Tensor x, shared_ptr<SearchParams> search_params);
    Tensor get(Tensor ids);
    Tensor get_ids();
    shared_ptr<ModifyTimingInfo> add(Tensor x, Tensor ids);
    shared_ptr<ModifyTimingInfo> remove(Tensor ids);
    shared_ptr<ModifyTimingInfo> modify(Tensor ids, Tensor x);
    void initialize_maintenance_policy(shared_ptr<MaintenancePolicyParams> maintenance_policy_params);
    shared_ptr<MaintenanceTimingInfo> maintenance();
    void refine_partitions(Tensor partition_ids, int iterations);
    // extension: a filter over this index's vector ids for SearchParams::filter (ids: any integer tensor, host or device)
    shared_ptr<SearchFilter> make_filter(Tensor ids, bool exclude = false);
    // extension: a predicate filter over the attribute columns below -- every clause must hold; it holds no ids and follows
    // later set_attribute / add calls (qk_filter_create_where)
    shared_ptr<SearchFilter> make_filter_where(const std::vector<WhereTerm> &where);
    // extension: an OR of up to QK_MAX_TERMS such conjunctions, with the value sets "in" / "not_in" (qk_filter_create_expr);
    // make_filter_where hands a `where` that names a set op to it
    shared_ptr<SearchFilter> make_filter_expr(const std::vector<std::vector<WhereTerm>> &any_of);
    // extension: attribute columns -- int64 values keyed by vector id, on the device (qk_attr_*); a column is created by its
    // first set_attribute; ids need not be stored, remove / modify keep the values; not persisted by save()
    void set_attribute(const std::string &name, Tensor ids, Tensor values);
    void unset_attribute(const std::string &name, Tensor ids);
    std::pair<Tensor, Tensor> get_attribute(const std::string &name, Tensor ids);  // (values int64 [n], found bool [n])
    std::vector<std::string> attribute_names();
    // extension: the page of search_params->k results behind `cursor` (null: from the start); pages chained from the start concatenate
    // to what search() with a larger k returns (qk_search_after).  Records no hits for maintenance
    shared_ptr<SearchResult> search_after(Tensor x, shared_ptr<SearchParams> search_params, shared_ptr<SearchCursor> cursor = nullptr);
    // extension: every vector of the search_params->nprobe nearest partitions within `radius` of each query (qk_range_search)
    shared_ptr<RangeSearchResult> range_search(Tensor x, float radius, shared_ptr<SearchParams> search_params);
    // extension: the search_params->k best groups of attribute column `group_by` among the vectors of the nprobe nearest partitions,
    // every group represented by its best (allowed) vector (qk_search_grouped)
    // group_size = m, 1 <= m <= QK_MAX_GROUP_SIZE: the m best vectors of every group, ids / distances [Q, k, m] (qk_search_grouped_n)
    shared_ptr<GroupedSearchResult> grouped_search(Tensor x, const std::string &group_by, shared_ptr<SearchParams> search_params,
                                                   std::optional<int> group_size = std::nullopt);
    // extension: per query, the value counts of up to QK_MAX_FACET_COLS attribute columns over the hits of range_search with the
    // same arguments (radius unset: every vector of the probed partitions), the n_values most frequent per column (qk_facet_search)
    shared_ptr<FacetResult> facet_counts(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> search_params,
                                         std::optional<float> radius = std::nullopt, int n_values = 10);
    // extension: count, min, max, exact sum and a histogram with the given bucket edges (one checked list per column, lower_edges)
    // of up to QK_MAX_FACET_COLS attribute columns over the same hits (qk_facet_stats_search)
    shared_ptr<FacetStatsResult> facet_stats(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> search_params,
                                             std::optional<float> radius, const std::vector<std::vector<int64_t>> &edges);
    // the same with the edges produced on demand, behind the call's refusals (the binding: Python objects are parsed there)
    shared_ptr<FacetStatsResult> facet_stats(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> search_params,
                                             std::optional<float> radius, const FacetEdgesFn &edges_fn);
    // extension: "sort by" -- the search_params->k first range hits by the attribute column `order_by`, ascending or descending, ties
    // to the nearer vector, then to the smaller id; missing: "exclude" | "last" (qk_order_search)
    shared_ptr<OrderedSearchResult> ordered_search(Tensor x, const std::string &order_by, shared_ptr<SearchParams> search_params,
                                                   std::optional<float> radius = std::nullopt, bool descending = false,
                                                   const std::string &missing = "exclude");
    // extension: multi-vector (late interaction) search -- x [L, T, d]; per logical query the search_params->k best values of the
    // attribute column `group_by` by the sum over the query's vectors of the best range hit among the value's vectors, `missing`
    // where there is none (qk_maxsim_search)
    shared_ptr<MultiVectorSearchResult> multi_vector_search(Tensor x, const std::string &group_by, shared_ptr<SearchParams> search_params,
                                                            std::optional<float> radius = std::nullopt,
                                                            const std::optional<std::vector<int64_t>> &n_tokens = std::nullopt,
                                                            std::optional<double> missing = std::nullopt);
    // extension: diversified search -- search_params->k of the fetch_k nearest vectors of each query, chosen greedily by maximal
    // marginal relevance with weight lambda_mult in [0, 1] (qk_diverse_search)
    shared_ptr<DiverseSearchResult> diverse_search(Tensor x, shared_ptr<SearchParams> search_params, int64_t fetch_k, double lambda_mult = 0.5);
    // the reference never feeds its hit tracker from search(): with this switch on, search() records the
    // partitions every query probed, so maintenance() has a window to act on
    void set_track_hits(bool on);
    // scan-latency grid of the maintenance cost model from a CSV in the reference's profile format
    // (maintenance_cost_estimator.cpp:259-365): loaded if the file exists, else profiled on the device and saved there
    void set_latency_profile(const std::string &path);
    void publish();  // pending modifications visible to searches now, not inside the next query (qk_store_publish)
    bool validate();
    void save(const std::string &path);
    void load(const std::string &path, int n_workers = 0);
    int64_t ntotal();
    int64_t nlist();
    int d();

    qk_store *store() { return partition_manager_ ? partition_manager_->store() : nullptr; }

private:
    std::map<std::string, qk_attr *> attrs_;  // columns of attrs_store_ (a rebuilt or loaded index starts without columns)
    qk_store *attrs_store_ = nullptr;
    std::map<std::string, qk_attr *> &attributes(const char *who);
    void drop_attributes();
    void require_built(const char *msg) const;
    void make_coordinator(int num_workers);
};

}  // namespace quake_amd
