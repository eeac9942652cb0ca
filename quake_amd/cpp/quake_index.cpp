// quake_index.cpp -- method bodies of the QuakeIndex facade (see quake_index.h) and the plumbing shared by the mirror's
// translation units.  No arithmetic here.
#include "quake_index.h"

#include <algorithm>
#include <cstdio>
#include <chrono>
#include <filesystem>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>

namespace quake_amd {

namespace {
using clk = std::chrono::high_resolution_clock;
inline int us_since(clk::time_point t0) { return (int)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); }
}  // namespace

void qk_check(int st) {
    if (st == QK_OK) return;
    if (st == QK_ERR_INVALID) throw std::invalid_argument(qk_last_error());
    throw std::runtime_error(qk_last_error());
}

qk_ctx *qk_device_context(int device) {
    static std::mutex mu;
    static std::map<int, qk_ctx *> ctxs;
    std::lock_guard<std::mutex> lock(mu);
    auto it = ctxs.find(device);
    if (it != ctxs.end()) return it->second;
    qk_ctx *c = nullptr;
    qk_check(qk_ctx_create(device, &c));
    ctxs[device] = c;
    return c;
}

Tensor host_f32(const Tensor &t) { return t.to(torch::kCPU, torch::kFloat32).contiguous(); }
Tensor host_i64(const Tensor &t) { return t.to(torch::kCPU, torch::kInt64).contiguous(); }

int str_to_metric_type(std::string metric) {
    std::transform(metric.begin(), metric.end(), metric.begin(), ::tolower);
    if (metric == "l2") return QK_METRIC_L2;
    if (metric == "ip") return QK_METRIC_IP;
    throw std::invalid_argument("Invalid metric type: " + metric);
}

QuakeIndex::QuakeIndex(int current_level) : current_level_(current_level) {}
QuakeIndex::~QuakeIndex() { drop_attributes(); }

void QuakeIndex::require_built(const char *msg) const {
    if (!partition_manager_ || !partition_manager_->has_lists()) throw std::runtime_error(msg);
}

void QuakeIndex::make_coordinator(int num_workers) {
    initialize_maintenance_policy(maintenance_policy_params_ ? maintenance_policy_params_ : std::make_shared<MaintenancePolicyParams>());
    query_coordinator_ = std::make_shared<QueryCoordinator>(parent_, partition_manager_, maintenance_policy_, (MetricType)metric_, num_workers);
}

shared_ptr<BuildTimingInfo> QuakeIndex::build(Tensor x, Tensor ids, shared_ptr<IndexBuildParams> build_params) {  // quake_index.cpp:29-90
    auto t_total = clk::now();
    drop_attributes();  // (columns belong to the store that is replaced here)
    build_params_ = build_params;
    metric_ = str_to_metric_type(build_params_->metric);
    if (x.dim() != 2) throw std::runtime_error("[QuakeIndex::build] x must be 2-D [num_vectors, dimension]");
    if (x.size(0) != ids.size(0)) throw std::runtime_error("[QuakeIndex::build] x.size(0) != ids.size(0)");
    const int64_t n = x.size(0);
    const int d = (int)x.size(1);
    auto info = std::make_shared<BuildTimingInfo>();
    info->n_vectors = n;
    info->d = d;
    partition_manager_ = std::make_shared<PartitionManager>();
    partition_manager_->metric_ = metric_;
    // num_workers > 0: the partitions go straight to the members of a device group (initialize_workers -> distribute_partitions
    // would move them there anyway, through one device)
    partition_manager_->plan_workers(build_params_->num_workers);
    const int nlist = build_params_->nlist;
    if (nlist > 1) {
        // The build's copy of x (:33) lives on the DEVICE: one transfer of the caller's rows, then k-means, the stable bucketing by
        // assignment (torch::sort + index_select in the reference, clustering.cpp:69-72) and the store's ingest all run there.
        // (Host-side the same steps -- clone, argsort and index_select of 5 GB, a second transfer -- were 10.8 s for 10M x 128.)
        auto t0 = clk::now();
        const auto dev0 = torch::Device(torch::kCUDA, 0);
        Tensor xd = x.to(dev0, torch::kFloat32, /*non_blocking=*/false, /*copy=*/true).contiguous();
        Tensor idd = ids.to(dev0, torch::kInt64).reshape({-1}).contiguous();
        Tensor centroids_d = torch::empty({nlist, d}, torch::TensorOptions().dtype(torch::kFloat32).device(dev0));
        Tensor assign_d = torch::empty({n}, torch::TensorOptions().dtype(torch::kInt64).device(dev0));
        torch::cuda::synchronize();
        // kmeans() (clustering.cpp:13-97); IP: the copy is normalised in place, the normalised rows are what gets stored
        qk_check(qk_kmeans(qk_device_context(0), xd.data_ptr<float>(), n, d, nlist, metric_, build_params_->niter, 1234ULL,
                           centroids_d.data_ptr<float>(), assign_d.data_ptr<int64_t>(), QK_MEM_DEVICE));
        qk_check(qk_ctx_synchronize(qk_device_context(0)));
        info->train_time_us = us_since(t0);
        t0 = clk::now();
        Tensor order = torch::argsort(assign_d, /*stable=*/true);
        Tensor counts = torch::bincount(assign_d, {}, nlist).to(torch::kInt64).cpu();
        Tensor offsets = torch::zeros({nlist + 1}, torch::kInt64);
        offsets.slice(0, 1, nlist + 1).copy_(torch::cumsum(counts, 0));
        parent_ = std::make_shared<QuakeIndex>(current_level_ + 1);
        auto pp = std::make_shared<IndexBuildParams>();
        pp->metric = build_params_->metric;
        pp->num_workers = build_params_->num_workers;
        parent_->build(centroids_d.cpu(), torch::arange(nlist, torch::kInt64), pp);
        Tensor ids_sorted = idd.index_select(0, order);
        Tensor x_sorted = xd.index_select(0, order);
        xd = Tensor();  // (the unsorted copy is not needed next to the sorted one and the arena)
        partition_manager_->init_from_csr(parent_, offsets, ids_sorted, x_sorted);
        info->assign_time_us = us_since(t0);
        info->n_clusters = nlist;
    } else {  // flat index (:68-79): one partition
        Tensor xh = host_f32(x).clone();  // build clones x (:33)
        Tensor idh = host_i64(ids);
        parent_ = nullptr;
        Tensor offsets = torch::tensor({(int64_t)0, n}, torch::kInt64);
        partition_manager_->init_from_csr(nullptr, offsets, idh, xh);
        info->n_clusters = 1;
    }
    make_coordinator(build_params_->num_workers);
    info->total_time_us = us_since(t_total);
    return info;
}

shared_ptr<SearchResult> QuakeIndex::search(Tensor x, shared_ptr<SearchParams> sp) {  // :93-99
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::search()] No query coordinator. Did you build the index?");
    return query_coordinator_->search(x, sp);
}

shared_ptr<SearchResult> QuakeIndex::search_after(Tensor x, shared_ptr<SearchParams> sp, shared_ptr<SearchCursor> cursor) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::search_after()] No query coordinator. Did you build the index?");
    return query_coordinator_->search_after(x, sp, cursor);
}

shared_ptr<RangeSearchResult> QuakeIndex::range_search(Tensor x, float radius, shared_ptr<SearchParams> sp) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::range_search()] No query coordinator. Did you build the index?");
    return query_coordinator_->range_search(x, radius, sp);
}

shared_ptr<GroupedSearchResult> QuakeIndex::grouped_search(Tensor x, const std::string &group_by, shared_ptr<SearchParams> sp,
                                                           std::optional<int> group_size) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::grouped_search()] No query coordinator. Did you build the index?");
    qk_attr *col = nullptr;
    if (partition_manager_ && partition_manager_->has_lists() && partition_manager_->store() && partition_manager_->store() == attrs_store_) {
        auto it = attrs_.find(group_by);
        if (it != attrs_.end()) col = it->second;
    }
    return query_coordinator_->grouped_search(x, col, group_by, sp, group_size);
}

shared_ptr<FacetResult> QuakeIndex::facet_counts(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> sp,
                                                 std::optional<float> radius, int n_values) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::facet_counts()] No query coordinator. Did you build the index?");
    std::vector<qk_attr *> cols(facet_by.size(), nullptr);
    if (partition_manager_ && partition_manager_->has_lists() && partition_manager_->store() && partition_manager_->store() == attrs_store_)
        for (size_t c = 0; c < facet_by.size(); c++) {
            auto it = attrs_.find(facet_by[c]);
            if (it != attrs_.end()) cols[c] = it->second;
        }
    return query_coordinator_->facet_counts(x, cols, facet_by, sp, radius, n_values);
}

std::vector<std::vector<int64_t>> lower_edges(const std::vector<std::string> &names, const std::vector<std::vector<WhereOperand>> &edges) {
    const std::string who = "[QuakeIndex::facet_stats()]";
    if (edges.size() != names.size())
        throw std::runtime_error(who + " edges has " + std::to_string(edges.size()) + " per-column entries for " + std::to_string(names.size()) +
                                 " columns");
    std::vector<std::vector<int64_t>> out(names.size());
    for (size_t c = 0; c < names.size(); c++) {
        const std::vector<WhereOperand> &e = edges[c];
        if (e.size() > QK_MAX_FACET_EDGES)
            throw std::runtime_error(who + " '" + names[c] + "' has " + std::to_string(e.size()) + " edges, at most " +
                                     std::to_string(QK_MAX_FACET_EDGES) + " are supported");
        for (size_t i = 0; i < e.size(); i++) {
            if (e[i].over) throw std::runtime_error(who + " edge " + std::to_string(i) + " of '" + names[c] + "' does not fit int64");
            if (i && e[i - 1].v >= e[i].v)
                throw std::runtime_error(who + " the edges of '" + names[c] + "' are not strictly ascending (edge " + std::to_string(i) + ")");
            out[c].push_back(e[i].v);
        }
    }
    return out;
}

shared_ptr<FacetStatsResult> QuakeIndex::facet_stats(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> sp,
                                                     std::optional<float> radius, const std::vector<std::vector<int64_t>> &edges) {
    return facet_stats(x, facet_by, sp, radius, FacetEdgesFn([&edges]() { return edges; }));
}

shared_ptr<FacetStatsResult> QuakeIndex::facet_stats(Tensor x, const std::vector<std::string> &facet_by, shared_ptr<SearchParams> sp,
                                                     std::optional<float> radius, const FacetEdgesFn &edges_fn) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::facet_stats()] No query coordinator. Did you build the index?");
    std::vector<qk_attr *> cols(facet_by.size(), nullptr);
    if (partition_manager_ && partition_manager_->has_lists() && partition_manager_->store() && partition_manager_->store() == attrs_store_)
        for (size_t c = 0; c < facet_by.size(); c++) {
            auto it = attrs_.find(facet_by[c]);
            if (it != attrs_.end()) cols[c] = it->second;
        }
    return query_coordinator_->facet_stats(x, cols, facet_by, sp, radius, edges_fn);
}

int lower_order(const std::vector<std::string> &columns, const std::string &order_by, int64_t k, bool descending, const std::string &missing) {
    const std::string who = "[QuakeIndex::ordered_search()]";
    if (std::find(columns.begin(), columns.end(), order_by) == columns.end())
        throw std::runtime_error(who + " unknown attribute column '" + order_by + "'");
    if (k < 1 || k > QK_MAX_ORDER_K)
        throw std::runtime_error(who + " k=" + std::to_string(k) + " must be between 1 and " + std::to_string(QK_MAX_ORDER_K));
    if (missing != "exclude" && missing != "last") throw std::runtime_error(who + " missing must be 'exclude' or 'last', got '" + missing + "'");
    return (descending ? QK_ORDER_DESC : 0) | (missing == "last" ? QK_ORDER_MISSING_LAST : 0);
}

shared_ptr<OrderedSearchResult> QuakeIndex::ordered_search(Tensor x, const std::string &order_by, shared_ptr<SearchParams> sp,
                                                           std::optional<float> radius, bool descending, const std::string &missing) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::ordered_search()] No query coordinator. Did you build the index?");
    std::vector<std::string> known;
    qk_attr *col = nullptr;
    if (partition_manager_ && partition_manager_->has_lists() && partition_manager_->store() && partition_manager_->store() == attrs_store_)
        for (const auto &kv : attrs_) {
            known.push_back(kv.first);
            if (kv.first == order_by) col = kv.second;
        }
    return query_coordinator_->ordered_search(x, col, known, order_by, sp, radius, descending, missing);
}

double lower_maxsim(const std::vector<std::string> &columns, const std::string &group_by, int64_t k, int64_t T,
                    const std::optional<std::vector<int64_t>> &n_tokens, std::optional<double> missing, bool is_ip) {
    const std::string who = "[QuakeIndex::multi_vector_search()]";
    if (std::find(columns.begin(), columns.end(), group_by) == columns.end())
        throw std::runtime_error(who + " unknown attribute column '" + group_by + "'");
    if (k < 1 || k > QK_MAXSIM_MAX_K)
        throw std::runtime_error(who + " k=" + std::to_string(k) + " must be between 1 and " + std::to_string(QK_MAXSIM_MAX_K));
    if (T < 1 || T > QK_MAXSIM_MAX_TOKENS)
        throw std::runtime_error(who + " T=" + std::to_string(T) + " vectors per query must be between 1 and " +
                                 std::to_string(QK_MAXSIM_MAX_TOKENS));
    if (n_tokens)
        for (size_t i = 0; i < n_tokens->size(); i++)
            if ((*n_tokens)[i] < 0 || (*n_tokens)[i] > T)
                throw std::runtime_error(who + " n_tokens[" + std::to_string(i) + "]=" + std::to_string((*n_tokens)[i]) +
                                         " must be between 0 and T=" + std::to_string(T));
    if (!missing) {
        if (!is_ip)
            throw std::runtime_error(who + " missing must be given for the l2 metric: the term of a vector without a match has no default");
        missing = 0.0;
    }
    if (*missing != *missing) throw std::runtime_error(who + " missing is NaN");
    return *missing;
}

shared_ptr<MultiVectorSearchResult> QuakeIndex::multi_vector_search(Tensor x, const std::string &group_by, shared_ptr<SearchParams> sp,
                                                                    std::optional<float> radius,
                                                                    const std::optional<std::vector<int64_t>> &n_tokens,
                                                                    std::optional<double> missing) {
    if (!query_coordinator_)
        throw std::runtime_error("[QuakeIndex::multi_vector_search()] No query coordinator. Did you build the index?");
    std::vector<std::string> known;
    qk_attr *col = nullptr;
    if (partition_manager_ && partition_manager_->has_lists() && partition_manager_->store() && partition_manager_->store() == attrs_store_)
        for (const auto &kv : attrs_) {
            known.push_back(kv.first);
            if (kv.first == group_by) col = kv.second;
        }
    return query_coordinator_->multi_vector_search(x, col, known, group_by, sp, radius, n_tokens, missing);
}

float lower_diverse(int64_t k, int64_t fetch_k, double lambda_mult) {
    const std::string who = "[QuakeIndex::diverse_search()]";
    if (k < 1) throw std::runtime_error(who + " k=" + std::to_string(k) + " must be at least 1");
    if (fetch_k < k) throw std::runtime_error(who + " fetch_k=" + std::to_string(fetch_k) + " must be at least k=" + std::to_string(k));
    if (fetch_k > QK_MAX_FETCH_K)
        throw std::runtime_error(who + " fetch_k=" + std::to_string(fetch_k) + " must not exceed " + std::to_string(QK_MAX_FETCH_K));
    if (lambda_mult != lambda_mult) throw std::runtime_error(who + " lambda_mult is NaN");
    if (!(lambda_mult >= 0.0 && lambda_mult <= 1.0)) {
        char buf[64];
        snprintf(buf, sizeof(buf), "%g", lambda_mult);
        throw std::runtime_error(who + " lambda_mult=" + buf + " must lie in [0, 1]");
    }
    return (float)lambda_mult;
}

shared_ptr<DiverseSearchResult> QuakeIndex::diverse_search(Tensor x, shared_ptr<SearchParams> sp, int64_t fetch_k, double lambda_mult) {
    if (!query_coordinator_) throw std::runtime_error("[QuakeIndex::diverse_search()] No query coordinator. Did you build the index?");
    return query_coordinator_->diverse_search(x, sp, fetch_k, lambda_mult);
}

shared_ptr<SearchFilter> QuakeIndex::make_filter(Tensor ids, bool exclude) {
    require_built("[QuakeIndex::make_filter()] No partition manager. Index not built?");
    qk_store *s = partition_manager_->store();
    if (!s) throw std::runtime_error("[QuakeIndex::make_filter()] filtered search is not supported with num_workers > 0");
    auto f = std::make_shared<SearchFilter>();
    f->exclude = exclude;
    f->owner = s;
    const bool on_dev = ids.defined() && ids.is_cuda();
    Tensor idl = !ids.defined() ? torch::empty({0}, torch::kInt64)
                 : on_dev     ? ids.reshape({-1}).to(torch::kInt64).contiguous()
                              : host_i64(ids.reshape({-1}));
    if (on_dev) torch::cuda::synchronize();  // (torch's stream made the ids; the library copies them out on its own)
    qk_check(qk_filter_create(s, idl.numel() > 0 ? idl.data_ptr<int64_t>() : nullptr, idl.numel(), exclude ? QK_FILTER_DENY : QK_FILTER_ALLOW,
                              on_dev ? QK_MEM_DEVICE : QK_MEM_HOST, &f->h));
    return f;
}

// ---- attribute columns and predicate filters (extension) -------------------------------------------------------------------------
std::vector<LoweredClause> lower_where(const std::vector<WhereTerm> &where) {
    const char *who = "[QuakeIndex::make_filter()]";
    constexpr int64_t MIN = INT64_MIN, MAX = INT64_MAX;
    if (where.empty()) throw std::runtime_error(std::string(who) + " where needs at least one clause");
    if (where.size() > QK_MAX_CLAUSES)
        throw std::runtime_error(std::string(who) + " where has " + std::to_string(where.size()) + " clauses, at most " +
                                 std::to_string(QK_MAX_CLAUSES) + " are supported");
    std::vector<LoweredClause> out;
    for (const WhereTerm &t : where) {
        LoweredClause c;
        c.name = t.name;
        const bool between = t.op == "between";
        const bool bits = t.op == "any_bits" || t.op == "all_bits" || t.op == "no_bits";
        if (!(between || bits || t.op == "==" || t.op == "!=" || t.op == "<" || t.op == "<=" || t.op == ">" || t.op == ">="))
            throw std::runtime_error(std::string(who) + " unknown where op '" + t.op + "'");
        if (t.n_operands != (between ? 2 : 1))
            throw std::runtime_error(std::string(who) + " where op '" + t.op + "' takes " + (between ? "2 operands" : "1 operand"));
        if (bits) {
            if (t.a.over) throw std::runtime_error(std::string(who) + " the mask of '" + t.op + "' does not fit 64 bits");
            c.op = t.op == "any_bits" ? QK_OP_ANY_BITS : t.op == "all_bits" ? QK_OP_ALL_BITS : QK_OP_NO_BITS;
            c.a = t.a.v;
            out.push_back(c);
            continue;
        }
        // the interval over the integers, cut to int64; (1, 0) if nothing is left
        bool empty = false;
        int64_t lo = MIN, hi = MAX;
        auto at_least = [&](const WhereOperand &o) {  // lo = o
            if (o.over > 0) empty = true;
            else if (o.over == 0) lo = o.v;
        };
        auto at_most = [&](const WhereOperand &o) {  // hi = o
            if (o.over < 0) empty = true;
            else if (o.over == 0) hi = o.v;
        };
        if (t.op == "==" || t.op == "!=") {
            at_least(t.a);
            at_most(t.a);
        } else if (t.op == "<") {
            if (t.a.over == 0 && t.a.v == MIN) empty = true;
            else at_most(t.a.over ? t.a : WhereOperand{t.a.v - 1, 0});
        } else if (t.op == "<=") {
            at_most(t.a);
        } else if (t.op == ">") {
            if (t.a.over == 0 && t.a.v == MAX) empty = true;
            else at_least(t.a.over ? t.a : WhereOperand{t.a.v + 1, 0});
        } else if (t.op == ">=") {
            at_least(t.a);
        } else {
            at_least(t.a);
            at_most(t.b);
        }
        if (empty || lo > hi) lo = 1, hi = 0;
        c.op = t.op == "!=" ? QK_OP_NOT_RANGE : QK_OP_RANGE;
        c.a = lo;
        c.b = hi;
        out.push_back(c);
    }
    return out;
}

std::vector<std::vector<LoweredClause>> lower_expr(const std::vector<std::vector<WhereTerm>> &any_of) {
    const std::string who = "[QuakeIndex::make_filter()]";
    if (any_of.empty()) throw std::runtime_error(who + " any_of needs at least one term");
    if (any_of.size() > QK_MAX_TERMS)
        throw std::runtime_error(who + " any_of has " + std::to_string(any_of.size()) + " terms, at most " + std::to_string(QK_MAX_TERMS) +
                                 " are supported");
    std::vector<std::vector<LoweredClause>> out;
    size_t total = 0;
    for (const std::vector<WhereTerm> &term : any_of) {
        if (term.empty()) throw std::runtime_error(who + " where needs at least one clause");
        if (term.size() > QK_MAX_CLAUSES)
            throw std::runtime_error(who + " where has " + std::to_string(term.size()) + " clauses, at most " + std::to_string(QK_MAX_CLAUSES) +
                                     " are supported");
        std::vector<LoweredClause> lt;
        for (const WhereTerm &t : term) {
            if (t.op != "in" && t.op != "not_in") {
                lt.push_back(lower_where({t})[0]);
                continue;
            }
            if (!t.has_values) throw std::runtime_error(who + " the operand of '" + t.op + "' must be a sequence of integers");
            if (t.values.size() > (size_t)QK_MAX_SET_VALUES)
                throw std::runtime_error(who + " the set of '" + t.op + "' has " + std::to_string(t.values.size()) + " values, at most " +
                                         std::to_string(QK_MAX_SET_VALUES) + " are supported");
            LoweredClause c;
            c.name = t.name;
            c.op = t.op == "in" ? QK_OP_IN_SET : QK_OP_NOT_IN_SET;
            for (const WhereOperand &o : t.values)
                if (!o.over) c.values.push_back(o.v);  // (a value outside int64 equals no stored value)
            std::sort(c.values.begin(), c.values.end());
            c.values.erase(std::unique(c.values.begin(), c.values.end()), c.values.end());
            lt.push_back(std::move(c));
        }
        total += lt.size();
        out.push_back(std::move(lt));
    }
    if (total > QK_MAX_EXPR_CLAUSES)
        throw std::runtime_error(who + " any_of has " + std::to_string(total) + " clauses in total, at most " +
                                 std::to_string(QK_MAX_EXPR_CLAUSES) + " are supported");
    return out;
}

void QuakeIndex::drop_attributes() {
    for (auto &kv : attrs_) (void)qk_attr_destroy(kv.second);  // (filters that name a column keep its values)
    attrs_.clear();
    attrs_store_ = nullptr;
}

std::map<std::string, qk_attr *> &QuakeIndex::attributes(const char *who) {
    const std::string w = std::string("[QuakeIndex::") + who + "()] ";
    if (!partition_manager_ || !partition_manager_->has_lists()) throw std::runtime_error(w + "No partition manager. Index not built?");
    qk_store *s = partition_manager_->store();
    if (!s) throw std::runtime_error(w + "filtered search is not supported with num_workers > 0");
    if (attrs_store_ != s) {
        drop_attributes();
        attrs_store_ = s;
    }
    return attrs_;
}

namespace {
// ids / values of an attribute call: int64, flat, where they are (the library copies device data out on its own)
Tensor attr_arg(const Tensor &t, bool on_dev) {
    return on_dev ? t.reshape({-1}).to(torch::kInt64).contiguous() : host_i64(t.reshape({-1}));
}
}  // namespace

void QuakeIndex::set_attribute(const std::string &name, Tensor ids, Tensor values) {
    auto &cols = attributes("set_attribute");
    if (ids.numel() != values.numel()) throw std::runtime_error("[QuakeIndex::set_attribute()] ids and values must have the same length");
    const bool on_dev = ids.is_cuda() && values.is_cuda();
    Tensor idl = attr_arg(ids, on_dev), vl = attr_arg(values, on_dev);
    if (on_dev) torch::cuda::synchronize();
    auto it = cols.find(name);
    if (it == cols.end()) {
        qk_attr *a = nullptr;
        qk_check(qk_attr_create(attrs_store_, &a));
        it = cols.emplace(name, a).first;
    }
    const int64_t n = idl.numel();
    qk_check(qk_attr_set(it->second, n ? idl.data_ptr<int64_t>() : nullptr, n ? vl.data_ptr<int64_t>() : nullptr, n,
                         on_dev ? QK_MEM_DEVICE : QK_MEM_HOST));
}

void QuakeIndex::unset_attribute(const std::string &name, Tensor ids) {
    auto &cols = attributes("unset_attribute");
    auto it = cols.find(name);
    if (it == cols.end()) throw std::runtime_error("[QuakeIndex::unset_attribute()] unknown attribute column '" + name + "'");
    const bool on_dev = ids.is_cuda();
    Tensor idl = attr_arg(ids, on_dev);
    if (on_dev) torch::cuda::synchronize();
    const int64_t n = idl.numel();
    qk_check(qk_attr_unset(it->second, n ? idl.data_ptr<int64_t>() : nullptr, n, on_dev ? QK_MEM_DEVICE : QK_MEM_HOST));
}

std::pair<Tensor, Tensor> QuakeIndex::get_attribute(const std::string &name, Tensor ids) {
    auto &cols = attributes("get_attribute");
    auto it = cols.find(name);
    if (it == cols.end()) throw std::runtime_error("[QuakeIndex::get_attribute()] unknown attribute column '" + name + "'");
    Tensor idl = host_i64(ids.reshape({-1}));
    const int64_t n = idl.numel();
    Tensor vals = torch::zeros({n}, torch::kInt64);
    Tensor found = torch::zeros({n}, torch::kInt32);
    if (n) qk_check(qk_attr_get(it->second, idl.data_ptr<int64_t>(), n, vals.data_ptr<int64_t>(), found.data_ptr<int>()));
    return {vals, found.to(torch::kBool)};
}

std::vector<std::string> QuakeIndex::attribute_names() {
    std::vector<std::string> names;
    if (!partition_manager_ || !partition_manager_->has_lists() || partition_manager_->store() != attrs_store_) return names;
    for (const auto &kv : attrs_) names.push_back(kv.first);
    return names;
}

shared_ptr<SearchFilter> QuakeIndex::make_filter_expr(const std::vector<std::vector<WhereTerm>> &any_of) {
    auto &cols = attributes("make_filter");
    const std::vector<std::vector<LoweredClause>> terms = lower_expr(any_of);
    std::vector<qk_expr_clause> cl;
    std::vector<int> sizes;
    for (const std::vector<LoweredClause> &term : terms) {
        for (const LoweredClause &c : term) {
            auto it = cols.find(c.name);
            if (it == cols.end()) throw std::runtime_error("[QuakeIndex::make_filter()] unknown attribute column '" + c.name + "'");
            cl.push_back(qk_expr_clause{it->second, c.op, c.a, c.b, c.values.empty() ? nullptr : c.values.data(), (int64_t)c.values.size()});
        }
        sizes.push_back((int)term.size());
    }
    auto f = std::make_shared<SearchFilter>();
    f->owner = attrs_store_;
    qk_check(qk_filter_create_expr(attrs_store_, cl.data(), sizes.data(), (int)sizes.size(), &f->h));
    return f;
}

shared_ptr<SearchFilter> QuakeIndex::make_filter_where(const std::vector<WhereTerm> &where) {
    // (a conjunction without sets keeps its own entry point and kernel)
    for (const WhereTerm &t : where)
        if (t.op == "in" || t.op == "not_in") return make_filter_expr({where});
    auto &cols = attributes("make_filter");
    std::vector<qk_clause> cl;
    for (const LoweredClause &c : lower_where(where)) {
        auto it = cols.find(c.name);
        if (it == cols.end()) throw std::runtime_error("[QuakeIndex::make_filter()] unknown attribute column '" + c.name + "'");
        cl.push_back(qk_clause{it->second, c.op, c.a, c.b});
    }
    auto f = std::make_shared<SearchFilter>();
    f->owner = attrs_store_;
    qk_check(qk_filter_create_where(attrs_store_, cl.data(), (int)cl.size(), &f->h));
    return f;
}

Tensor QuakeIndex::get(Tensor ids) {
    require_built("[QuakeIndex::get()] No partition manager. Index not built?");
    return partition_manager_->get(ids);
}

Tensor QuakeIndex::get_ids() {
    require_built("[QuakeIndex::get_ids()] No partition manager. Index not built?");
    return partition_manager_->get_ids();
}

shared_ptr<ModifyTimingInfo> QuakeIndex::add(Tensor x, Tensor ids) {
    require_built("[QuakeIndex::add()] No partition manager. Build the index first.");
    if (maintenance_policy_) maintenance_policy_->flush_hits();  // (hits are credited with the sizes of the moment they were scanned)
    auto info = partition_manager_->add(x, ids);
    publish();
    return info;
}

// what a modification left for the next search to do (list table upload, the parent's row-major copy) is done now: the queries
// after an add / remove / maintenance do not pay for it (qk_store_publish, include/quake_hip.h)
void QuakeIndex::publish() {
    if (!partition_manager_) return;
    qk_check(partition_manager_->lists().publish());
    if (parent_ && parent_->partition_manager_) qk_check(parent_->partition_manager_->lists().publish());
}

shared_ptr<ModifyTimingInfo> QuakeIndex::remove(Tensor ids) {
    require_built("[QuakeIndex::remove()] No partition manager. Build the index first.");
    if (maintenance_policy_) maintenance_policy_->flush_hits();
    auto info = partition_manager_->remove(ids);
    publish();
    return info;
}

shared_ptr<ModifyTimingInfo> QuakeIndex::modify(Tensor ids, Tensor x) {  // :147-150
    remove(ids);
    return add(x, ids);
}

void QuakeIndex::initialize_maintenance_policy(shared_ptr<MaintenancePolicyParams> p) {  // :152-155
    maintenance_policy_params_ = p;
    if (partition_manager_) {
        if (maintenance_policy_) maintenance_policy_->flush_hits();  // (hits recorded under the old policy reach it before it goes)
        const bool track = maintenance_policy_ && maintenance_policy_->track_hits_;
        maintenance_policy_ = std::make_shared<MaintenancePolicy>(partition_manager_, p);
        maintenance_policy_->track_hits_ = track;
        if (query_coordinator_) query_coordinator_->maintenance_policy_ = maintenance_policy_;
    }
}

void QuakeIndex::set_latency_profile(const std::string &path) {
    if (!maintenance_policy_ || !partition_manager_) throw std::runtime_error("[QuakeIndex::set_latency_profile()] No maintenance policy set.");
    auto lat = default_latency_estimator(partition_manager_->d(), path);
    maintenance_policy_->cost_estimator_ =
        std::make_shared<MaintenanceCostEstimator>(partition_manager_->d(), maintenance_policy_->params_->alpha, 10, lat);
}

void QuakeIndex::set_track_hits(bool on) {
    if (!maintenance_policy_) throw std::runtime_error("[QuakeIndex::set_track_hits()] No maintenance policy set.");
    maintenance_policy_->track_hits_ = on;
}

shared_ptr<MaintenanceTimingInfo> QuakeIndex::maintenance() {  // :157-163
    if (!maintenance_policy_) throw std::runtime_error("[QuakeIndex::maintenance()] No maintenance policy set.");
    auto info = maintenance_policy_->perform_maintenance();
    publish();
    return info;
}

void QuakeIndex::refine_partitions(Tensor partition_ids, int iterations) {
    require_built("[PartitionManager] refine_partitions: index not built");
    if (maintenance_policy_) maintenance_policy_->flush_hits();
    partition_manager_->refine_partitions(partition_ids, iterations);
}

bool QuakeIndex::validate() { return partition_manager_ && partition_manager_->validate(); }

int64_t QuakeIndex::ntotal() { return partition_manager_ ? partition_manager_->ntotal() : 0; }
int64_t QuakeIndex::nlist() { return partition_manager_ ? partition_manager_->nlist() : 0; }
int QuakeIndex::d() { return partition_manager_ ? partition_manager_->d() : 0; }

// on-disk layout of the reference (quake_index.cpp:170-267): <dir>/metadata.txt, <dir>/partitions, <dir>/parent/...
void QuakeIndex::save(const std::string &dir_path) {
    namespace fs = std::filesystem;
    require_built("Cannot save an index that was not built");
    if (fs::exists(dir_path) && !fs::is_directory(dir_path)) throw std::runtime_error("save path exists but is not a directory: " + dir_path);
    fs::create_directories(dir_path);
    {
        std::ofstream ofs((fs::path(dir_path) / "metadata.txt").string());
        if (!ofs.is_open()) throw std::runtime_error("Cannot open metadata file for writing");
        ofs << "metric=" << metric_ << "\n" << "level=" << current_level_ << "\n" << "ntotal=" << ntotal() << "\n" << "nlist=" << nlist() << "\n";
    }
    partition_manager_->save((fs::path(dir_path) / "partitions").string());
    if (parent_) parent_->save((fs::path(dir_path) / "parent").string());
}

void QuakeIndex::load(const std::string &dir_path, int n_workers) {
    namespace fs = std::filesystem;
    drop_attributes();  // (attributes are not persisted)
    if (!fs::exists(dir_path) || !fs::is_directory(dir_path)) throw std::runtime_error("Cannot load QuakeIndex, directory does not exist: " + dir_path);
    {
        std::ifstream ifs((fs::path(dir_path) / "metadata.txt").string());
        if (!ifs.is_open()) throw std::runtime_error("Cannot open metadata file for reading");
        std::string line;
        while (std::getline(ifs, line)) {
            auto pos = line.find('=');
            if (pos == std::string::npos) continue;
            std::string key = line.substr(0, pos), val = line.substr(pos + 1);
            if (key == "metric") metric_ = std::stoi(val);
            else if (key == "level") current_level_ = std::stoi(val);
        }
    }
    const std::string pdir = (fs::path(dir_path) / "parent").string();
    if (fs::exists(pdir) && fs::is_directory(pdir)) {
        parent_ = std::make_shared<QuakeIndex>(current_level_ + 1);
        parent_->load(pdir, n_workers);
    } else {
        parent_ = nullptr;
    }
    partition_manager_ = std::make_shared<PartitionManager>();
    partition_manager_->metric_ = metric_;
    partition_manager_->parent_ = parent_;
    partition_manager_->plan_workers(n_workers);
    partition_manager_->load((fs::path(dir_path) / "partitions").string());
    maintenance_policy_params_ = nullptr;  // load resets the policy to its defaults (:262-264)
    maintenance_policy_ = nullptr;
    make_coordinator(n_workers);
}

}  // namespace quake_amd
