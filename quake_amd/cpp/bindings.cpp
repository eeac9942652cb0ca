// bindings.cpp -- pybind11 module quake_amd._bindings: the classes, attributes and method names of the reference's
// `quake._bindings` (src/cpp/bindings/wrap.cpp:48-368), bound to the C++ host mirror in quake_index.h.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <algorithm>
#include <cctype>
#include <limits>
#include <sstream>

#include "quake_index.h"

namespace py = pybind11;
using namespace quake_amd;

namespace {
// the JSON-style one-line summaries of wrap.cpp's __repr__s: Repr().kv("a", 1).kv("b", true).str() -> {"a": 1, "b": true}
// (`trailing` reproduces the ", }" two of the reference's summaries end in)
class Repr {
    std::ostringstream os_;
    bool first_ = true;
    void key(const char *k) {
        os_ << (first_ ? "" : ", ") << '"' << k << "\": ";
        first_ = false;
    }

public:
    template <typename T>
    Repr &kv(const char *k, const T &v) {
        key(k);
        os_ << v;
        return *this;
    }
    Repr &kv(const char *k, bool v) {
        key(k);
        os_ << (v ? "true" : "false");
        return *this;
    }
    Repr &kv(const char *k, const std::string &v) {
        key(k);
        os_ << '"' << v << '"';
        return *this;
    }
    std::string str(bool trailing = false) const { return "{" + os_.str() + (trailing ? ", }" : "}"); }
};

// an operand of a where clause: a Python integer of any size (`mask`: values in [2^63, 2^64) are bit patterns)
WhereOperand parse_operand(const py::handle &h, bool mask) {
    if (!PyLong_Check(h.ptr()) || PyBool_Check(h.ptr())) {
        if (!PyIndex_Check(h.ptr()) || PyBool_Check(h.ptr()))
            throw std::runtime_error("[QuakeIndex::make_filter()] operands must be integers, got " + std::string(py::repr(h)));
    }
    py::object i = py::reinterpret_steal<py::object>(PyNumber_Index(h.ptr()));
    if (!i) throw py::error_already_set();
    WhereOperand o;
    int over = 0;
    o.v = (int64_t)PyLong_AsLongLongAndOverflow(i.ptr(), &over);
    if (over > 0 && mask) {
        const unsigned long long u = PyLong_AsUnsignedLongLong(i.ptr());
        if (!PyErr_Occurred()) {
            o.v = (int64_t)u;
            return o;
        }
        PyErr_Clear();
    }
    o.over = over;
    if (over) o.v = 0;
    return o;
}

std::vector<WhereTerm> parse_where(const py::object &where) {
    std::vector<WhereTerm> out;
    for (py::handle h : where) {
        if (!py::isinstance<py::tuple>(h) && !py::isinstance<py::list>(h))
            throw std::runtime_error("[QuakeIndex::make_filter()] a where clause is (name, op, a[, b]), got " + std::string(py::repr(h)));
        py::sequence cl = py::reinterpret_borrow<py::sequence>(h);
        if (cl.size() < 3 || cl.size() > 4 || !py::isinstance<py::str>(cl[0]) || !py::isinstance<py::str>(cl[1]))
            throw std::runtime_error("[QuakeIndex::make_filter()] a where clause is (name, op, a[, b]), got " + std::string(py::repr(h)));
        WhereTerm t;
        t.name = cl[0].cast<std::string>();
        t.op = cl[1].cast<std::string>();
        if (t.op == "in" || t.op == "not_in") {  // a value set (lower_expr)
            if (cl.size() != 3) throw std::runtime_error("[QuakeIndex::make_filter()] where op '" + t.op + "' takes 1 operand");
            py::object v = cl[2];
            if (py::isinstance<py::str>(v) || py::isinstance<py::bytes>(v) || py::isinstance<py::dict>(v) || !PySequence_Check(v.ptr()))
                throw std::runtime_error("[QuakeIndex::make_filter()] the operand of '" + t.op + "' must be a sequence of integers, got " +
                                         std::string(py::repr(v)));
            t.has_values = true;
            for (py::handle e : py::reinterpret_borrow<py::sequence>(v)) t.values.push_back(parse_operand(e, false));
            out.push_back(t);
            continue;
        }
        const bool mask = t.op == "any_bits" || t.op == "all_bits" || t.op == "no_bits";
        t.n_operands = (int)cl.size() - 2;
        t.a = parse_operand(cl[2], mask);
        if (cl.size() == 4) t.b = parse_operand(cl[3], false);
        out.push_back(t);
    }
    return out;
}

// where.py's _is_seq: indexable and sized, no string, no dict (not PySequence_Check: a tensor is indexable through the mapping
// protocol only)
bool is_edge_seq(const py::handle &v) {
    return !py::isinstance<py::str>(v) && !py::isinstance<py::bytes>(v) && !py::isinstance<py::dict>(v) && py::hasattr(v, "__getitem__") &&
           py::hasattr(v, "__len__");
}

// the edges of one column of facet_stats: None or a sequence of Python integers (where.py's _edge_list)
std::vector<WhereOperand> parse_edge_list(py::object v, const std::string &name) {
    std::vector<WhereOperand> out;
    if (v.is_none()) return out;
    if (py::hasattr(v, "tolist")) v = v.attr("tolist")();  // (a tensor, an array)
    if (!is_edge_seq(v))
        throw std::runtime_error("[QuakeIndex::facet_stats()] the edges of '" + name + "' must be a sequence of integers, got " +
                                 std::string(py::repr(v)));
    for (py::handle e : py::reinterpret_borrow<py::sequence>(v)) {
        if (PyBool_Check(e.ptr()) || !PyIndex_Check(e.ptr()))
            throw std::runtime_error("[QuakeIndex::facet_stats()] edges: operands must be integers, got " + std::string(py::repr(e)));
        out.push_back(parse_operand(e, false));
    }
    return out;
}

// `edges` of facet_stats -> one operand list per column: None, one sequence for every column, a dict name -> sequence, or a list
// with one sequence or None per column (where.py's lower_edges)
std::vector<std::vector<WhereOperand>> parse_edges(py::object edges, const std::vector<std::string> &names) {
    std::vector<std::vector<WhereOperand>> per(names.size());
    if (edges.is_none()) return per;
    if (py::isinstance<py::dict>(edges)) {
        py::dict d = edges.cast<py::dict>();
        for (auto kv : d) {
            const std::string k = py::str(kv.first).cast<std::string>();
            if (std::find(names.begin(), names.end(), k) == names.end())
                throw std::runtime_error("[QuakeIndex::facet_stats()] edges names '" + k + "', which is not one of the facet columns");
        }
        for (size_t c = 0; c < names.size(); c++)
            if (d.contains(py::str(names[c]))) per[c] = parse_edge_list(d[py::str(names[c])], names[c]);
        return per;
    }
    if (py::hasattr(edges, "tolist")) edges = edges.attr("tolist")();
    bool per_column = is_edge_seq(edges) && py::len(edges) > 0;
    std::vector<py::object> s;
    if (per_column)
        for (py::handle e : edges) {
            per_column = per_column && (e.is_none() || is_edge_seq(e));
            s.push_back(py::reinterpret_borrow<py::object>(e));
        }
    if (per_column) {
        if (s.size() != names.size())
            throw std::runtime_error("[QuakeIndex::facet_stats()] edges has " + std::to_string(s.size()) + " per-column entries for " +
                                     std::to_string(names.size()) + " columns");
        for (size_t c = 0; c < names.size(); c++) per[c] = parse_edge_list(s[c], names[c]);
        return per;
    }
    for (size_t c = 0; c < names.size(); c++) per[c] = parse_edge_list(edges, names[c]);
    return per;
}

// sum_hi * 2^64 + (sum_lo mod 2^64) of every (column, query) as Python ints: [C][Q]
py::list facet_stats_sums(const FacetStatsResult &r) {
    Tensor lo = r.sum_lo.cpu().contiguous(), hi = r.sum_hi.cpu().contiguous();
    const int64_t C = lo.size(0), Q = lo.size(1);
    const int64_t *pl = lo.data_ptr<int64_t>(), *ph = hi.data_ptr<int64_t>();
    py::list out;
    for (int64_t c = 0; c < C; c++) {
        py::list row;
        for (int64_t q = 0; q < Q; q++) {
            py::object h = py::int_(ph[c * Q + q]).attr("__lshift__")(64);
            row.append(h.attr("__add__")(py::int_((unsigned long long)pl[c * Q + q])));
        }
        out.append(row);
    }
    return out;
}
}  // namespace

PYBIND11_MODULE(_bindings, m) {
    m.def("lower_order",
          [](const std::vector<std::string> &columns, const std::string &order_by, int64_t k, bool descending, const std::string &missing) {
              const int flags = lower_order(columns, order_by, k, descending, missing);
              return py::make_tuple(order_by, k, flags);
          },
          py::arg("columns"), py::arg("order_by"), py::arg("k"), py::arg("descending") = false, py::arg("missing") = "exclude",
          "the arguments of ordered_search -> (column name, k, flags of qk_order_search); needs no device (where.py's lower_order)");
    m.def("lower_maxsim",
          [](const std::vector<std::string> &columns, const std::string &group_by, int64_t k, int64_t T, py::object n_tokens, py::object missing,
             const std::string &metric) {
              std::optional<std::vector<int64_t>> nt;
              if (!n_tokens.is_none()) nt = n_tokens.cast<std::vector<int64_t>>();
              std::optional<double> ms;
              if (!missing.is_none()) ms = missing.cast<double>();
              std::string m = metric;
              std::transform(m.begin(), m.end(), m.begin(), [](unsigned char ch) { return (char)std::tolower(ch); });
              const double mv = lower_maxsim(columns, group_by, k, T, nt, ms, m == "ip");
              py::object ntl = py::none();   // (a list, whatever sequence came in: what where.py returns)
              if (nt) ntl = py::cast(*nt);
              return py::make_tuple(group_by, k, T, ntl, mv);
          },
          py::arg("columns"), py::arg("group_by"), py::arg("k"), py::arg("T"), py::arg("n_tokens") = py::none(), py::arg("missing") = py::none(),
          py::arg("metric") = "ip",
          "the arguments of multi_vector_search -> (column name, k, T, n_tokens, missing); needs no device (where.py's lower_maxsim)");
    m.def("lower_diverse",
          [](int64_t k, int64_t fetch_k, double lambda_mult) {
              const float lambda = lower_diverse(k, fetch_k, lambda_mult);
              return py::make_tuple(k, fetch_k, (double)lambda);
          },
          py::arg("k"), py::arg("fetch_k"), py::arg("lambda_mult") = 0.5,
          "the arguments of diverse_search -> (k, fetch_k, lambda_mult rounded to float32); needs no device (where.py's lower_diverse)");
    m.doc() = "quake_amd: MI355X-native Quake search path (same surface as quake._bindings)";

    py::class_<QuakeIndex, std::shared_ptr<QuakeIndex>>(m, "QuakeIndex")
        .def(py::init<int>(), py::arg("current_level") = 0)
        .def("build", &QuakeIndex::build, "Build the index from vectors [n, d] and ids [n].")
        .def("search", &QuakeIndex::search, "Search the index for nearest neighbors.")
        .def("get", &QuakeIndex::get)
        .def("get_ids", &QuakeIndex::get_ids)
        .def("add", &QuakeIndex::add)
        .def("remove", &QuakeIndex::remove)
        .def("modify", &QuakeIndex::modify)
        .def("maintenance", &QuakeIndex::maintenance)
        .def("initialize_maintenance_policy", &QuakeIndex::initialize_maintenance_policy)
        .def("refine_partitions", &QuakeIndex::refine_partitions, py::arg("partition_ids"), py::arg("iterations") = 0)
        .def("make_filter", [](QuakeIndex &q, py::object ids, bool exclude, py::object where, py::object any_of) {
                 if ((int)!ids.is_none() + (int)!where.is_none() + (int)!any_of.is_none() != 1)
                     throw std::runtime_error("[QuakeIndex::make_filter()] exactly one of ids, where and any_of must be given");
                 if (!ids.is_none()) return q.make_filter(ids.cast<Tensor>(), exclude);
                 if (exclude) throw std::runtime_error("[QuakeIndex::make_filter()] exclude applies to ids, not to where (negate the clauses)");
                 if (!where.is_none()) return q.make_filter_where(parse_where(where));
                 std::vector<std::vector<WhereTerm>> terms;
                 if (PyObject *it = PyObject_GetIter(any_of.ptr())) {
                     Py_DECREF(it);
                 } else {
                     PyErr_Clear();
                     throw std::runtime_error("[QuakeIndex::make_filter()] any_of is a list of where lists, got " + std::string(py::repr(any_of)));
                 }
                 for (py::handle t : any_of) {
                     if (!py::isinstance<py::tuple>(t) && !py::isinstance<py::list>(t))
                         throw std::runtime_error("[QuakeIndex::make_filter()] a term is a list of where clauses, got " + std::string(py::repr(t)));
                     terms.push_back(parse_where(py::reinterpret_borrow<py::object>(t)));
                 }
                 return q.make_filter_expr(terms);
             }, py::arg("ids") = py::none(), py::arg("exclude") = false, py::arg("where") = py::none(), py::arg("any_of") = py::none(),
             "extension: a SearchFilter for SearchParams.filter -- over vector ids (ids, exclude) or a predicate over the attribute "
             "columns: where = [(name, op, a[, b]) | (name, 'in' | 'not_in', [v, ...]), ...], all of which must hold; any_of = a list of "
             "such lists, one of which must hold")
        .def("set_attribute", &QuakeIndex::set_attribute, py::arg("name"), py::arg("ids"), py::arg("values"),
             "extension: int64 values keyed by vector id in column `name` (created on first use)")
        .def("unset_attribute", &QuakeIndex::unset_attribute, py::arg("name"), py::arg("ids"))
        .def("get_attribute", &QuakeIndex::get_attribute, py::arg("name"), py::arg("ids"), "(values int64 [n], found bool [n])")
        .def("attribute_names", &QuakeIndex::attribute_names)
        .def("search_after", &QuakeIndex::search_after, py::arg("x"), py::arg("search_params"), py::arg("cursor") = nullptr,
             "extension: the page of search_params.k results behind `cursor` (a SearchResult.cursor of the same queries; None: from the "
             "start); the result's .cursor continues behind it.  Records no hits for maintenance")
        .def("range_search", &QuakeIndex::range_search, py::arg("x"), py::arg("radius"), py::arg("search_params"),
             "extension: every vector of the nprobe nearest partitions within `radius` of each query (lims, ids, distances)")
        .def("grouped_search", &QuakeIndex::grouped_search, py::arg("x"), py::arg("group_by"), py::arg("search_params"),
             py::arg("group_size") = py::none(),
             "extension: the k best groups of attribute column `group_by` per query, every group by its best vector (ids, distances, groups); "
             "group_size = m: by its m best vectors, ids / distances [Q, k, m]")
        .def("facet_counts",
             [](QuakeIndex &self, Tensor x, py::object facet_by, shared_ptr<SearchParams> sp, py::object radius, int n_values) {
                 std::vector<std::string> names;
                 if (py::isinstance<py::str>(facet_by)) names.push_back(facet_by.cast<std::string>());
                 else names = facet_by.cast<std::vector<std::string>>();
                 std::optional<float> r;
                 if (!radius.is_none()) r = radius.cast<float>();
                 return self.facet_counts(x, names, sp, r, n_values);
             },
             py::arg("x"), py::arg("facet_by"), py::arg("search_params"), py::arg("radius") = py::none(), py::arg("n_values") = 10,
             "extension: per query, the value counts of the attribute columns `facet_by` (a name or a list of names) over the vectors "
             "range_search returns for the same arguments (radius None: every vector of the probed partitions): values, counts, "
             "distinct, missing, totals")
        .def("facet_stats",
             [](QuakeIndex &self, Tensor x, py::object facet_by, shared_ptr<SearchParams> sp, py::object radius, py::object edges) {
                 std::vector<std::string> names;
                 if (py::isinstance<py::str>(facet_by)) names.push_back(facet_by.cast<std::string>());
                 else names = facet_by.cast<std::vector<std::string>>();
                 std::optional<float> r;
                 if (!radius.is_none()) r = radius.cast<float>();
                 // (the edges are parsed and checked where the Python mirror checks them: behind the refusals and the column lookup)
                 return self.facet_stats(x, names, sp, r, FacetEdgesFn([&]() { return lower_edges(names, parse_edges(edges, names)); }));
             },
             py::arg("x"), py::arg("facet_by"), py::arg("search_params"), py::arg("radius") = py::none(), py::arg("edges") = py::none(),
             "extension: per query, count / missing / min / max / exact sum / histogram of the attribute columns `facet_by` (a name or "
             "a list of names) over the vectors range_search returns for the same arguments; edges: None, one ascending sequence of "
             "integers for all columns, or a dict name -> sequence")
        .def("ordered_search",
             [](QuakeIndex &self, Tensor x, const std::string &order_by, shared_ptr<SearchParams> sp, py::object radius, bool descending,
                const std::string &missing) {
                 std::optional<float> r;
                 if (!radius.is_none()) r = radius.cast<float>();
                 return self.ordered_search(x, order_by, sp, r, descending, missing);
             },
             py::arg("x"), py::arg("order_by"), py::arg("search_params"), py::arg("radius") = py::none(), py::arg("descending") = false,
             py::arg("missing") = "exclude",
             "extension: per query, the search_params.k first of the vectors range_search returns for the same arguments by the "
             "attribute column `order_by` (ascending, or descending), ties to the nearer vector, then to the smaller id; missing: "
             "'exclude' or 'last'")
        .def("multi_vector_search",
             [](QuakeIndex &self, Tensor x, const std::string &group_by, shared_ptr<SearchParams> sp, py::object radius, py::object n_tokens,
                py::object missing) {
                 std::optional<float> r;
                 if (!radius.is_none()) r = radius.cast<float>();
                 std::optional<std::vector<int64_t>> nt;
                 if (!n_tokens.is_none()) {
                     if (py::hasattr(n_tokens, "tolist")) n_tokens = n_tokens.attr("reshape")(-1).attr("tolist")();
                     nt = n_tokens.cast<std::vector<int64_t>>();
                 }
                 std::optional<double> ms;
                 if (!missing.is_none()) ms = missing.cast<double>();
                 return self.multi_vector_search(x, group_by, sp, r, nt, ms);
             },
             py::arg("x"), py::arg("group_by"), py::arg("search_params"), py::arg("radius") = py::none(), py::arg("n_tokens") = py::none(),
             py::arg("missing") = py::none(),
             "extension: multi-vector (late interaction) search -- x [L, T, d]; per logical query the search_params.k best values of the "
             "attribute column `group_by` by the sum over the query's vectors of the best vector range_search returns among the value's "
             "vectors; n_tokens [L]: the vectors of each query that take part; missing: the term of a vector without a match (None: 0 "
             "for the inner product)")
        .def("diverse_search", &QuakeIndex::diverse_search, py::arg("x"), py::arg("search_params"), py::arg("fetch_k"),
             py::arg("lambda_mult") = 0.5,
             "extension: per query, search_params.k of its fetch_k nearest vectors (what search() returns with k = fetch_k) chosen "
             "greedily by maximal marginal relevance; lambda_mult in [0, 1]: 1 is the plain top-k, 0 diversity alone")
        .def("save", &QuakeIndex::save)
        .def("load", &QuakeIndex::load, py::arg("path"), py::arg("n_workers") = 0)
        .def("ntotal", &QuakeIndex::ntotal)
        .def("nlist", &QuakeIndex::nlist)
        .def("d", &QuakeIndex::d)
        .def("set_track_hits", &QuakeIndex::set_track_hits, "Record the partitions each query probes, so that maintenance() can act.")
        .def("set_latency_profile", &QuakeIndex::set_latency_profile, "Scan-latency grid of the maintenance cost model from a CSV (reference profile format).")
        .def("validate", &QuakeIndex::validate)
        .def_readonly("parent", &QuakeIndex::parent_)
        .def_readonly("partition_manager", &QuakeIndex::partition_manager_)
        .def_readonly("query_coordinator", &QuakeIndex::query_coordinator_)
        .def_readonly("current_level", &QuakeIndex::current_level_)
        .def("__repr__", [](const QuakeIndex &q) { return Repr().kv("current_level", q.current_level_).str(true); });  // wrap.cpp:122-128

    // the collaborators the reference's own tests reach into (test/cpp/quake_index.cpp:50-54, query_coordinator.cpp:42,96)
    py::class_<PartitionManager, std::shared_ptr<PartitionManager>>(m, "PartitionManager")
        .def("ntotal", &PartitionManager::ntotal)
        .def("nlist", &PartitionManager::nlist)
        .def("d", &PartitionManager::d)
        .def("get_partition_ids", &PartitionManager::get_partition_ids)
        .def("get_partition_sizes", [](PartitionManager &pm, torch::Tensor pids) { return pm.get_partition_sizes(pids); })
        .def("get_ids", &PartitionManager::get_ids)
        .def("validate", &PartitionManager::validate)
        // workers = GPUs: the partition -> worker map (partition_manager.h:170-187)
        .def("distribute_partitions", &PartitionManager::distribute_partitions)
        .def("get_partition_core_id", &PartitionManager::get_partition_core_id)
        .def("set_partition_core_id", &PartitionManager::set_partition_core_id)
        .def("num_workers", &PartitionManager::num_workers, "Members of the device group the partitions are distributed over (0: one store).");

    py::class_<QueryCoordinator, std::shared_ptr<QueryCoordinator>>(m, "QueryCoordinator")
        .def("search", &QueryCoordinator::search)
        .def("scan_partitions", &QueryCoordinator::scan_partitions)
        .def("serial_scan", &QueryCoordinator::serial_scan)
        .def("batched_serial_scan", &QueryCoordinator::batched_serial_scan)
        .def("worker_scan", &QueryCoordinator::worker_scan)
        .def("initialize_workers", &QueryCoordinator::initialize_workers)  // query_coordinator.h:150-160
        .def("shutdown_workers", &QueryCoordinator::shutdown_workers)
        .def_readwrite("device_timing", &QueryCoordinator::device_timing_)  // query_coordinator.h: counters for device-tensor searches
        .def_readonly("workers_initialized", &QueryCoordinator::workers_initialized_)
        .def_readonly("num_workers", &QueryCoordinator::num_workers_);

    // list_scanning.h seam: one query (or a block of queries) against one raw list
    m.def("batched_scan_list", [](torch::Tensor queries, torch::Tensor list_vecs, torch::Tensor list_ids, int k, std::string metric) {
        torch::Tensor q = queries.to(torch::kCPU, torch::kFloat32).contiguous(), v = list_vecs.to(torch::kCPU, torch::kFloat32).contiguous();
        torch::Tensor ids = list_ids.defined() && list_ids.numel() ? list_ids.to(torch::kCPU, torch::kInt64).contiguous() : torch::Tensor();
        const MetricType mt = (MetricType)str_to_metric_type(metric);
        auto bufs = create_buffers((int)q.size(0), k, mt == METRIC_INNER_PRODUCT);
        batched_scan_list(q.data_ptr<float>(), v.data_ptr<float>(), ids.defined() ? ids.data_ptr<int64_t>() : nullptr, (int)q.size(0),
                          (int)v.size(0), (int)q.size(1), bufs, mt);
        return buffers_to_tensor(bufs);
    }, py::arg("queries"), py::arg("list_vecs"), py::arg("list_ids"), py::arg("k"), py::arg("metric") = "l2");

    py::class_<IndexBuildParams, std::shared_ptr<IndexBuildParams>>(m, "IndexBuildParams")
        .def(py::init<>())
        .def_readwrite("nlist", &IndexBuildParams::nlist)
        .def_readwrite("niter", &IndexBuildParams::niter)
        .def_readwrite("metric", &IndexBuildParams::metric)
        .def_readwrite("num_workers", &IndexBuildParams::num_workers)
        .def("__repr__", [](const IndexBuildParams &p) {  // wrap.cpp:141-150
            return Repr().kv("nlist", p.nlist).kv("niter", p.niter).kv("metric", p.metric).kv("num_workers", p.num_workers).str();
        });

    py::class_<SearchFilter, std::shared_ptr<SearchFilter>>(m, "SearchFilter")
        .def_readonly("exclude", &SearchFilter::exclude)
        .def("info", [](const SearchFilter &f) {  // qk_filter_info
            int64_t n = 0, ra = 0, rb = 0, db = 0;
            uint64_t ver = 0;
            qk_check(qk_filter_info(f.h, &n, &ra, &ver, &rb, &db));
            py::dict d;
            d["n_ids"] = n;
            d["rows_allowed"] = ra;
            d["store_version"] = ver;
            d["rebuilds"] = rb;
            d["device_bytes"] = db;
            return d;
        });

    py::class_<SearchParams, std::shared_ptr<SearchParams>>(m, "SearchParams")
        .def(py::init<>())
        .def_readwrite("k", &SearchParams::k)
        .def_readwrite("nprobe", &SearchParams::nprobe)
        .def_readwrite("recall_target", &SearchParams::recall_target)
        .def_readwrite("num_threads", &SearchParams::num_threads)
        .def_readwrite("batched_scan", &SearchParams::batched_scan)
        .def_readwrite("use_precomputed", &SearchParams::use_precomputed)
        .def_readwrite("initial_search_fraction", &SearchParams::initial_search_fraction)
        .def_readwrite("recompute_threshold", &SearchParams::recompute_threshold)
        .def_readwrite("aps_flush_period_us", &SearchParams::aps_flush_period_us)
        .def_readwrite("filter", &SearchParams::filter)  // extension; not part of the summary below
        .def_readwrite("filters", &SearchParams::filters)  // extension: one filter per query, with query_filter
        .def_property(
            "query_filter",
            [](const SearchParams &p) -> py::object {
                if (!p.query_filter.defined()) return py::none();
                return py::cast(p.query_filter);
            },
            [](SearchParams &p, py::object v) { p.query_filter = v.is_none() ? Tensor() : v.cast<Tensor>(); })
        .def_readwrite("max_nprobe", &SearchParams::max_nprobe)  // extension: adaptive probing under a filter; not in the summary
        .def_readwrite("filter_min_candidates", &SearchParams::filter_min_candidates)
        .def_readwrite("filter_exact_rows", &SearchParams::filter_exact_rows)  // extension: exact search under a selective filter
        .def_readwrite("filters_exact_rows", &SearchParams::filters_exact_rows)  // extension: the same, one filter per query
        .def_readwrite("filters_exact_pool_rows", &SearchParams::filters_exact_pool_rows)
        .def("__repr__", [](const SearchParams &p) {  // wrap.cpp:173-186
            return Repr().kv("k", p.k).kv("nprobe", p.nprobe).kv("recall_target", p.recall_target).kv("batched_scan", p.batched_scan)
                .kv("use_precomputed", p.use_precomputed).kv("initial_search_fraction", p.initial_search_fraction)
                .kv("recompute_threshold", p.recompute_threshold).kv("aps_flush_period_us", p.aps_flush_period_us).str();
        });

    py::class_<MaintenancePolicyParams, std::shared_ptr<MaintenancePolicyParams>>(m, "MaintenancePolicyParams")
        .def(py::init<>())
        .def_readwrite("maintenance_policy", &MaintenancePolicyParams::maintenance_policy)
        .def_readwrite("window_size", &MaintenancePolicyParams::window_size)
        .def_readwrite("refinement_radius", &MaintenancePolicyParams::refinement_radius)
        .def_readwrite("refinement_iterations", &MaintenancePolicyParams::refinement_iterations)
        .def_readwrite("min_partition_size", &MaintenancePolicyParams::min_partition_size)
        .def_readwrite("alpha", &MaintenancePolicyParams::alpha)
        .def_readwrite("enable_split_rejection", &MaintenancePolicyParams::enable_split_rejection)
        .def_readwrite("enable_delete_rejection", &MaintenancePolicyParams::enable_delete_rejection)
        .def_readwrite("delete_threshold_ns", &MaintenancePolicyParams::delete_threshold_ns)
        .def_readwrite("split_threshold_ns", &MaintenancePolicyParams::split_threshold_ns)
        .def_readwrite("split_after_delete_rejection", &MaintenancePolicyParams::split_after_delete_rejection)  // extension, common.h
        .def("__repr__", [](const MaintenancePolicyParams &p) {  // wrap.cpp:211-226
            return Repr().kv("maintenance_policy", p.maintenance_policy).kv("window_size", p.window_size)
                .kv("refinement_radius", p.refinement_radius).kv("refinement_iterations", p.refinement_iterations)
                .kv("min_partition_size", p.min_partition_size).kv("alpha", p.alpha)
                .kv("enable_split_rejection", p.enable_split_rejection).kv("enable_delete_rejection", p.enable_delete_rejection)
                .kv("delete_threshold_ns", p.delete_threshold_ns).kv("split_threshold_ns", p.split_threshold_ns).str(true);
        });

    py::class_<MaintenanceTimingInfo, std::shared_ptr<MaintenanceTimingInfo>>(m, "MaintenanceTimingInfo")
        .def_readonly("total_time_us", &MaintenanceTimingInfo::total_time_us)
        .def_readonly("split_time_us", &MaintenanceTimingInfo::split_time_us)
        .def_readonly("delete_time_us", &MaintenanceTimingInfo::delete_time_us)
        .def_readonly("split_refine_time_us", &MaintenanceTimingInfo::split_refine_time_us)
        .def_readonly("delete_refine_time_us", &MaintenanceTimingInfo::delete_refine_time_us)
        .def_readonly("n_splits", &MaintenanceTimingInfo::n_splits)
        .def_readonly("n_deletes", &MaintenanceTimingInfo::n_deletes)
        .def("__repr__", [](const MaintenanceTimingInfo &t) {  // wrap.cpp:244-256
            return Repr().kv("total_time_us", t.total_time_us).kv("split_time_us", t.split_time_us).kv("delete_time_us", t.delete_time_us)
                .kv("split_refine_time_us", t.split_refine_time_us).kv("delete_refine_time_us", t.delete_refine_time_us)
                .kv("n_splits", t.n_splits).kv("n_deletes", t.n_deletes).str();
        });

    py::class_<BuildTimingInfo, std::shared_ptr<BuildTimingInfo>>(m, "BuildTimingInfo")
        .def_readonly("n_vectors", &BuildTimingInfo::n_vectors)
        .def_readonly("n_clusters", &BuildTimingInfo::n_clusters)
        .def_readonly("d", &BuildTimingInfo::d)
        .def_readonly("train_time_us", &BuildTimingInfo::train_time_us)
        .def_readonly("assign_time_us", &BuildTimingInfo::assign_time_us)
        .def_readonly("total_time_us", &BuildTimingInfo::total_time_us)
        .def_readonly("code_size", &BuildTimingInfo::code_size)        // wrap.cpp:332-335 (PQ fields: -1, no PQ on this path)
        .def_readonly("n_codebooks", &BuildTimingInfo::num_codebooks)
        .def("__repr__", [](const BuildTimingInfo &b) {  // wrap.cpp:338-350
            return Repr().kv("total_time_us", b.total_time_us).kv("assign_time_us", b.assign_time_us).kv("train_time_us", b.train_time_us)
                .kv("d", b.d).kv("code_size", b.code_size).kv("n_codebooks", b.num_codebooks).kv("n_vectors", b.n_vectors).str();
        });

    py::class_<ModifyTimingInfo, std::shared_ptr<ModifyTimingInfo>>(m, "ModifyTimingInfo")
        .def_readonly("n_vectors", &ModifyTimingInfo::n_vectors)
        .def_readonly("modify_count", &ModifyTimingInfo::n_vectors)  // alias, wrap.cpp:264
        .def_readonly("input_validation_time_us", &ModifyTimingInfo::input_validation_time_us)
        .def_readonly("find_partition_time_us", &ModifyTimingInfo::find_partition_time_us)
        .def_readonly("modify_time_us", &ModifyTimingInfo::modify_time_us)
        .def_readonly("maintenance_time_us", &ModifyTimingInfo::maintenance_time_us)
        .def("__repr__", [](const ModifyTimingInfo &t) {  // wrap.cpp:267-276
            return Repr().kv("modify_count", t.n_vectors).kv("input_validation_time_us", t.input_validation_time_us)
                .kv("modify_time_us", t.modify_time_us).kv("find_partition_time_us", t.find_partition_time_us).str();
        });

    py::class_<SearchTimingInfo, std::shared_ptr<SearchTimingInfo>>(m, "SearchTimingInfo")
        .def(py::init<>())
        .def_readwrite("n_queries", &SearchTimingInfo::n_queries)
        .def_readwrite("n_clusters", &SearchTimingInfo::n_clusters)
        .def_readwrite("partitions_scanned", &SearchTimingInfo::partitions_scanned)
        .def_readwrite("search_params", &SearchTimingInfo::search_params)
        .def_readwrite("parent_info", &SearchTimingInfo::parent_info)
        .def_readwrite("buffer_init_time_ns", &SearchTimingInfo::buffer_init_time_ns)
        .def_readwrite("job_enqueue_time_ns", &SearchTimingInfo::job_enqueue_time_ns)
        .def_readwrite("boundary_distance_time_ns", &SearchTimingInfo::boundary_distance_time_ns)
        .def_readwrite("job_wait_time_ns", &SearchTimingInfo::job_wait_time_ns)
        .def_readwrite("result_aggregate_time_ns", &SearchTimingInfo::result_aggregate_time_ns)
        .def_readwrite("total_time_ns", &SearchTimingInfo::total_time_ns)
        .def("__repr__", [](const SearchTimingInfo &t) {  // wrap.cpp:303-320
            Repr r;
            r.kv("total_time_ns", t.total_time_ns).kv("buffer_init_time_ns", t.buffer_init_time_ns)
                .kv("job_enqueue_time_ns", t.job_enqueue_time_ns).kv("boundary_distance_time_ns", t.boundary_distance_time_ns)
                .kv("job_wait_time_ns", t.job_wait_time_ns).kv("result_aggregate_time_ns", t.result_aggregate_time_ns);
            if (t.parent_info) r.kv("parent_scan_time_ns", t.parent_info->total_time_ns);
            return r.kv("n_queries", t.n_queries).kv("n_clusters", t.n_clusters).kv("partitions_scanned", t.partitions_scanned).str();
        });

    py::class_<RangeSearchResult, std::shared_ptr<RangeSearchResult>>(m, "RangeSearchResult")
        .def(py::init<>())
        .def_readwrite("lims", &RangeSearchResult::lims)
        .def_readwrite("ids", &RangeSearchResult::ids)
        .def_readwrite("distances", &RangeSearchResult::distances)
        .def_readwrite("timing_info", &RangeSearchResult::timing_info);

    py::class_<GroupedSearchResult, std::shared_ptr<GroupedSearchResult>>(m, "GroupedSearchResult")
        .def(py::init<>())
        .def_readwrite("ids", &GroupedSearchResult::ids)
        .def_readwrite("distances", &GroupedSearchResult::distances)
        .def_readwrite("groups", &GroupedSearchResult::groups)
        .def_readwrite("timing_info", &GroupedSearchResult::timing_info);

    py::class_<FacetResult, std::shared_ptr<FacetResult>>(m, "FacetResult")
        .def(py::init<>())
        .def_readwrite("values", &FacetResult::values)
        .def_readwrite("counts", &FacetResult::counts)
        .def_readwrite("distinct", &FacetResult::distinct)
        .def_readwrite("missing", &FacetResult::missing)
        .def_readwrite("totals", &FacetResult::totals)
        .def_readwrite("columns", &FacetResult::columns)
        .def_readwrite("timing_info", &FacetResult::timing_info);

    py::class_<FacetStatsResult, std::shared_ptr<FacetStatsResult>>(m, "FacetStatsResult")
        .def(py::init<>())
        .def_readwrite("count", &FacetStatsResult::count)
        .def_readwrite("missing", &FacetStatsResult::missing)
        .def_readwrite("min", &FacetStatsResult::min)
        .def_readwrite("max", &FacetStatsResult::max)
        .def_readwrite("sum_lo", &FacetStatsResult::sum_lo)
        .def_readwrite("sum_hi", &FacetStatsResult::sum_hi)
        .def_readwrite("histogram", &FacetStatsResult::histogram)
        .def_readwrite("totals", &FacetStatsResult::totals)
        .def_readwrite("columns", &FacetStatsResult::columns)
        .def_readwrite("edges", &FacetStatsResult::edges)
        .def_readwrite("timing_info", &FacetStatsResult::timing_info)
        .def("sums", &facet_stats_sums, "[C][Q] exact Python ints: sum_hi * 2**64 + (sum_lo mod 2**64)")
        .def("means",
             [](const FacetStatsResult &r) {  // float64 [C, Q], NaN where count == 0 (Python's own int / int division)
                 py::list sums = facet_stats_sums(r), rows;
                 Tensor cnt = r.count.cpu().contiguous();
                 const int64_t C = cnt.size(0), Q = cnt.size(1);
                 const int64_t *pc = cnt.data_ptr<int64_t>();
                 for (int64_t c = 0; c < C; c++) {
                     py::list row, srow = sums[c].cast<py::list>();
                     for (int64_t q = 0; q < Q; q++) {
                         if (pc[c * Q + q] == 0) row.append(py::float_(std::numeric_limits<double>::quiet_NaN()));
                         else row.append(srow[q].attr("__truediv__")(py::int_(pc[c * Q + q])));
                     }
                     rows.append(row);
                 }
                 py::object np = py::module_::import("numpy");
                 return np.attr("array")(rows, py::arg("dtype") = "float64").attr("reshape")(C, -1);
             },
             "[C, Q] float64 numpy array of sum / count, NaN where count == 0");

    py::class_<MultiVectorSearchResult, std::shared_ptr<MultiVectorSearchResult>>(m, "MultiVectorSearchResult")
        .def(py::init<>())
        .def_readwrite("groups", &MultiVectorSearchResult::groups)
        .def_readwrite("scores", &MultiVectorSearchResult::scores)
        .def_readwrite("matched", &MultiVectorSearchResult::matched)
        .def_readwrite("n_groups", &MultiVectorSearchResult::n_groups)
        .def_readwrite("hits", &MultiVectorSearchResult::hits)
        .def_readwrite("column", &MultiVectorSearchResult::column)
        .def_readwrite("timing_info", &MultiVectorSearchResult::timing_info);
    py::class_<OrderedSearchResult, std::shared_ptr<OrderedSearchResult>>(m, "OrderedSearchResult")
        .def(py::init<>())
        .def_readwrite("ids", &OrderedSearchResult::ids)
        .def_readwrite("distances", &OrderedSearchResult::distances)
        .def_readwrite("values", &OrderedSearchResult::values)
        .def_readwrite("counts", &OrderedSearchResult::counts)
        .def_readwrite("missing", &OrderedSearchResult::missing)
        .def_readwrite("totals", &OrderedSearchResult::totals)
        .def_readwrite("column", &OrderedSearchResult::column)
        .def_readwrite("timing_info", &OrderedSearchResult::timing_info);

    py::class_<DiverseSearchResult, std::shared_ptr<DiverseSearchResult>>(m, "DiverseSearchResult")
        .def(py::init<>())
        .def_readwrite("ids", &DiverseSearchResult::ids)
        .def_readwrite("distances", &DiverseSearchResult::distances)
        .def_readwrite("ranks", &DiverseSearchResult::ranks)
        .def_readwrite("timing_info", &DiverseSearchResult::timing_info);

    py::class_<SearchCursor, std::shared_ptr<SearchCursor>>(m, "SearchCursor")
        .def(py::init([](py::object keys, py::object ids) {  // (None: left undefined -- search_after refuses such a cursor)
                 auto c = std::make_shared<SearchCursor>();
                 if (!keys.is_none()) c->keys = keys.cast<Tensor>();
                 if (!ids.is_none()) c->ids = ids.cast<Tensor>();
                 return c;
             }), py::arg("keys"), py::arg("ids"))
        .def_property("keys", [](const SearchCursor &c) -> py::object { return c.keys.defined() ? py::cast(c.keys) : py::none(); },
                      [](SearchCursor &c, py::object v) { c.keys = v.is_none() ? Tensor() : v.cast<Tensor>(); })
        .def_property("ids", [](const SearchCursor &c) -> py::object { return c.ids.defined() ? py::cast(c.ids) : py::none(); },
                      [](SearchCursor &c, py::object v) { c.ids = v.is_none() ? Tensor() : v.cast<Tensor>(); })
        .def("__len__", [](const SearchCursor &c) { return c.ids.defined() ? c.ids.numel() : (int64_t)0; });

    py::class_<SearchResult, std::shared_ptr<SearchResult>>(m, "SearchResult")
        .def(py::init<>())
        .def_readwrite("ids", &SearchResult::ids)
        .def_readwrite("distances", &SearchResult::distances)
        .def_readwrite("timing_info", &SearchResult::timing_info)
        .def_property(
            "nprobed",  // extension: int32 [Q] under SearchParams.max_nprobe, else None
            [](const SearchResult &r) -> py::object {
                if (!r.nprobed.defined()) return py::none();
                return py::cast(r.nprobed);
            },
            [](SearchResult &r, py::object v) { r.nprobed = v.is_none() ? Tensor() : v.cast<Tensor>(); })
        .def_property(
            "exact",  // extension: True / False on a search that consulted SearchParams.filter_exact_rows, else None
            [](const SearchResult &r) -> py::object {
                if (r.exact < 0) return py::none();
                return py::bool_(r.exact == 1);
            },
            [](SearchResult &r, py::object v) { r.exact = v.is_none() ? -1 : (v.cast<bool>() ? 1 : 0); })
        .def_property(
            "exact_mask",  // extension: bool [Q], the queries answered exactly under SearchParams.filters_exact_rows, else None
            [](const SearchResult &r) -> py::object { return r.exact_mask.defined() ? py::cast(r.exact_mask) : py::none(); },
            [](SearchResult &r, py::object v) { r.exact_mask = v.is_none() ? Tensor() : v.cast<Tensor>(); })
        .def_readwrite("cursor", &SearchResult::cursor);  // extension: the SearchCursor behind a search_after page, else None
}
