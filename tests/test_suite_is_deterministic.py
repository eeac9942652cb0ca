"""The GPU suite must be a function of its inputs: a `-m gpu` test that asserts on a wall clock fails on a busy or a fresh box and
(`pytest -x`) hides every parity test collected after it -- round 5's driver run stopped at test 102 of 411 that way.  The reference's
own tests for this path are value assertions, none on time (test/cpp/query_coordinator.cpp:201-254, list_scanning.cpp:432-562).
Checked here, on the CPU, by reading the sources of every tests/*_gpu.py:
  * no `time` module, no perf_counter / monotonic / process_time;
  * device_profile_fn (the cost model's device clock) only with an injected `elapsed=`;
  * MaintenanceCostEstimator only with an injected latency grid (latency_estimator= / profile_fn=);
  * initialize_maintenance_policy without a cost estimator only where a recorded profile is set right after it
    (set_latency_profile) or in the functions listed below, whose assertions do not depend on what the policy decides;
  * the oracle-parity files are collected before the replays and property streams (conftest.collection_rank)."""
import ast
import glob
import os

import conftest

HERE = os.path.dirname(os.path.abspath(__file__))
GPU_FILES = sorted(glob.glob(os.path.join(HERE, "*_gpu.py")))

# function -> why a device-profiled (measured) cost model is harmless there
MEASURED_POLICY_OK = {
    ("test_bindings_gpu.py", "test_bindings_compiled_maintenance"): "asserts the index's invariants after maintenance, whatever it did",
    ("test_sharded_maintenance_gpu.py", "_world2_worker"): "asserts that the ranks hold the SAME grid (it is broadcast), not its values",
}
# GPU files whose stated place is the alphabetical middle block of conftest.collection_rank (after the named parity files, before
# the replays, soaks and property streams), and why
MIDDLE_BLOCK = {
    "test_kmeans_shapes_gpu.py": "an oracle-parity sweep of the k-means kernels: nothing collected after the first block depends on it",
}
CLOCKS = {"perf_counter", "perf_counter_ns", "monotonic", "monotonic_ns", "process_time", "time_ns"}


def _functions(tree):
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            yield node


def _call_name(call):
    f = call.func
    return f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else ""


def _outermost_function(tree, call):
    best = None
    for fn in tree.body:
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)) and any(n is call for n in ast.walk(fn)):
            best = fn
    return best


def test_there_are_gpu_files():
    assert len(GPU_FILES) >= 20


def test_no_wall_clock_in_gpu_tests():
    bad = []
    for path in GPU_FILES:
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import) and any(a.name.split(".")[0] in ("time", "timeit") for a in node.names):
                bad.append((os.path.basename(path), node.lineno, "import time"))
            if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] in ("time", "timeit"):
                bad.append((os.path.basename(path), node.lineno, "from time import"))
            if isinstance(node, ast.Attribute) and node.attr in CLOCKS:
                bad.append((os.path.basename(path), node.lineno, node.attr))
            if isinstance(node, ast.Name) and node.id in CLOCKS:
                bad.append((os.path.basename(path), node.lineno, node.id))
    assert not bad, bad


def test_cost_models_are_injected_in_gpu_tests():
    bad = []
    for path in GPU_FILES:
        base = os.path.basename(path)
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            name, kws = _call_name(node), {k.arg for k in node.keywords}
            if name == "device_profile_fn" and "elapsed" not in kws:
                bad.append((base, node.lineno, "device_profile_fn without elapsed="))
            if name == "MaintenanceCostEstimator" and not kws & {"latency_estimator", "profile_fn"}:
                bad.append((base, node.lineno, "MaintenanceCostEstimator profiles the device"))
            if name == "initialize_maintenance_policy" and "cost_estimator" not in kws and len(node.args) < 2:
                fn = _outermost_function(tree, node)
                calls_after = {_call_name(c) for c in ast.walk(fn) if isinstance(c, ast.Call)} if fn is not None else set()
                if "set_latency_profile" not in calls_after and (base, fn.name if fn else "") not in MEASURED_POLICY_OK:
                    bad.append((base, node.lineno, "policy on a measured cost model in " + (fn.name if fn else "<module>")))
    assert not bad, bad


def test_parity_files_are_collected_first():
    order = sorted((os.path.basename(p) for p in glob.glob(os.path.join(HERE, "test_*.py"))), key=conftest.collection_rank)
    pos = {n: i for i, n in enumerate(order)}
    parity = ["test_bench_parity_gpu.py", "test_scan_gpu.py", "test_scan_mixed_gpu.py", "test_kmeans_gpu.py", "test_assign_pf_gpu.py",
              "test_dense_fused_gpu.py", "test_dense_pf_gpu.py", "test_store_dynamic_gpu.py", "test_aps_gpu.py", "test_index_gpu.py",
              "test_group_gpu.py", "test_workers_gpu.py"]
    late = ["test_dynamic_workload_10m_gpu.py", "test_random_index_streams_gpu.py", "test_random_shapes_gpu.py", "test_full_size_gpu.py"]
    assert max(pos[p] for p in parity) < min(pos[l] for l in late), order
    gpu_unranked = [n for n in order if n.endswith("_gpu.py") and conftest.collection_rank(n)[0] == 1 and n not in MIDDLE_BLOCK]
    assert not gpu_unranked, gpu_unranked  # every GPU file has a stated place
    for n in MIDDLE_BLOCK:  # ... and a file stated to be in the middle block is there, ahead of every late file
        assert conftest.collection_rank(n)[0] == 1 and pos[n] < min(pos[l] for l in late), n
