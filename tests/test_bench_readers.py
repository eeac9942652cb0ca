"""bench.py --sift-dir: the TEXMEX .fvecs / .ivecs layout (int32 dimension in front of every vector; the reference reads the same
files in src/python/utils.py and datasets/ann_datasets.py:44) read back exactly, and malformed files refused."""
import numpy as np
import pytest

import bench as B


def _write_vecs(path, a):
    a = np.ascontiguousarray(a)
    rec = np.empty((a.shape[0], 4 + a.shape[1] * a.dtype.itemsize), np.uint8)
    rec[:, :4] = np.array([a.shape[1]], np.int32).view(np.uint8)
    rec[:, 4:] = a.view(np.uint8).reshape(a.shape[0], -1)
    rec.tofile(path)


def test_vecs_round_trip_and_directory(tmp_path):
    rng = np.random.default_rng(0)
    base = rng.standard_normal((37, 128)).astype(np.float32)
    query = rng.standard_normal((5, 128)).astype(np.float32)
    gt = rng.integers(0, 37, (5, 100)).astype(np.int32)
    _write_vecs(tmp_path / "sift_base.fvecs", base)
    _write_vecs(tmp_path / "sift_query.fvecs", query)
    _write_vecs(tmp_path / "sift_groundtruth.ivecs", gt)
    b, q, g = B.load_sift_dir(str(tmp_path))
    assert b.dtype == np.float32 and np.array_equal(b.view(np.uint32), base.view(np.uint32))
    assert np.array_equal(q, query) and g.dtype == np.int32 and np.array_equal(g, gt)
    (tmp_path / "sift_groundtruth.ivecs").unlink()
    assert B.load_sift_dir(str(tmp_path))[2] is None  # the ground-truth file is optional (the run computes its own)


def test_malformed_vecs_are_refused(tmp_path):
    p = tmp_path / "x_base.fvecs"
    np.array([128, 1, 2, 3], np.int32).tofile(p)  # says d = 128, holds 3 components
    with pytest.raises(SystemExit):
        B.read_vecs(str(p), np.float32)
    p.write_bytes(b"")
    with pytest.raises(SystemExit):
        B.read_vecs(str(p), np.float32)


@pytest.mark.gpu
def test_bench_runs_on_a_dataset_directory(tmp_path):
    """`bench.py --sift-dir DIR`: the headline workload on the files of a TEXMEX-layout directory (here a 200k x 128 integer-valued
    stand-in written by this test), end to end on the GPU: one JSON line, `data` says where the vectors came from, recall at the
    target, parity against the oracle enforced inside the run (bench.py exits non-zero otherwise)."""
    import json
    import os
    import subprocess
    import sys
    rng = np.random.default_rng(3)
    cent = rng.integers(0, 200, (256, 128)).astype(np.float32)
    base = np.clip(cent[rng.integers(0, 256, 200000)] + rng.normal(0, 12, (200000, 128)), 0, 255).round().astype(np.float32)
    query = np.clip(cent[rng.integers(0, 256, 2048)] + rng.normal(0, 12, (2048, 128)), 0, 255).round().astype(np.float32)
    _write_vecs(tmp_path / "sift_base.fvecs", base)
    _write_vecs(tmp_path / "sift_query.fvecs", query)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--sift-dir", str(tmp_path), "--nlist", "256", "--batch", "512",
                        "--steps", "5", "--warmup", "2", "--settle", "5", "--full", "--no-extra", "--no-pmc", "--cpu-seconds", "1", "--inflight", "1"],
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["data"] == "dataset files (--sift-dir)" and line["config"]["nvec"] == 200000 and line["config"]["dim"] == 128
    assert line["config"]["recall_at_k"] >= 0.9 and line["value"] > 0 and line["cpu_baseline"]["ids_equal_to_gpu_frac"] == 1.0


def test_dump_outputs_types_and_bounded_sample(tmp_path):
    """--dump-outputs writes ids as float64 (exact) and distances as float32; an answer above 64 MB in all is cut to the same seeded
    sample of query rows in both files, the same rows on every call"""
    import torch
    ids = torch.arange(40 * 7, dtype=torch.int64).reshape(40, 7) - 1
    dists = torch.rand((40, 7), generator=torch.Generator().manual_seed(1))
    B.dump_outputs(str(tmp_path / "small"), ids, dists)
    gi, gd = np.load(tmp_path / "small" / "ids.npy"), np.load(tmp_path / "small" / "distances.npy")
    assert gi.dtype == np.float64 and np.array_equal(gi, ids.numpy()) and gd.dtype == np.float32 and np.array_equal(gd, dists.numpy())
    n, k = 6_000_000, 10  # 12 bytes per entry: 720 MB
    ids = torch.arange(n, dtype=torch.int64)[:, None].expand(n, k).contiguous()
    dists = ids.float()
    for sub in ("a", "b"):
        B.dump_outputs(str(tmp_path / sub), ids, dists)
    ga, gb = np.load(tmp_path / "a" / "ids.npy"), np.load(tmp_path / "b" / "ids.npy")
    da = np.load(tmp_path / "a" / "distances.npy")
    assert ga.nbytes + da.nbytes <= B.DUMP_LIMIT_BYTES and ga.shape[0] > n // 20 and ga.shape[1] == k
    assert np.array_equal(ga, gb) and np.array_equal(da, ga.astype(np.float32))  # the same rows, in both files
    assert (np.diff(ga[:, 0]) > 0).all()  # in query order


def test_bench_refuses_zero_steps():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "0"], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_its_answer(tmp_path):
    """a plain run (no --full): exactly --steps timed steps, the headline fields and nothing measured beside them; --dump-outputs
    writes the answer of the last timed step, and a second run of the same command writes the same bits"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--settle", "3",
                            "--nvec", "200000", "--nlist", "256", "--batch", "512", "--dump-outputs", str(tmp_path / run)],
                           cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    line = lines[0]
    assert line["steps"] == 7 and line["timed_steps_total"] == 7 and line["timed_groups"]["groups"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 512) < 1e-2 * 512
    assert line["unit"] == "queries/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["config"]["recall_at_k"] >= 0.9 and line["config"]["nprobe"] == lines[1]["config"]["nprobe"]
    assert not {"roofline", "phases_ms", "cpu_baseline", "workloads", "host_api", "batches_in_flight"} & set(line)
    ia, da = np.load(tmp_path / "a" / "ids.npy"), np.load(tmp_path / "a" / "distances.npy")
    ib, db = np.load(tmp_path / "b" / "ids.npy"), np.load(tmp_path / "b" / "distances.npy")
    assert ia.dtype == np.float64 and da.dtype == np.float32 and ia.shape == da.shape == (512, 10)
    full_rows = (ia >= 0).all(1)  # (a query whose probed lists hold fewer than k rows gets -1 entries)
    assert full_rows.mean() > 0.9 and ((ia >= -1) & (ia < 200000)).all() and (np.diff(da[full_rows], axis=1) >= 0).all()
    assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
