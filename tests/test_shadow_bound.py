"""The error bound of the fp16 shadow form (qk_shadow_error_bound, quake_amd/csrc/qk_shadow_bound.h), without a GPU.

The form selects candidates by approximate keys -- the exact stored norms and a dot product of the fp16 images of query and row --
and proves its answer from |approximate key - canonical fp32 key| <= E.  Here both sides are emulated: the fp16 rounding (numpy's
round-to-nearest-even), once with subnormal images kept and once flushed to zero, the dot product of the images in float64 and as
fp32 accumulations in two orders, and the canonical fp32 chain (one fused step per column, natural order).  The bound's inputs are
what the kernels compute: ||q||, the distance of q and of the rows to their images (a subnormal image counts as the farther of
itself and zero), the largest image norm -- each rounded up.  The assertion is the inequality, for every (query, row) pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_MIN_NORMAL = 2.0 ** -14


def _bound(metric, d, qn, rho_q, rho, xmax):
    from quake_amd import _lib
    lib = _lib.load()
    code = {"ip": _lib.QK_METRIC_IP, "l2": _lib.QK_METRIC_L2}[metric]
    return float(lib.qk_shadow_error_bound(code, int(d), C.c_float(qn), C.c_float(rho_q), C.c_float(rho), C.c_float(xmax)))


def _up32(v):
    """a float32 >= v (v: float64 >= 0)"""
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def _images(a):
    """fp16 images of a float32 array, as float64: (kept, flushed)"""
    h = a.astype(np.float16).astype(np.float64)
    f = np.where(np.abs(h) < H_MIN_NORMAL, 0.0, h)
    return h, f


def _dist_to_image(a):
    """per row: the distance to the fp16 image with a subnormal element counted as the farther of itself and zero"""
    a64 = a.astype(np.float64)
    h, _ = _images(a)
    e = np.abs(a64 - h)
    sub = (h != 0) & (np.abs(h) < H_MIN_NORMAL)
    e = np.where(sub, np.maximum(e, np.abs(a64)), e)
    return np.sqrt((e * e).sum(-1))


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _chain(q, x):
    """canonical dot products [nq, n]: acc = fma(x[k], q[k], acc), k = 0 .. d-1"""
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    for k in range(q.shape[1]):
        acc = _fma32(np.broadcast_to(x[None, :, k], acc.shape), np.broadcast_to(q[:, None, k], acc.shape), acc)
    return acc


def _norms(a):
    acc = np.zeros(a.shape[0], np.float32)
    for k in range(a.shape[1]):
        acc = _fma32(a[:, k], a[:, k], acc)
    return acc


def _l2_key(xn, yn, ip):
    s = (xn[:, None] + yn[None, :]).astype(np.float32)
    r = _fma32(np.full_like(ip, -2.0), ip, s)
    return np.maximum(r, np.float32(0.0))


def _approx_dots(q, x):
    """the dot product of the images as the matrix unit may deliver it: float64 (then fp32), fp32 accumulation forwards and
    backwards, each with subnormal images kept and flushed"""
    out = []
    for qi, xi in zip(_images(q), _images(x)):
        out.append((qi @ xi.T).astype(np.float32))
        for order in (range(q.shape[1]), reversed(range(q.shape[1]))):
            acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
            for k in order:
                acc = (acc.astype(np.float64) + qi[:, None, k] * xi[None, :, k]).astype(np.float32)
            out.append(acc)
    return out


def _check(q, x, metric):
    q, x = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(x, np.float32)
    d = q.shape[1]
    canon = _chain(q, x)
    xn, yn = _norms(q), _norms(x)
    rho = _up32(_dist_to_image(x).max())
    xmax = _up32(np.sqrt((_images(x)[0] ** 2).sum(-1)).max())
    qn = [_up32(np.sqrt(float(v))) for v in (q.astype(np.float64) ** 2).sum(-1)]
    rho_q = [_up32(v) for v in _dist_to_image(q)]
    E = np.array([_bound(metric, d, qn[i], rho_q[i], rho, xmax) for i in range(q.shape[0])])
    assert np.all(E >= 0), "finite inputs inside the fp16 range must have a bound"
    ck = _l2_key(xn, yn, canon) if metric == "l2" else canon
    worst = 0.0
    for a in _approx_dots(q, x):
        ak = _l2_key(xn, yn, a) if metric == "l2" else a
        err = np.abs(ak.astype(np.float64) - ck.astype(np.float64))
        worst = max(worst, float((err / np.maximum(E[:, None], 1e-300)).max()))
        assert np.all(err <= E[:, None]), (metric, d, float(err.max()), float(E.min()))
    return worst


def _cases(d, rng):
    g = lambda n, s=1.0: (s * rng.standard_normal((n, d))).astype(np.float32)
    yield "gaussian", g(6), g(40)
    yield "clustered", g(6) + 3.0, g(40) + 3.0
    yield "tiny", g(4, 1e-6), g(30, 1e-6)
    yield "subnormal images", g(4, 3e-5), g(30, 3e-5)
    yield "below the smallest image", g(4, 1e-9), g(30, 1e-9)
    yield "underflowing products", g(4, 1e-20), g(30, 1e-20)
    yield "huge", g(4, 2e4).clip(-65504, 65504), g(30, 2e4).clip(-65504, 65504)
    yield "near the top of the range", np.full((3, d), 6e4, np.float32) + g(3, 100.0), np.full((20, d), -6e4, np.float32) + g(20, 100.0)
    mixed = g(30) * (10.0 ** rng.integers(-7, 4, size=(30, d))).astype(np.float32)
    yield "mixed magnitudes", g(4) * (10.0 ** rng.integers(-7, 4, size=(4, d))).astype(np.float32), mixed
    z = g(30)
    z[::3] = 0
    yield "zero rows", np.concatenate([g(3), np.zeros((1, d), np.float32)]), z
    yield "integers", rng.integers(-40, 41, size=(4, d)).astype(np.float32), rng.integers(-40, 41, size=(30, d)).astype(np.float32)
    # adversarial: every element half an fp16 ulp above an image (the largest rounding error), all errors of one sign, the query
    # aligned with the error vector
    h = np.abs(g(30)).astype(np.float16)
    ulp = (np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64))
    xa = (h.astype(np.float64) + 0.4999 * ulp).astype(np.float32)
    yield "half-ulp errors, aligned query", np.abs(g(4)) + 1.0, xa


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_bound_holds_for_every_pair(metric):
    rng = np.random.default_rng(5)
    dims = sorted(set(list(range(1, 20)) + [31, 32, 33, 47, 48, 63, 64, 65, 96, 127, 128, 129, 200, 255, 256]))
    worst = {}
    for d in dims:
        for name, q, x in _cases(d, rng):
            worst[name] = max(worst.get(name, 0.0), _check(q, x, metric))
    print({k: round(v, 4) for k, v in worst.items()})  # the largest error / bound per case: how much of the bound is used


def test_every_dimension_up_to_256():
    rng = np.random.default_rng(6)
    for d in range(1, 257):
        q = rng.standard_normal((2, d)).astype(np.float32)
        x = (rng.standard_normal((12, d)) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
        _check(q, x, "l2")


def test_no_bound_outside_the_range():
    for bad in (float("inf"), float("nan"), -1.0):
        assert _bound("l2", 128, bad, 0.0, 0.0, 1.0) == -1.0
        assert _bound("ip", 128, 1.0, 0.0, bad, 1.0) == -1.0
    assert _bound("l2", 0, 1.0, 0.0, 0.0, 1.0) == -1.0
    assert 0 < _bound("l2", 128, 15.0, 3e-3, 3e-3, 15.0) < 0.5  # the bench's scale: keys near 15 ** 2, the bound a fraction of one


def test_native_edge_values_under_sanitizers(tmp_path):
    """tests/native/shadow_bound_check.cpp: the same function on zeros, subnormals, FLT_MAX, infinities and NaN, compiled with the
    address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "shadow_bound_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "quake_amd", "csrc"), os.path.join(ROOT, "tests", "native", "shadow_bound_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
