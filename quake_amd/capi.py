"""Thin object wrappers over the C ABI (include/quake_hip.h) for Python callers and the test-suite.

Host data is passed as numpy arrays (QK_MEM_HOST); device data as torch CUDA tensors (QK_MEM_DEVICE).
Every call goes through libquake_hip.so -- there is no alternative code path.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import QK_MEM_DEVICE, QK_MEM_HOST, QK_METRIC_IP, QK_METRIC_L2, QkTiming, check


def metric_code(metric):
    """str_to_metric_type (src/cpp/include/common.h:145-156)."""
    if isinstance(metric, str):
        m = metric.lower()
        if m == "l2":
            return QK_METRIC_L2
        if m == "ip":
            return QK_METRIC_IP
        raise ValueError("Invalid metric type: " + metric)
    return int(metric)


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _mem_of(*arrs):
    kinds = set()
    for a in arrs:
        if a is None:
            continue
        if _is_torch(a):
            kinds.add(QK_MEM_DEVICE if a.is_cuda else QK_MEM_HOST)
        else:
            kinds.add(QK_MEM_HOST)
    if len(kinds) > 1:
        raise ValueError("mixed host/device arguments")
    return kinds.pop() if kinds else QK_MEM_HOST


def _f32(a):
    if _is_torch(a):
        import torch
        return a.contiguous().to(torch.float32)
    return np.ascontiguousarray(a, dtype=np.float32)


def _i64(a):
    if _is_torch(a):
        import torch
        return a.contiguous().to(torch.int64)
    return np.ascontiguousarray(a, dtype=np.int64)


def _pids_rows(pids, Q):
    """pids as [Q, P]: a one-dimensional list is the same set for every query (query_coordinator.cpp:506-508)"""
    if pids.ndim != 1:
        return pids
    if _is_torch(pids):
        return pids[None, :].expand(Q, -1).contiguous()
    return np.ascontiguousarray(np.broadcast_to(pids[None, :], (Q, pids.shape[0])))


def _i32_with(a, ref):
    """`a` as a contiguous int32 vector in the memory space of `ref` (numpy on the host, torch on ref's device)"""
    if _is_torch(ref) and ref.is_cuda:
        import torch
        a = a if _is_torch(a) else torch.as_tensor(np.ascontiguousarray(a))
        return a.reshape(-1).to(device=ref.device, dtype=torch.int32).contiguous()
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _filter_batch(filter, filters, query_filter, x):
    """the (handle array, F, qfilter) of a per-query call, or None: filters= / query_filter= come together and exclude filter="""
    if filters is None and query_filter is None:
        return None
    if filter is not None:
        raise ValueError("filter= and filters= / query_filter= are exclusive")
    if filters is None or query_filter is None:
        raise ValueError("filters= and query_filter= must be given together")
    filters = list(filters)
    qf = _i32_with(query_filter, x)
    if qf.shape[0] != x.shape[0]:
        raise ValueError("query_filter must have one entry per query: %d != %d" % (qf.shape[0], x.shape[0]))
    harr = (C.c_void_p * max(len(filters), 1))(*[f.h if f is not None else None for f in filters])
    return harr, len(filters), qf


def _empty_like_mem(shape, dtype, ref):
    if _is_torch(ref) and ref.is_cuda:
        import torch
        tdt = torch.int64 if dtype == np.int64 else torch.int32 if dtype == np.int32 else torch.float32
        return torch.empty(shape, dtype=tdt, device=ref.device)
    return np.empty(shape, dtype)


QK_ORDER_DESC = 1          # include/quake_hip.h: the flags of ordered search
QK_ORDER_MISSING_LAST = 2
QK_MAX_ORDER_K = 1024
QK_MAX_FETCH_K = 256       # diversified search
QK_MAXSIM_MAX_TOKENS = 64  # multi-vector search
QK_MAXSIM_MAX_K = 1024


def timing_dict(t):
    return {f: getattr(t, f) for f, _ in QkTiming._fields_}


class Context:
    def __init__(self, device=0):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        check(self.lib.qk_ctx_create(int(device), C.byref(self.h)))
        self.device = int(device)

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.lib.qk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.qk_ctx_synchronize(self.h))

    def set_form_feedback(self, enabled):
        """measured choice between the scan forms per batch shape (default on); off = the static rule alone"""
        check(self.lib.qk_ctx_set_form_feedback(self.h, int(bool(enabled))))

    def set_form_times(self, ms3):
        """the feedback rule on injected figures: ms3 = (tile form, per-wave walk, mixed) in ms, or None for measured times"""
        if ms3 is None:
            check(self.lib.qk_ctx_set_form_times(self.h, None))
        else:
            check(self.lib.qk_ctx_set_form_times(self.h, (C.c_float * 3)(*[float(v) for v in ms3])))

    def set_shadow(self, mode):
        """the fp16 shadow form of the single-probe search (qk_ctx_set_shadow): 0 never, 1 automatic, 2 forced"""
        check(self.lib.qk_ctx_set_shadow(self.h, int(mode)))

    def shadow_stats(self):
        """{verified, fallback, candidates}: queries the shadow form's finish verified / answered by the exact scan of their
        list, and candidates it re-scored in fp32, since the context was created (qk_ctx_shadow_stats)"""
        v, f, c, ch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.qk_ctx_shadow_stats(self.h, C.byref(v), C.byref(f), C.byref(c), C.byref(ch)))
        return {"verified": v.value, "fallback": f.value, "candidates": c.value, "chained": ch.value}

    def set_shadow_form_time(self, ms):
        """the fourth injected figure of set_form_times (the shadow form's); None or 0 clears it"""
        check(self.lib.qk_ctx_set_shadow_form_time(self.h, C.c_float(float(ms or 0.0))))

    def set_stream(self, hip_stream):
        """hip_stream: a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream); 0 = the device's NULL stream
        (torch's default stream); None = back to the context's private stream.
        Calls on DEVICE buffers (torch CUDA tensors in, torch CUDA tensors out) are ordered on the context's stream only: the private
        stream is non-blocking, so a caller that mixes them with torch operations binds the context to torch's current stream first
        (GpuEngine and the bindings do) -- otherwise torch may read an output before the library's kernel wrote it."""
        if hip_stream is None:
            check(self.lib.qk_ctx_set_stream(self.h, None))
        elif int(hip_stream) == 0:
            check(self.lib.qk_ctx_set_null_stream(self.h))
        else:
            check(self.lib.qk_ctx_set_stream(self.h, C.c_void_p(int(hip_stream))))

    def set_timing(self, mode=1):
        """0 off, 1 per-call (synchronising), 2 deferred (read with read_timing()), 3 deferred with one event pair around
        the scan kernel only (what bench.py keeps on inside its timed region)."""
        check(self.lib.qk_ctx_set_timing(self.h, int(mode)))

    def get_timing(self):
        """the timing mode set last (qk_ctx_get_timing)"""
        m = C.c_int(0)
        check(self.lib.qk_ctx_get_timing(self.h, C.byref(m)))
        return int(m.value)

    def read_timing(self):
        t, n = QkTiming(), C.c_int64()
        check(self.lib.qk_ctx_read_timing(self.h, C.byref(t), C.byref(n)))
        out = timing_dict(t)
        out["calls"] = n.value
        return out

    def set_squared_l2(self, on=True):
        check(self.lib.qk_ctx_set_squared_l2(self.h, int(bool(on))))

    def last_scan_kernel(self):
        """name of the partition-scan kernel the last scan / search on this context launched"""
        buf = C.create_string_buffer(64)
        check(self.lib.qk_ctx_last_scan_kernel(self.h, buf, 64))
        return buf.value.decode()

    def device_info(self):
        cus, clk, hbm = C.c_int(), C.c_int(), C.c_int64()
        arch = C.create_string_buffer(64)
        check(self.lib.qk_ctx_device_info(self.h, C.byref(cus), C.byref(clk), C.byref(hbm), arch, 64))
        return dict(num_cus=cus.value, clock_khz=clk.value, hbm_bytes=hbm.value, arch=arch.value.decode())

    # ---- search ---------------------------------------------------------------------------------------
    def coarse(self, parent, x, nprobe, metric, values=True):
        """the nprobe nearest lists of every row (and, with values, their distances; values=False passes out_dist = NULL)"""
        x = _f32(x)
        Q = x.shape[0]
        kk = int(min(nprobe, parent.ntotal()))
        mem = _mem_of(x)
        out_p = _empty_like_mem((Q, kk), np.int64, x)
        out_d = _empty_like_mem((Q, kk), np.float32, x) if values else None
        check(self.lib.qk_coarse(self.h, parent.h, _ptr(x), Q, int(nprobe), metric_code(metric), _ptr(out_p),
                                 _ptr(out_d) if values else None, mem))
        return out_p, out_d

    def scan(self, store, x, pids, k, metric, timing=False, filter=None, filters=None, query_filter=None):
        """filter: a Filter of `store` -- only its candidates are returned (qk_scan_filtered).
        filters + query_filter: one filter per query -- query i sees the candidates of filters[query_filter[i]]; query_filter is
        an int32 array / tensor of shape [Q], on the host or on the device with x (qk_scan_filtered_batch)"""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        t = QkTiming()
        fb = _filter_batch(filter, filters, query_filter, x)
        if fb is not None:
            check(self.lib.qk_scan_filtered_batch(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None,
                                                  int(pids.shape[1]), int(k), metric_code(metric), fb[0], fb[1], _ptr(fb[2]),
                                                  _ptr(out_i), _ptr(out_d), mem, C.byref(t) if timing else None))
            return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)
        if filter is not None:
            check(self.lib.qk_scan_filtered(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None,
                                            int(pids.shape[1]), int(k), metric_code(metric), filter.h, _ptr(out_i), _ptr(out_d),
                                            mem, C.byref(t) if timing else None))
            return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)
        check(self.lib.qk_scan(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]),
                               int(k), metric_code(metric), _ptr(out_i), _ptr(out_d), mem, C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)

    def scan_into(self, store, x, pids, k, metric, out):
        """scan() writing into caller-provided (ids, dist) tensors (no allocation in the timed loop)."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        out_i, out_d = out
        check(self.lib.qk_scan(self.h, store.h, _ptr(x), Q, _ptr(pids), int(pids.shape[1]), int(k), metric_code(metric),
                               _ptr(out_i), _ptr(out_d), _mem_of(x, pids), None))
        return out_i, out_d

    def search(self, parent, store, x, nprobe, k, metric, timing=False, out=None, filter=None, filters=None, query_filter=None):
        """filter: a Filter of `store` -- the k best of its candidates in the probed lists (qk_search_filtered).
        filters + query_filter: one filter per query, as in scan() (qk_search_filtered_batch)"""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        if out is None:
            out_i = _empty_like_mem((Q, k), np.int64, x)
            out_d = _empty_like_mem((Q, k), np.float32, x)
        else:
            out_i, out_d = out
        t = QkTiming()
        fb = _filter_batch(filter, filters, query_filter, x)
        if fb is not None:
            check(self.lib.qk_search_filtered_batch(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q,
                                                    int(nprobe), int(k), metric_code(metric), fb[0], fb[1], _ptr(fb[2]),
                                                    _ptr(out_i), _ptr(out_d), mem, C.byref(t) if timing else None))
            return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)
        if filter is not None:
            check(self.lib.qk_search_filtered(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe),
                                              int(k), metric_code(metric), filter.h, _ptr(out_i), _ptr(out_d), mem,
                                              C.byref(t) if timing else None))
            return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)
        check(self.lib.qk_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe), int(k),
                                 metric_code(metric), _ptr(out_i), _ptr(out_d), mem, C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)

    def search_exact(self, store, x, k, metric, filter, max_rows=0, timing=False, out=None):
        """qk_search_filtered_exact: the k best candidates of `filter` over the WHOLE store -- no parent, no nprobe; the flat
        search of the filter's candidate rows, k up to 8192.  max_rows > 0: a filter with more candidates is refused."""
        x = _f32(x)
        Q = x.shape[0]
        if out is None:
            out_i = _empty_like_mem((Q, k), np.int64, x)
            out_d = _empty_like_mem((Q, k), np.float32, x)
        else:
            out_i, out_d = out
        t = QkTiming()
        check(self.lib.qk_search_filtered_exact(self.h, store.h, _ptr(x), Q, int(k), metric_code(metric),
                                                filter.h if filter is not None else None, int(max_rows), _ptr(out_i), _ptr(out_d),
                                                _mem_of(x), C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)

    def search_exact_batch(self, store, x, k, metric, filters, query_filter, max_rows=0, pool_rows=0, timing=False, out=None):
        """qk_search_filtered_exact_batch: query i gets the k best candidates of filters[query_filter[i]] over the WHOLE store,
        exactly, in one enqueue -- every filter's candidates are a list of the store's candidate pool (Store.exact_pool_info).
        query_filter: int32 [Q], on the host or on the device with x.  max_rows > 0: a filter with more candidates is refused;
        pool_rows > 0: the rows the pool may hold after the call."""
        x = _f32(x)
        Q = x.shape[0]
        if out is None:
            out_i = _empty_like_mem((Q, k), np.int64, x)
            out_d = _empty_like_mem((Q, k), np.float32, x)
        else:
            out_i, out_d = out
        t = QkTiming()
        harr, F, qf = _filter_batch(None, filters, query_filter, x)
        check(self.lib.qk_search_filtered_exact_batch(self.h, store.h, _ptr(x), Q, int(k), metric_code(metric), harr, F, _ptr(qf),
                                                      int(max_rows), int(pool_rows), _ptr(out_i), _ptr(out_d), _mem_of(x),
                                                      C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)

    def search_tracked(self, parent, store, x, nprobe, k, metric, timing=False, filter=None, filters=None, query_filter=None):
        """qk_search_tracked: search + the [Q, min(nprobe, parent lists)] list numbers every query scanned, one enqueue.
        Returns (ids, dist, probed[, timing]).  filter: a Filter of `store` (qk_search_filtered_tracked; the probed lists are
        those of the unfiltered search).  filters + query_filter: one filter per query (qk_search_filtered_batch_tracked)."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        width = max(min(int(nprobe), int(parent.ntotal())), 0)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        out_p = _empty_like_mem((Q, max(width, 1)), np.int64, x)
        t = QkTiming()
        fb = _filter_batch(filter, filters, query_filter, x)
        if fb is not None:
            check(self.lib.qk_search_filtered_batch_tracked(self.h, parent.h, store.h, _ptr(x), Q, int(nprobe), int(k),
                                                            metric_code(metric), fb[0], fb[1], _ptr(fb[2]), _ptr(out_i),
                                                            _ptr(out_d), _ptr(out_p), mem, C.byref(t) if timing else None))
        elif filter is not None:
            check(self.lib.qk_search_filtered_tracked(self.h, parent.h, store.h, _ptr(x), Q, int(nprobe), int(k),
                                                      metric_code(metric), filter.h, _ptr(out_i), _ptr(out_d), _ptr(out_p), mem,
                                                      C.byref(t) if timing else None))
        else:
            check(self.lib.qk_search_tracked(self.h, parent.h, store.h, _ptr(x), Q, int(nprobe), int(k), metric_code(metric),
                                             _ptr(out_i), _ptr(out_d), _ptr(out_p), mem, C.byref(t) if timing else None))
        out_p = out_p[:, :width]
        return (out_i, out_d, out_p, timing_dict(t)) if timing else (out_i, out_d, out_p)

    def search_adaptive(self, parent, store, x, nprobe, max_nprobe, k, metric, min_candidates=None, filter=None, filters=None,
                        query_filter=None, probed=True, nprobed=True):
        """qk_search_filtered_adaptive: every query probes the shortest prefix of its max_nprobe ranked lists, at least nprobe of
        them, that holds min_candidates (default k) candidates of its filter.  filter, or filters + query_filter as in search().
        Returns (ids, dist, nprobed, probed, timing): nprobed int32 [Q] (None with nprobed=False), probed int64
        [Q, min(max_nprobe, parent lists)] -- the prefix, then -1 -- or None with probed=False."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        fb = _filter_batch(filter, filters, query_filter, x)
        if fb is None:
            harr, F, qf = (C.c_void_p * 1)(filter.h if filter is not None else None), 1, None
        else:
            harr, F, qf = fb
        width = max(min(int(max_nprobe), int(parent.ntotal())), 0) if parent is not None else 0
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        out_n = _empty_like_mem((Q,), np.int32, x) if nprobed else None
        out_p = _empty_like_mem((Q, max(width, 1)), np.int64, x) if probed else None
        t = QkTiming()
        check(self.lib.qk_search_filtered_adaptive(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe),
                                                   int(max_nprobe), int(k if min_candidates is None else min_candidates), int(k),
                                                   metric_code(metric), harr, F, _ptr(qf), _ptr(out_i), _ptr(out_d), _ptr(out_n),
                                                   _ptr(out_p), mem, C.byref(t)))
        if probed:
            out_p = out_p[:, :width]
        return out_i, out_d, out_n, out_p, timing_dict(t)

    # ---- paged search ---------------------------------------------------------------------------------
    def _after(self, after, x):
        """the (keys, ids) of a cursor in x's memory space -- keys int32 holding the uint32 bit pattern, ids int64, one entry per
        query; either may be None (the C ABI then says what it thinks of one without the other)"""
        if after is None:
            return None, None
        keys, ids = after
        Q = x.shape[0]
        if keys is not None:
            if not _is_torch(keys):
                keys = np.ascontiguousarray(keys)
                if keys.dtype == np.uint32:
                    keys = keys.view(np.int32)
            keys = _i32_with(keys, x)
        if ids is not None:
            if _is_torch(x) and x.is_cuda:
                import torch
                ids = ids if _is_torch(ids) else torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64))
                ids = ids.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
            else:
                ids = _i64(ids.detach().cpu().numpy() if _is_torch(ids) else ids).reshape(-1)
        for a in (keys, ids):
            if a is not None and a.shape[0] != Q:
                raise ValueError("a cursor has one entry per query: %d != %d" % (a.shape[0], Q))
        return keys, ids

    def search_after(self, parent, store, x, nprobe, k, metric, after=None, filter=None, timing=False):
        """qk_search_after: the page of k results behind every query's cursor, in (key, id) order over the lists search() probes.
        after: (keys, ids) as a call returned them, or None = from the start (the page is then search()'s, bit for bit).
        filter: a Filter of `store`.  Returns (ids, dist, (next_keys, next_ids)[, timing]); keys are int32 arrays / tensors that
        hold the uint32 bit pattern, a row with fewer than k results leaves the exhausted cursor (0xFFFFFFFF, INT64_MAX)."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        ak, ai = self._after(after, x)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        nk, ni = _empty_like_mem((Q,), np.int32, x), _empty_like_mem((Q,), np.int64, x)
        t = QkTiming()
        check(self.lib.qk_search_after(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe), int(k),
                                       metric_code(metric), _ptr(ak), _ptr(ai), filter.h if filter is not None else None, _ptr(out_i),
                                       _ptr(out_d), _ptr(nk), _ptr(ni), mem, C.byref(t) if timing else None))
        return (out_i, out_d, (nk, ni), timing_dict(t)) if timing else (out_i, out_d, (nk, ni))

    def scan_after(self, store, x, pids, k, metric, after=None, filter=None, timing=False):
        """qk_scan_after: search_after over the given lists (pids as in scan())"""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        ak, ai = self._after(after, x)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        nk, ni = _empty_like_mem((Q,), np.int32, x), _empty_like_mem((Q,), np.int64, x)
        t = QkTiming()
        check(self.lib.qk_scan_after(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]), int(k),
                                     metric_code(metric), _ptr(ak), _ptr(ai), filter.h if filter is not None else None, _ptr(out_i),
                                     _ptr(out_d), _ptr(nk), _ptr(ni), mem, C.byref(t) if timing else None))
        return (out_i, out_d, (nk, ni), timing_dict(t)) if timing else (out_i, out_d, (nk, ni))

    # ---- range search ---------------------------------------------------------------------------------
    def _range(self, call, x, cap, timing, out):
        """the capacity protocol of qk_range_search / qk_range_scan around `call(cap, lims, ids, dist, timing)`: with cap=None a
        guess, then one more call only if lims[Q] says it was short; ids / dist come back trimmed to what was written"""
        Q = x.shape[0]
        lims = _empty_like_mem((Q + 1,), np.int64, x)
        t = QkTiming()
        self.last_range_calls = 0

        def run(c, ids, dist):
            self.last_range_calls += 1
            call(int(c), lims, ids, dist, C.byref(t) if timing else None)
            if _is_torch(lims) and lims.is_cuda:
                self.synchronize()
            return int(lims[Q])

        if out is not None:
            ids, dist = out
            if cap is None:
                cap = 0 if ids is None else int(ids.shape[0])
            total = run(cap, ids, dist)
        elif cap is not None:
            ids = _empty_like_mem((int(cap),), np.int64, x) if cap > 0 else None
            dist = _empty_like_mem((int(cap),), np.float32, x) if cap > 0 else None
            total = run(cap, ids, dist)
        else:
            cap = max(4096, 64 * Q)
            ids, dist = _empty_like_mem((cap,), np.int64, x), _empty_like_mem((cap,), np.float32, x)
            total = run(cap, ids, dist)
            if total > cap:
                cap = total
                ids, dist = _empty_like_mem((cap,), np.int64, x), _empty_like_mem((cap,), np.float32, x)
                total = run(cap, ids, dist)
        n = min(int(cap), total)
        ids = ids[:n] if ids is not None else _empty_like_mem((0,), np.int64, x)
        dist = dist[:n] if dist is not None else _empty_like_mem((0,), np.float32, x)
        return (lims, ids, dist, timing_dict(t)) if timing else (lims, ids, dist)

    def range_search(self, parent, store, x, nprobe, radius, metric, filter=None, cap=None, timing=False, out=None):
        """qk_range_search: every row of the lists qk_search probes whose distance passes `radius` (L2: <=, IP: >=), in scan
        order.  Returns (lims [Q + 1], ids, dist[, timing]): query q's hits are [lims[q], lims[q+1]).  cap=None: the wrapper
        sizes the buffers (a second call only when the first guess was short) and returns everything; a given cap (or
        out=(ids, dist) buffers of the caller, untouched behind the written prefix) returns the first min(cap, lims[Q]) hits
        while lims stays exact; cap=0 counts only.  filter: a Filter of `store`."""
        x = _f32(x)
        mem = _mem_of(x)

        def call(c, lims, ids, dist, t):
            check(self.lib.qk_range_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), x.shape[0], int(nprobe),
                                           metric_code(metric), float(radius), filter.h if filter is not None else None, c,
                                           _ptr(lims), _ptr(ids), _ptr(dist), mem, t))
        return self._range(call, x, cap, timing, out)

    def range_scan(self, store, x, pids, radius, metric, filter=None, cap=None, timing=False, out=None):
        """qk_range_scan: range_search over the given lists -- pids [Q, P] (or [P] for every query), -1 / absent / empty lists
        contribute nothing; a query's hits follow the order of its pids row."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)

        def call(c, lims, ids, dist, t):
            check(self.lib.qk_range_scan(self.h, store.h, _ptr(x), Q, _ptr(pids), int(pids.shape[1]), metric_code(metric), float(radius),
                                         filter.h if filter is not None else None, c, _ptr(lims), _ptr(ids), _ptr(dist), mem, t))
        return self._range(call, x, cap, timing, out)

    # ---- grouped search ---------------------------------------------------------------------------------
    @staticmethod
    def _grouped_out(x, Q, k, group_size, out):
        # group_size None: the one-row shapes [Q, k]; an int m: ids / dist [Q, k, m], groups [Q, k]
        if out is not None:
            return out
        shp = (Q, k) if group_size is None else (Q, k, int(group_size))
        return (_empty_like_mem(shp, np.int64, x), _empty_like_mem(shp, np.float32, x), _empty_like_mem((Q, k), np.int64, x))

    def search_grouped(self, parent, store, x, nprobe, k, metric, group_by, filter=None, timing=False, out=None, group_size=None):
        """qk_search_grouped: the k best groups of the Attr `group_by` per query over the lists qk_search probes, every group
        represented by its best row.  Returns (ids [Q, k], dist [Q, k], groups [Q, k][, timing]); out=(ids, dist, groups):
        buffers of the caller.  filter: a Filter of `store` (a group is then represented by its best allowed row).
        group_size=m (an int, 1 <= m <= 16): qk_search_grouped_n, the m best rows of every group -- ids / dist [Q, k, m],
        groups [Q, k]; `out` follows."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        out_i, out_d, out_g = self._grouped_out(x, Q, k, group_size, out)
        t = QkTiming()
        head = (self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe), int(k))
        tail = (metric_code(metric), group_by.h if group_by is not None else None, filter.h if filter is not None else None,
                _ptr(out_i), _ptr(out_d), _ptr(out_g), mem, C.byref(t) if timing else None)
        if group_size is None:
            check(self.lib.qk_search_grouped(*head, *tail))
        else:
            check(self.lib.qk_search_grouped_n(*head, int(group_size), *tail))
        return (out_i, out_d, out_g, timing_dict(t)) if timing else (out_i, out_d, out_g)

    def scan_grouped(self, store, x, pids, k, metric, group_by, filter=None, timing=False, out=None, group_size=None):
        """qk_scan_grouped: search_grouped over the given lists -- pids [Q, P] (or [P] for every query); -1 / absent / empty lists
        contribute nothing.  group_size as for search_grouped (qk_scan_grouped_n)."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        out_i, out_d, out_g = self._grouped_out(x, Q, k, group_size, out)
        t = QkTiming()
        head = (self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]), int(k))
        tail = (metric_code(metric), group_by.h if group_by is not None else None, filter.h if filter is not None else None,
                _ptr(out_i), _ptr(out_d), _ptr(out_g), mem, C.byref(t) if timing else None)
        if group_size is None:
            check(self.lib.qk_scan_grouped(*head, *tail))
        else:
            check(self.lib.qk_scan_grouped_n(*head, int(group_size), *tail))
        return (out_i, out_d, out_g, timing_dict(t)) if timing else (out_i, out_d, out_g)

    # ---- facet counts -----------------------------------------------------------------------------------
    @staticmethod
    def _facet_args(x, Q, facet_by, n_values, out):
        cols = list(facet_by) if isinstance(facet_by, (list, tuple)) else [facet_by]
        C_, n = len(cols), int(n_values)
        harr = (C.c_void_p * max(C_, 1))(*[a.h if a is not None else None for a in cols])
        if out is None:
            # (the library refuses a count outside its limits before it writes: the buffers only have to exist)
            shp = (max(C_, 0), Q, max(n, 0))
            out = (_empty_like_mem(shp, np.int64, x), _empty_like_mem(shp, np.int64, x), _empty_like_mem(shp[:2], np.int64, x),
                   _empty_like_mem(shp[:2], np.int64, x), _empty_like_mem((Q,), np.int64, x))
        return harr, C_, n, out

    def facet_search(self, parent, store, x, nprobe, radius, metric, facet_by, n_values=10, filter=None, timing=False, out=None):
        """qk_facet_search: per query, the value counts of the Attr columns `facet_by` (one Attr or a list of up to 4) over the
        hits of range_search with the same arguments.  Returns (values [C, Q, n], counts [C, Q, n], distinct [C, Q],
        missing [C, Q], total [Q][, timing]): per column the n_values most frequent values, count descending then value
        ascending, padded with value 0 / count 0; out=(values, counts, distinct, missing, total): buffers of the caller."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        harr, C_, n, out = self._facet_args(x, Q, facet_by, n_values, out)
        t = QkTiming()
        check(self.lib.qk_facet_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe),
                                       metric_code(metric), float(radius), filter.h if filter is not None else None, harr, C_, n,
                                       *[_ptr(o) for o in out], mem, C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    def facet_scan(self, store, x, pids, radius, metric, facet_by, n_values=10, filter=None, timing=False, out=None):
        """qk_facet_scan: facet_search over the given lists -- pids [Q, P] (or [P] for every query); -1 / absent / empty lists
        contribute nothing."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        harr, C_, n, out = self._facet_args(x, Q, facet_by, n_values, out)
        t = QkTiming()
        check(self.lib.qk_facet_scan(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]),
                                     metric_code(metric), float(radius), filter.h if filter is not None else None, harr, C_, n,
                                     *[_ptr(o) for o in out], mem, C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    # ---- facet statistics -------------------------------------------------------------------------------
    @staticmethod
    def _facet_stats_args(x, Q, attrs, edges):
        from .where import lower_edges
        cols = list(attrs) if isinstance(attrs, (list, tuple)) else [attrs]
        C_ = len(cols)
        harr = (C.c_void_p * max(C_, 1))(*[a.h if a is not None else None for a in cols])
        flat, n_edges = lower_edges(["column %d" % c for c in range(C_)], edges, "[facet_stats]")
        earr = (C.c_int64 * max(len(flat), 1))(*flat) if edges is not None else None
        narr = (C.c_int * max(C_, 1))(*n_edges) if edges is not None else None
        hs = 1 + max(n_edges, default=0)
        # (the library refuses a count outside its limits before it writes: the buffers only have to exist)
        out = [_empty_like_mem((C_, Q), np.int64, x) for _ in range(6)]
        out += [_empty_like_mem((C_, Q, hs), np.int64, x), _empty_like_mem((Q,), np.int64, x)]
        return harr, C_, earr, narr, out

    def facet_stats_search(self, parent, store, x, nprobe, radius, metric, attrs, edges=None, filter=None, timing=False):
        """qk_facet_stats_search: per query, count / missing / min / max / exact sum / histogram of the Attr columns `attrs` (one
        Attr or a list of up to 4) over the hits of range_search with the same arguments.  edges: None, one ascending sequence of
        integers applied to every column, or a list with one sequence (or None) per column (quake_amd/where.py: lower_edges).
        Returns (count, missing, min, max, sum_lo, sum_hi [C, Q], hist [C, Q, 1 + the most edges of a column], total [Q][, timing])
        on x's device; the sum of (c, q) is sum_hi * 2**64 + (sum_lo mod 2**64), and min / max of a count of 0 are INT64_MAX /
        INT64_MIN."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        harr, C_, earr, narr, out = self._facet_stats_args(x, Q, attrs, edges)
        t = QkTiming()
        check(self.lib.qk_facet_stats_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe),
                                             metric_code(metric), float(radius), filter.h if filter is not None else None, harr, C_,
                                             earr, narr, *[_ptr(o) for o in out], mem, C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    def facet_stats_scan(self, store, x, pids, radius, metric, attrs, edges=None, filter=None, timing=False):
        """qk_facet_stats_scan: facet_stats_search over the given lists -- pids [Q, P] (or [P] for every query); -1 / absent / empty
        lists contribute nothing."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        harr, C_, earr, narr, out = self._facet_stats_args(x, Q, attrs, edges)
        t = QkTiming()
        check(self.lib.qk_facet_stats_scan(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]),
                                           metric_code(metric), float(radius), filter.h if filter is not None else None, harr, C_,
                                           earr, narr, *[_ptr(o) for o in out], mem, C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    # ---- ordered search ---------------------------------------------------------------------------------
    @staticmethod
    def _order_args(x, Q, k, descending, missing_last):
        k = int(k)
        flags = (QK_ORDER_DESC if descending else 0) | (QK_ORDER_MISSING_LAST if missing_last else 0)
        # (the library refuses a k outside its limits before it writes: the buffers of such a call only have to exist)
        kk = k if 1 <= k <= QK_MAX_ORDER_K else 1
        out = [_empty_like_mem((Q, kk), np.int64, x), _empty_like_mem((Q, kk), np.float32, x), _empty_like_mem((Q, kk), np.int64, x)]
        out += [_empty_like_mem((Q,), np.int64, x) for _ in range(3)]
        return k, flags, out

    def order_search(self, parent, store, x, nprobe, radius, metric, order_by, k, descending=False, missing_last=False, filter=None,
                     timing=False):
        """qk_order_search: per query, the k first hits of range_search with the same arguments ordered by the Attr column
        `order_by` (ascending, or descending), ties to the nearer row, then to the smaller id.  missing_last: hits whose id has no
        value follow those that have one instead of being left out.  Returns (ids [Q, k] padded with -1, dist [Q, k] padded as
        search pads, values [Q, k] (0 without a value), count, missing, total [Q][, timing]) on x's device."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        k, flags, out = self._order_args(x, Q, k, descending, missing_last)
        t = QkTiming()
        check(self.lib.qk_order_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe),
                                       metric_code(metric), float(radius), filter.h if filter is not None else None,
                                       order_by.h if order_by is not None else None, flags, k, *[_ptr(o) for o in out], mem,
                                       C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    def order_scan(self, store, x, pids, radius, metric, order_by, k, descending=False, missing_last=False, filter=None, timing=False):
        """qk_order_scan: order_search over the given lists -- pids [Q, P] (or [P] for every query); -1 / absent / empty lists
        contribute nothing."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        k, flags, out = self._order_args(x, Q, k, descending, missing_last)
        t = QkTiming()
        check(self.lib.qk_order_scan(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]),
                                     metric_code(metric), float(radius), filter.h if filter is not None else None,
                                     order_by.h if order_by is not None else None, flags, k, *[_ptr(o) for o in out], mem,
                                     C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    # ---- multi-vector search ------------------------------------------------------------------------------
    @staticmethod
    def _maxsim_args(x, n_tokens, k):
        """x [L, T, d] -> the flat sub-queries [L * T, d], L, T, n_tokens as int32 in x's memory, k, the output buffers"""
        if x.ndim != 3:
            raise ValueError("multi-vector queries are [L, T, d], got %d dimensions" % x.ndim)
        L, T = int(x.shape[0]), int(x.shape[1])
        xf = _f32(x).reshape(L * T, x.shape[2])
        nt = _i32_with(n_tokens, xf) if n_tokens is not None else None
        if nt is not None and nt.shape[0] != L:
            raise ValueError("n_tokens has %d entries for %d logical queries" % (nt.shape[0], L))
        k = int(k)
        # (the library refuses a k or T outside its limits before it writes: the buffers of such a call only have to exist)
        kk = k if 1 <= k <= QK_MAXSIM_MAX_K else 1
        out = [_empty_like_mem((L, kk), np.int64, xf), _empty_like_mem((L, kk), np.float32, xf), _empty_like_mem((L, kk), np.int32, xf),
               _empty_like_mem((L,), np.int64, xf), _empty_like_mem((L, T), np.int64, xf)]
        return xf, L, T, nt, k, out

    def maxsim_search(self, parent, store, x, nprobe, radius, metric, group_by, k, missing=0.0, n_tokens=None, filter=None, timing=False):
        """qk_maxsim_search: multi-vector (late interaction) search.  x [L, T, d]: T sub-queries per logical query; per logical query
        the k best values of the Attr column `group_by` by the sum over the sub-queries of the best hit of range_search (same
        arguments) among the rows of the value, `missing` where a sub-query has none; n_tokens [L]: only the first n_tokens[l]
        sub-queries take part.  Returns (groups [L, k] padded with 0, scores [L, k] padded as search pads, matched [L, k] int32,
        n_groups [L], hits [L, T][, timing]) on x's device."""
        xf, L, T, nt, k, out = self._maxsim_args(x, n_tokens, k)
        mem = _mem_of(xf)
        t = QkTiming()
        check(self.lib.qk_maxsim_search(self.h, parent.h if parent is not None else None, store.h, _ptr(xf), L, T, _ptr(nt), int(nprobe),
                                        metric_code(metric), float(radius), filter.h if filter is not None else None,
                                        group_by.h if group_by is not None else None, float(missing), k, *[_ptr(o) for o in out], mem,
                                        C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    def maxsim_scan(self, store, x, pids, radius, metric, group_by, k, missing=0.0, n_tokens=None, filter=None, timing=False):
        """qk_maxsim_scan: maxsim_search over the given lists -- pids [L, T, P] or [L * T, P] (or [P] for every sub-query); -1 /
        absent / empty lists contribute nothing."""
        xf, L, T, nt, k, out = self._maxsim_args(x, n_tokens, k)
        pids = _i64(pids)
        if pids.ndim == 3:
            pids = pids.reshape(L * T, pids.shape[2])
        pids = _pids_rows(pids, L * T)
        mem = _mem_of(xf, pids)
        t = QkTiming()
        check(self.lib.qk_maxsim_scan(self.h, store.h, _ptr(xf), L, T, _ptr(nt), _ptr(pids) if pids.shape[1] > 0 else None,
                                      int(pids.shape[1]), metric_code(metric), float(radius), filter.h if filter is not None else None,
                                      group_by.h if group_by is not None else None, float(missing), k, *[_ptr(o) for o in out], mem,
                                      C.byref(t) if timing else None))
        return (*out, timing_dict(t)) if timing else tuple(out)

    # ---- diversified search ------------------------------------------------------------------------------
    @staticmethod
    def _diverse_out(x, Q, k, fetch_k, want_dist, want_rank):
        # (the library refuses a k outside its limits before it writes: the buffers of such a call only have to exist)
        kk = k if 1 <= k <= fetch_k <= QK_MAX_FETCH_K else 1
        return (_empty_like_mem((Q, kk), np.int64, x), _empty_like_mem((Q, kk), np.float32, x) if want_dist else None,
                _empty_like_mem((Q, kk), np.int32, x) if want_rank else None)

    def diverse_search(self, parent, store, x, nprobe, k, fetch_k, lambda_mult, metric, filter=None, want_dist=True, want_rank=True,
                       timing=False):
        """qk_diverse_search: per query, k of the fetch_k nearest rows (the row search / search_filtered returns with k = fetch_k)
        chosen greedily by maximal marginal relevance with weight lambda_mult in [0, 1] (1: the plain top-k, 0: diversity only).
        Returns (ids [Q, k] in selection order padded with -1, dist [Q, k] padded as search pads, rank [Q, k] int32 -- the position
        of each pick in the candidate row, padding -1 --[, timing]) on x's device; dist / rank are None where not wanted."""
        x = _f32(x)
        Q = x.shape[0]
        mem = _mem_of(x)
        k, fetch_k = int(k), int(fetch_k)
        ids, dist, rank = self._diverse_out(x, Q, k, fetch_k, want_dist, want_rank)
        t = QkTiming()
        check(self.lib.qk_diverse_search(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, int(nprobe), k, fetch_k,
                                         float(lambda_mult), metric_code(metric), filter.h if filter is not None else None, _ptr(ids),
                                         _ptr(dist) if dist is not None else None, _ptr(rank) if rank is not None else None, mem,
                                         C.byref(t) if timing else None))
        return (ids, dist, rank, timing_dict(t)) if timing else (ids, dist, rank)

    def diverse_scan(self, store, x, pids, k, fetch_k, lambda_mult, metric, filter=None, want_dist=True, want_rank=True, timing=False):
        """qk_diverse_scan: diverse_search over the given lists -- pids [Q, P] (or [P] for every query); -1 / empty lists contribute
        nothing."""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        mem = _mem_of(x, pids)
        k, fetch_k = int(k), int(fetch_k)
        ids, dist, rank = self._diverse_out(x, Q, k, fetch_k, want_dist, want_rank)
        t = QkTiming()
        check(self.lib.qk_diverse_scan(self.h, store.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]), k,
                                       fetch_k, float(lambda_mult), metric_code(metric), filter.h if filter is not None else None,
                                       _ptr(ids), _ptr(dist) if dist is not None else None, _ptr(rank) if rank is not None else None,
                                       mem, C.byref(t) if timing else None))
        return (ids, dist, rank, timing_dict(t)) if timing else (ids, dist, rank)

    def search_aps(self, parent, store, x, k, metric, recall_target, recompute_threshold=0.001, use_precomputed=True,
                   initial_search_fraction=0.02, timing=False):
        """recall-target search (adaptive partition scanning).  Returns (ids, dist, nscanned[, timing])."""
        x = _f32(x)
        Q = x.shape[0]
        k = max(int(k), 1)
        mem = _mem_of(x)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        out_n = _empty_like_mem((Q,), np.int32, x)
        t = QkTiming()
        check(self.lib.qk_search_aps(self.h, parent.h if parent is not None else None, store.h, _ptr(x), Q, k, metric_code(metric),
                                     float(recall_target), float(recompute_threshold), int(bool(use_precomputed)),
                                     float(initial_search_fraction), _ptr(out_i), _ptr(out_d), _ptr(out_n), mem,
                                     C.byref(t) if timing else None))
        return (out_i, out_d, out_n, timing_dict(t)) if timing else (out_i, out_d, out_n)

    def merge_topk(self, ids, keys, metric):
        """ids/keys: CUDA tensors [G][Q][k] (keys = squared L2 / dot); returns ([Q][k] ids, [Q][k] distances)."""
        import torch
        ids, keys = _i64(ids), _f32(keys)
        G, Q, k = ids.shape
        out_i = torch.empty((Q, k), dtype=torch.int64, device=ids.device)
        out_d = torch.empty((Q, k), dtype=torch.float32, device=ids.device)
        check(self.lib.qk_merge_topk(self.h, _ptr(ids), _ptr(keys), G, Q, k, metric_code(metric), _ptr(out_i), _ptr(out_d)))
        return out_i, out_d

    def topk_block_bytes(self, per, k):
        return int(self.lib.qk_topk_block_bytes(int(per), int(k)))

    def pack_topk(self, ids, keys, G, out=None):
        """ids/keys: CUDA tensors [G*per][k] -> uint8 [G][block] send buffer of the one-collective exchange (block j = the
        entries of queries [j*per, (j+1)*per): ids then keys)."""
        import torch
        ids, keys = _i64(ids), _f32(keys)
        Q, k = ids.shape
        per = Q // int(G)
        blk = self.topk_block_bytes(per, k)
        if out is None or tuple(out.shape) != (int(G), blk) or out.device != ids.device:
            out = torch.empty((int(G), blk), dtype=torch.uint8, device=ids.device)
        check(self.lib.qk_pack_topk(self.h, _ptr(ids), _ptr(keys), int(G), per, k, _ptr(out)))
        return out

    def merge_topk_packed(self, packed, per, k, metric):
        """packed: uint8 [G][block] receive buffer (block r = rank r's entries for this rank's `per` queries)."""
        import torch
        G = packed.shape[0]
        out_i = torch.empty((per, k), dtype=torch.int64, device=packed.device)
        out_d = torch.empty((per, k), dtype=torch.float32, device=packed.device)
        check(self.lib.qk_merge_topk_packed(self.h, _ptr(packed), G, int(per), int(k), metric_code(metric), _ptr(out_i), _ptr(out_d)))
        return out_i, out_d

    MERGE_FORMS = {"rule": 0, "chain": 1, "flat": 2, "wide": 3}

    def merge_records(self, pair_slots, pair_head, rec_hdr, rec_ord, rec_id, k, metric, form=0, sqrt_l2=True, dist=True, cursor=False):
        """the per-query merge stage on caller-built records (qk_debug_merge_records; test and diagnosis hook).  CUDA tensors in the
        scan's layout: pair_slots int32 [Q, P, 32], pair_head int32 [Q, P], rec_hdr int32 [max_recs, 2], rec_ord int32 (the uint32
        keys' bits) [max_recs, k], rec_id int64 [max_recs, k].  form: 0 / "rule" = what a search launches, 1 / "chain", 2 / "flat",
        3 / "wide".  Returns a dict: ids [Q, k], dist [Q, k] (None with dist=False), kernel (the kernel launched) and, with
        cursor=True, next_key int32 [Q] (bits) / next_id int64 [Q]."""
        import torch
        Q, P = int(pair_head.shape[0]), int(pair_head.shape[1])
        k = int(k)
        max_recs = int(rec_hdr.shape[0])
        for t, dt, shape in ((pair_slots, torch.int32, (Q, P, 32)), (pair_head, torch.int32, (Q, P)), (rec_hdr, torch.int32, (max_recs, 2)),
                             (rec_ord, torch.int32, (max_recs, k)), (rec_id, torch.int64, (max_recs, k))):
            if not (_is_torch(t) and t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("merge_records: expected a contiguous CUDA %s tensor of shape %s" % (dt, shape))
        dev = pair_head.device
        out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
        out_d = torch.empty((Q, k), dtype=torch.float32, device=dev) if dist else None
        nk = torch.empty((Q,), dtype=torch.int32, device=dev) if cursor else None
        ni = torch.empty((Q,), dtype=torch.int64, device=dev) if cursor else None
        name = C.create_string_buffer(64)
        check(self.lib.qk_debug_merge_records(self.h, Q, P, k, metric_code(metric), int(bool(sqrt_l2)), int(self.MERGE_FORMS.get(form, form)),
                                              _ptr(pair_slots), _ptr(pair_head), _ptr(rec_hdr), _ptr(rec_ord), _ptr(rec_id), max_recs,
                                              _ptr(out_i), _ptr(out_d), _ptr(nk), _ptr(ni), name, 64))
        out = dict(ids=out_i, dist=out_d, kernel=name.value.decode())
        if cursor:
            out.update(next_key=nk, next_id=ni)
        return out

    def shadow_finish(self, store, x, E, lists, pair_slots, pair_head, rec_hdr, rec_ord, ent_list, ent_pos, k, metric, sqrt_l2=True, dist=True):
        """the exact finish of the fp16 shadow form on caller-built records over `store` (qk_debug_shadow_finish; test and diagnosis
        hook).  numpy arrays: x float32 [Q, d], E float32 [Q], lists int64 [Q] (the probed list, -1: none), pair_slots int32 [Q, 32],
        pair_head int32 [Q], rec_hdr int32 [max_recs, 2], rec_ord uint32 [max_recs, 32], ent_list / ent_pos int64 [max_recs, 32]
        (every entry's row: list number, position in the list).  Returns a dict: ids [Q, k], dist [Q, k] (None with dist=False) and
        what the call added to the counters verified / fallback / candidates / chained.  Malformed records raise, nothing runs."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        Q = int(x.shape[0])
        k = int(k)
        max_recs = int(rec_hdr.shape[0])
        arrs = []
        for a, dt, shape in ((E, np.float32, (Q,)), (lists, np.int64, (Q,)), (pair_slots, np.int32, (Q, 32)), (pair_head, np.int32, (Q,)),
                             (rec_hdr, np.int32, (max_recs, 2)), (rec_ord, np.uint32, (max_recs, 32)), (ent_list, np.int64, (max_recs, 32)),
                             (ent_pos, np.int64, (max_recs, 32))):
            a = np.ascontiguousarray(a, dtype=dt)
            if tuple(a.shape) != shape:
                raise ValueError("shadow_finish: expected a %s array of shape %s, got %s" % (np.dtype(dt).name, shape, tuple(a.shape)))
            arrs.append(a)
        if x.ndim != 2 or x.shape[1] != store.d:
            raise ValueError("shadow_finish: x must be [Q, %d]" % store.d)
        out_i = np.empty((Q, max(k, 0)), dtype=np.int64)
        out_d = np.empty((Q, max(k, 0)), dtype=np.float32) if dist else None
        cnt = np.zeros(4, dtype=np.int64)
        check(self.lib.qk_debug_shadow_finish(self.h, store.h, Q, k, metric_code(metric), int(bool(sqrt_l2)), _ptr(x), *[_ptr(a) for a in arrs],
                                              max_recs, _ptr(out_i), _ptr(out_d), _ptr(cnt)))
        return dict(ids=out_i, dist=out_d, verified=int(cnt[0]), fallback=int(cnt[1]), candidates=int(cnt[2]), chained=int(cnt[3]))

    # ---- k-means ----------------------------------------------------------------------------------------
    def kmeans_assign(self, x, c, metric, values=True):
        """nearest centroid of every row (and, with values, its distance / dot product); values=False passes val = NULL, the
        form the Lloyd driver uses (rows with a single candidate skip the exact key: qk_assign_pf.hip)."""
        x, c = _f32(x), _f32(c)
        n, d = x.shape
        mem = _mem_of(x, c)
        a = _empty_like_mem((n,), np.int64, x)
        v = _empty_like_mem((n,), np.float32, x) if values else None
        check(self.lib.qk_kmeans_assign(self.h, _ptr(x), n, _ptr(c), c.shape[0], d, metric_code(metric), _ptr(a),
                                        _ptr(v) if values else None, mem))
        return a, v

    def kmeans_assign_only(self, x, c, metric):
        """the assignments alone (val = NULL): what a Lloyd iteration needs"""
        return self.kmeans_assign(x, c, metric, values=False)[0]

    def kmeans_accumulate(self, x, assign, m, blocked=False):
        """per-centroid sums and counts.  blocked=False: rows added one after the other (the reference's refine loop,
        clustering.cpp:162-176); True: the blocked canonical order of the Lloyd driver (qk_kmeans_accumulate_blocked)."""
        x, assign = _f32(x), _i64(assign)
        n, d = x.shape
        mem = _mem_of(x, assign)
        sums = _empty_like_mem((m, d), np.float32, x)
        counts = _empty_like_mem((m,), np.int64, x)
        fn = self.lib.qk_kmeans_accumulate_blocked if blocked else self.lib.qk_kmeans_accumulate
        check(fn(self.h, _ptr(x), n, d, _ptr(assign), m, _ptr(sums), _ptr(counts), mem))
        return sums, counts

    def normalize_rows(self, x):
        """x /= ||x|| row by row, in place (canonical norm); returns x."""
        check(self.lib.qk_normalize_rows(self.h, _ptr(x), x.shape[0], x.shape[1], _mem_of(x)))
        return x

    def kmeans_update(self, sums, counts, centroids):
        """mean update + empty-cluster split of one Lloyd iteration; `centroids` and `counts` are updated in place."""
        m, d = centroids.shape
        check(self.lib.qk_kmeans_update(self.h, _ptr(sums), _ptr(counts), m, d, _ptr(centroids), _mem_of(sums, counts, centroids)))
        return centroids, counts

    def rand_perm(self, n, m, seed):
        out = np.empty(min(int(n), int(m)), np.int64)
        check(self.lib.qk_rand_perm(int(n), int(m), int(seed), _ptr(out)))
        return out

    def kmeans(self, x, m, metric, niter=5, seed=1234):
        """Returns (centroids, assign, x_used); x_used is the (IP-normalised) copy the caller should store."""
        x = _f32(x)
        x = x.clone() if _is_torch(x) else x.copy()
        n, d = x.shape
        mem = _mem_of(x)
        c = _empty_like_mem((m, d), np.float32, x)
        a = _empty_like_mem((n,), np.int64, x)
        check(self.lib.qk_kmeans(self.h, _ptr(x), n, d, m, metric_code(metric), int(niter), int(seed), _ptr(c), _ptr(a), mem))
        return c, a, x

    def kmeans_inplace(self, x, m, metric, centroids, assign, niter=5, seed=1234):
        """qk_kmeans on CUDA tensors the caller owns: x [n, d] (IP: normalised IN PLACE), centroids [m, d] and assign [n] written"""
        n, d = x.shape
        check(self.lib.qk_kmeans(self.h, _ptr(x), n, d, int(m), metric_code(metric), int(niter), int(seed), _ptr(centroids), _ptr(assign),
                                 QK_MEM_DEVICE))

    def kmeans_last_timing(self):
        """kernel-side ms of the assign / update step of the last Lloyd iteration of the last kmeans() (qk_kmeans_last_timing)"""
        am, um = C.c_float(0), C.c_float(0)
        rows, m = C.c_int64(0), C.c_int64(0)
        check(self.lib.qk_kmeans_last_timing(self.h, C.byref(am), C.byref(um), C.byref(rows), C.byref(m)))
        return dict(assign_ms=am.value, update_ms=um.value, rows=rows.value, m=m.value)


class Store:
    """Device mirror of faiss::DynamicInvertedLists (dynamic_inverted_list.h:25-33)."""

    def __init__(self, ctx, d):
        self.ctx = ctx
        self.lib = ctx.lib
        self.h = C.c_void_p()
        check(self.lib.qk_store_create(ctx.h, int(d), C.byref(self.h)))
        self.d = int(d)

    def close(self):
        if getattr(self, "h", None) and self.h and self.ctx.h:
            self.lib.qk_store_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self.lib.qk_store_reset(self.h))

    def add_list(self, list_no):
        check(self.lib.qk_store_add_list(self.h, int(list_no)))

    def remove_list(self, list_no):
        check(self.lib.qk_store_remove_list(self.h, int(list_no)))

    def add_entries(self, list_no, ids, vecs):
        ids, vecs = _i64(ids), _f32(vecs)
        n = ids.shape[0]
        check(self.lib.qk_store_add_entries(self.h, int(list_no), n, _ptr(ids), _ptr(vecs), _mem_of(ids, vecs)))

    def add_batch(self, ids, vecs, assign):
        ids, vecs, assign = _i64(ids), _f32(vecs), _i64(assign)
        check(self.lib.qk_store_add_batch(self.h, ids.shape[0], _ptr(ids), _ptr(vecs), _ptr(assign), _mem_of(ids, vecs, assign)))

    def build_csr(self, offsets, ids, vecs):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ids, vecs = _i64(ids), _f32(vecs)
        check(self.lib.qk_store_build_csr(self.h, offsets.shape[0] - 1, _ptr(offsets), _ptr(ids), _ptr(vecs),
                                          _mem_of(ids, vecs)))

    def remove_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = C.c_int64()
        check(self.lib.qk_store_remove_ids(self.h, ids.shape[0], _ptr(ids), C.byref(n)))
        return n.value

    def list_size(self, list_no):
        out = C.c_int64()
        check(self.lib.qk_store_list_size(self.h, int(list_no), C.byref(out)))
        return out.value

    def list_sizes(self, list_nos):
        """sizes of many lists in one call -> int64 array"""
        nos = np.ascontiguousarray(list_nos, dtype=np.int64).reshape(-1)
        out = np.empty(nos.shape[0], np.int64)
        if nos.shape[0]:
            check(self.lib.qk_store_list_sizes(self.h, _ptr(nos), nos.shape[0], _ptr(out)))
        return out

    def ntotal(self):
        return self.lib.qk_store_ntotal(self.h)

    def nlist(self):
        return self.lib.qk_store_nlist(self.h)

    def list_ids(self):
        n = C.c_int64()
        check(self.lib.qk_store_list_ids(self.h, None, C.byref(n)))
        out = np.empty(n.value, np.int64)
        if n.value:
            check(self.lib.qk_store_list_ids(self.h, _ptr(out), C.byref(n)))
        return out

    def get_list(self, list_no):
        n = self.list_size(list_no)
        vecs = np.empty((n, self.d), np.float32)
        ids = np.empty(n, np.int64)
        check(self.lib.qk_store_get_list(self.h, int(list_no), _ptr(vecs), _ptr(ids), QK_MEM_HOST))
        return vecs, ids

    def get_list_ids(self, list_no):
        """ids [n] of a list in row order, from the store's host mirror (qk_store_get_list with vecs = NULL: nothing is extracted)"""
        n = self.list_size(list_no)
        ids = np.empty(n, np.int64)
        if n:
            check(self.lib.qk_store_get_list(self.h, int(list_no), None, _ptr(ids), QK_MEM_HOST))
        return ids

    def get_list_device(self, list_no):
        """(vectors [n, d] as a CUDA tensor on the store's device -- extracted from the tile-major arena on the context's stream,
        no host hop -- , ids [n] as a host array: the store's own id mirror)"""
        import torch
        n = self.list_size(list_no)
        dev = torch.device("cuda", self.ctx.device)
        vecs = torch.empty((n, self.d), dtype=torch.float32, device=dev)
        ids = np.empty(n, np.int64)
        if n:
            check(self.lib.qk_store_get_list(self.h, int(list_no), _ptr(vecs), None, QK_MEM_DEVICE))
            check(self.lib.qk_store_get_list(self.h, int(list_no), None, _ptr(ids), QK_MEM_HOST))
        return vecs, ids

    def get_vectors(self, ids):
        """vectors of many ids in one call -> (float32 [n, d], bool [n] found)"""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        out = np.empty((ids.shape[0], self.d), np.float32)
        found = np.zeros(ids.shape[0], np.int32)
        if ids.shape[0]:
            check(self.lib.qk_store_get_vectors(self.h, _ptr(ids), ids.shape[0], _ptr(out), _ptr(found)))
        return out, found.astype(bool)

    def publish(self):
        """pending modifications become visible to searches now (list table upload, row-major copy) instead of inside the next query"""
        check(self.lib.qk_store_publish(self.h))

    def get_lists_device(self, list_nos, with_ids=False):
        """rows of many lists, one list after the other, as ONE CUDA tensor [sum of sizes, d] (qk_store_get_lists) + the sizes
        (+ with_ids: the rows' ids as a CUDA tensor)"""
        import torch
        nos = np.ascontiguousarray(list_nos, dtype=np.int64).reshape(-1)
        sizes = self.list_sizes(nos)
        dev = torch.device("cuda", self.ctx.device)
        vecs = torch.empty((int(sizes.sum()), self.d), dtype=torch.float32, device=dev)
        ids = torch.empty((vecs.shape[0],), dtype=torch.int64, device=dev) if with_ids else None
        if vecs.shape[0]:
            check(self.lib.qk_store_get_lists(self.h, _ptr(nos), nos.shape[0], _ptr(vecs), _ptr(ids) if with_ids else None, QK_MEM_DEVICE))
        return (vecs, sizes, ids) if with_ids else (vecs, sizes)

    def get_vector(self, vid):
        out = np.empty(self.d, np.float32)
        found = C.c_int()
        check(self.lib.qk_store_get_vector(self.h, int(vid), _ptr(out), C.byref(found)))
        return out if found.value else None

    def refine_lists(self, list_nos, centroids, metric, refinement_iterations=0):
        """kmeans_refine_partitions on the device store; returns the centroids used for the last assignment."""
        list_nos = np.ascontiguousarray(list_nos, dtype=np.int64)
        c = _f32(centroids)
        c = c.clone() if _is_torch(c) else c.copy()
        check(self.lib.qk_store_refine_lists(self.h, _ptr(list_nos), list_nos.shape[0], _ptr(c), metric_code(metric),
                                             int(refinement_iterations), _mem_of(c)))
        return c

    def device_bytes(self):
        return self.lib.qk_store_device_bytes(self.h)

    def shadow_info(self):
        """{valid, bytes, builds} of the store's fp16 shadow (qk_store_shadow_info)"""
        v, b, n = C.c_int(), C.c_int64(), C.c_int64()
        check(self.lib.qk_store_shadow_info(self.h, C.byref(v), C.byref(b), C.byref(n)))
        return {"valid": bool(v.value), "bytes": b.value, "builds": n.value}

    def shadow_drop(self):
        """free the fp16 shadow (qk_store_shadow_drop); eligible searches build it again"""
        check(self.lib.qk_store_shadow_drop(self.h))

    def exact_pool_info(self):
        """{slots, rows, cap_rows, builds, evictions, device_bytes} of the candidate pool of exact per-query search
        (qk_store_exact_pool_info); all 0 before the first Context.search_exact_batch and after exact_pool_drop"""
        v = [C.c_int64() for _ in range(6)]
        check(self.lib.qk_store_exact_pool_info(self.h, *[C.byref(a) for a in v]))
        return dict(zip(("slots", "rows", "cap_rows", "builds", "evictions", "device_bytes"), (a.value for a in v)))

    def exact_pool_drop(self):
        """free the candidate pool (qk_store_exact_pool_drop); filters stay valid and are admitted again on demand"""
        check(self.lib.qk_store_exact_pool_drop(self.h))

    COUNTER_NAMES = ("arena_reallocations", "arena_compactions", "list_relocations", "rows_copied", "rowmajor_rebuilds",
                     "table_uploads", "id_index_rebuilds", "context_scratch_reallocations")

    def counters(self):
        """what mutations cost beyond the rows they wrote (qk_store_counters), as a dict"""
        out = np.zeros(8, np.int64)
        check(self.lib.qk_store_counters(self.h, _ptr(out), 8))
        return dict(zip(self.COUNTER_NAMES, (int(v) for v in out)))


QK_MAX_BATCH_FILTERS = 4096  # include/quake_hip.h: most filters of one per-query call


class Filter:
    """A set of ids of one Store and a mode: "allow" (a row is a candidate iff its id is in the set) or "deny" (iff it is not).
    Pass it as `filter=` to Context.search / search_tracked / scan.  Defined by ids, not rows: it stays correct while the store
    changes (the row mask inside is re-derived at the next filtered call).  ids: numpy or torch, host or device."""

    MODES = {"allow": 0, "deny": 1}

    def __init__(self, store, ids, mode="allow"):
        if mode not in self.MODES:
            raise ValueError("Filter mode must be 'allow' or 'deny'")
        self.lib = store.lib
        self.store = store  # (keeps the store alive; the C object itself does not need it)
        self.mode = mode
        self.h = C.c_void_p()
        ids = _i64(ids).reshape(-1)
        check(self.lib.qk_filter_create(store.h, _ptr(ids) if ids.shape[0] > 0 else None, int(ids.shape[0]), self.MODES[mode],
                                        _mem_of(ids), C.byref(self.h)))

    OPS = {"range": _lib.QK_OP_RANGE, "not_range": _lib.QK_OP_NOT_RANGE, "any_bits": _lib.QK_OP_ANY_BITS,
           "all_bits": _lib.QK_OP_ALL_BITS, "no_bits": _lib.QK_OP_NO_BITS}

    @classmethod
    def where(cls, store, clauses):
        """A predicate filter (qk_filter_create_where): `clauses` is a sequence of (attr, op, a[, b]) -- attr an Attr of `store`,
        op one of OPS (or its QK_OP_* code), a / b int64 -- and a stored row is a candidate iff its id has a value in every
        clause's column that satisfies the clause.  It holds no ids and follows later Attr.set / unset and store changes."""
        clauses = list(clauses)
        arr = (_lib.QkClause * max(len(clauses), 1))()
        for i, cl in enumerate(clauses):
            attr, op, a = cl[0], cl[1], cl[2]
            b = cl[3] if len(cl) > 3 else 0
            arr[i].attr = attr.h if attr is not None else None
            arr[i].op = cls.OPS[op] if isinstance(op, str) else int(op)
            arr[i].a, arr[i].b = int(a), int(b)
        self = cls.__new__(cls)
        self.lib = store.lib
        self.store = store
        self.mode = "where"
        self.h = C.c_void_p()
        check(self.lib.qk_filter_create_where(store.h, arr, len(clauses), C.byref(self.h)))
        return self

    EXPR_OPS = dict(OPS, **{"in": _lib.QK_OP_IN_SET, "not_in": _lib.QK_OP_NOT_IN_SET})

    @classmethod
    def expr(cls, store, terms):
        """An expression filter (qk_filter_create_expr): `terms` is a sequence of sequences of (attr, op, a[, b]) as for where(),
        or (attr, "in" | "not_in", values) with values a host sequence / array of int64 (any order, duplicates allowed).  A
        stored row is a candidate iff for SOME term EVERY clause of it holds for the row's id.  Holds no ids; follows later
        Attr.set / unset and store changes like where()."""
        terms = [list(t) for t in terms]
        flat = [cl for t in terms for cl in t]
        arr = (_lib.QkExprClause * max(len(flat), 1))()
        sizes = (C.c_int * max(len(terms), 1))(*[len(t) for t in terms])
        keep = []  # the value arrays, alive until the call returns
        for i, cl in enumerate(flat):
            attr, op = cl[0], cl[1]
            code = cls.EXPR_OPS[op] if isinstance(op, str) else int(op)
            arr[i].attr = attr.h if attr is not None else None
            arr[i].op = code
            if code in (_lib.QK_OP_IN_SET, _lib.QK_OP_NOT_IN_SET):
                vals = np.ascontiguousarray(cl[2], dtype=np.int64).reshape(-1)
                keep.append(vals)
                arr[i].set = vals.ctypes.data_as(C.POINTER(C.c_int64)) if vals.shape[0] else None
                arr[i].n_set = vals.shape[0]
            else:
                arr[i].a, arr[i].b = int(cl[2]), int(cl[3]) if len(cl) > 3 else 0
        self = cls.__new__(cls)
        self.lib = store.lib
        self.store = store
        self.mode = "expr"
        self.h = C.c_void_p()
        check(self.lib.qk_filter_create_expr(store.h, arr, sizes, len(terms), C.byref(self.h)))
        return self

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.lib.qk_filter_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{n_ids, rows_allowed, store_version, rebuilds, device_bytes} (qk_filter_info)"""
        n, ra, rb, db = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        ver = C.c_uint64()
        check(self.lib.qk_filter_info(self.h, C.byref(n), C.byref(ra), C.byref(ver), C.byref(rb), C.byref(db)))
        return {"n_ids": n.value, "rows_allowed": ra.value, "store_version": ver.value, "rebuilds": rb.value,
                "device_bytes": db.value}

    def candidate_rows(self, ctx):
        """the candidate rows of the store NOW (qk_filter_candidate_rows): brings the mask up to date on ctx's stream"""
        n = C.c_int64()
        check(self.lib.qk_filter_candidate_rows(ctx.h, self.store.h, self.h, C.byref(n)))
        return n.value

    def exact_info(self):
        """{rows, builds, device_bytes} of the candidate store of exact search (qk_filter_exact_info)"""
        r, b, db = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.qk_filter_exact_info(self.h, C.byref(r), C.byref(b), C.byref(db)))
        return {"rows": r.value, "builds": b.value, "device_bytes": db.value}


class Attr:
    """An attribute column of one Store (qk_attr_*): a partial map vector id -> int64 kept on the device, keyed by id (nothing
    that moves or removes rows touches it).  Clauses of Filter.where name it.  ids / values: numpy or torch, host or device."""

    LAYOUTS = {_lib.QK_ATTR_TABLE: "table", _lib.QK_ATTR_SORTED: "sorted"}

    def __init__(self, store):
        self.lib = store.lib
        self.store = store
        self.h = C.c_void_p()
        check(self.lib.qk_attr_create(store.h, C.byref(self.h)))

    def close(self):
        """(filters that name the column keep its values and go on answering)"""
        if getattr(self, "h", None) and self.h:
            self.lib.qk_attr_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, ids, values):
        """upsert; of an id given twice the last value wins"""
        ids, values = _i64(ids).reshape(-1), _i64(values).reshape(-1)
        if ids.shape[0] != values.shape[0]:
            raise ValueError("Attr.set: %d ids, %d values" % (ids.shape[0], values.shape[0]))
        n = int(ids.shape[0])
        check(self.lib.qk_attr_set(self.h, _ptr(ids) if n else None, _ptr(values) if n else None, n, _mem_of(ids, values)))

    def unset(self, ids):
        ids = _i64(ids).reshape(-1)
        n = int(ids.shape[0])
        check(self.lib.qk_attr_unset(self.h, _ptr(ids) if n else None, n, _mem_of(ids)))

    def get(self, ids):
        """(values int64 [n], found bool [n]) as the device holds them; values are 0 where found is False"""
        if _is_torch(ids):
            ids = ids.detach().cpu().numpy()
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        vals = np.zeros(ids.shape[0], np.int64)
        found = np.zeros(ids.shape[0], np.int32)
        check(self.lib.qk_attr_get(self.h, _ptr(ids) if ids.shape[0] else None, int(ids.shape[0]), _ptr(vals), _ptr(found)))
        return vals, found.astype(bool)

    def info(self):
        """{n_ids, version, layout ("table" / "sorted"), device_bytes} (qk_attr_info)"""
        n, db = C.c_int64(), C.c_int64()
        ver = C.c_uint64()
        lay = C.c_int()
        check(self.lib.qk_attr_info(self.h, C.byref(n), C.byref(ver), C.byref(lay), C.byref(db)))
        return {"n_ids": n.value, "version": ver.value, "layout": self.LAYOUTS[lay.value], "device_bytes": db.value}

    def group_info(self):
        """{builds, device_bytes} of the per-row values grouped search keeps for this column (qk_attr_group_info): builds counts
        their derivations -- one per grouped call that found the store or the column changed"""
        b, db = C.c_int64(), C.c_int64()
        check(self.lib.qk_attr_group_info(self.h, C.byref(b), C.byref(db)))
        return {"builds": b.value, "device_bytes": db.value}


class Group:
    """Device group (qk_group_*): IndexBuildParams.num_workers as GPUs.  One process drives G members -- a context and a shard
    store each, list p in member p % G -- behind the Store surface (same method names; every call is routed to the member that
    holds the list) plus search() / scan() over the members.  `devices`: one HIP ordinal per member (repeats allowed)."""

    def __init__(self, devices, d):
        self.lib = _lib.load()
        devs = [int(v) for v in devices]
        arr = (C.c_int * len(devs))(*devs)
        self.h = C.c_void_p()
        check(self.lib.qk_group_create(arr, len(devs), int(d), C.byref(self.h)))
        self.devices = devs
        self.device = devs[0]
        self.d = int(d)

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.lib.qk_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(self.lib.qk_group_size(self.h))

    def owner(self, list_no):
        return int(self.lib.qk_group_owner(self.h, int(list_no)))

    def member_handles(self, i):
        """(qk_ctx*, qk_store*) of member i (borrowed)"""
        c, s = C.c_void_p(), C.c_void_p()
        check(self.lib.qk_group_member(self.h, int(i), C.byref(c), C.byref(s)))
        return c, s

    def member_list_ids(self, i):
        """list numbers member i holds"""
        _, s = self.member_handles(i)
        n = C.c_int64()
        check(self.lib.qk_store_list_ids(s, None, C.byref(n)))
        out = np.empty(n.value, np.int64)
        if n.value:
            check(self.lib.qk_store_list_ids(s, _ptr(out), C.byref(n)))
        return out

    def set_stream(self, hip_stream):
        """the lead's stream (see Context.set_stream)"""
        if hip_stream is None:
            check(self.lib.qk_group_set_stream(self.h, None))
        elif int(hip_stream) == 0:
            check(self.lib.qk_group_set_null_stream(self.h))
        else:
            check(self.lib.qk_group_set_stream(self.h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        check(self.lib.qk_group_synchronize(self.h))

    def set_form_feedback(self, enabled):
        check(self.lib.qk_group_set_form_feedback(self.h, int(bool(enabled))))

    def set_submit_threads(self, enabled):
        """one persistent enqueue thread per member (default) / everything on the caller's thread"""
        check(self.lib.qk_group_set_submit_threads(self.h, int(bool(enabled))))

    # ---- the Store surface ------------------------------------------------------------------------------------------------
    def reset(self):
        check(self.lib.qk_group_reset(self.h))

    def add_list(self, list_no):
        check(self.lib.qk_group_add_list(self.h, int(list_no)))

    def remove_list(self, list_no):
        check(self.lib.qk_group_remove_list(self.h, int(list_no)))

    def add_entries(self, list_no, ids, vecs):
        ids, vecs = _i64(ids), _f32(vecs)
        check(self.lib.qk_group_add_entries(self.h, int(list_no), ids.shape[0], _ptr(ids), _ptr(vecs), _mem_of(ids, vecs)))

    def add_batch(self, ids, vecs, assign):
        ids, vecs, assign = _i64(ids), _f32(vecs), _i64(assign)
        check(self.lib.qk_group_add_batch(self.h, ids.shape[0], _ptr(ids), _ptr(vecs), _ptr(assign), _mem_of(ids, vecs, assign)))

    def build_csr(self, offsets, ids, vecs):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        ids, vecs = _i64(ids), _f32(vecs)
        check(self.lib.qk_group_build_csr(self.h, offsets.shape[0] - 1, _ptr(offsets), _ptr(ids), _ptr(vecs), _mem_of(ids, vecs)))

    def remove_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = C.c_int64()
        check(self.lib.qk_group_remove_ids(self.h, ids.shape[0], _ptr(ids), C.byref(n)))
        return n.value

    def list_size(self, list_no):
        out = C.c_int64()
        check(self.lib.qk_group_list_size(self.h, int(list_no), C.byref(out)))
        return out.value

    def list_sizes(self, list_nos):
        nos = np.ascontiguousarray(list_nos, dtype=np.int64).reshape(-1)
        out = np.empty(nos.shape[0], np.int64)
        if nos.shape[0]:
            check(self.lib.qk_group_list_sizes(self.h, _ptr(nos), nos.shape[0], _ptr(out)))
        return out

    def ntotal(self):
        return self.lib.qk_group_ntotal(self.h)

    def nlist(self):
        return self.lib.qk_group_nlist(self.h)

    def list_ids(self):
        n = C.c_int64()
        check(self.lib.qk_group_list_ids(self.h, None, C.byref(n)))
        out = np.empty(n.value, np.int64)
        if n.value:
            check(self.lib.qk_group_list_ids(self.h, _ptr(out), C.byref(n)))
        return out

    def get_list(self, list_no):
        n = self.list_size(list_no)
        vecs = np.empty((n, self.d), np.float32)
        ids = np.empty(n, np.int64)
        check(self.lib.qk_group_get_list(self.h, int(list_no), _ptr(vecs), _ptr(ids), QK_MEM_HOST))
        return vecs, ids

    def get_list_ids(self, list_no):
        n = self.list_size(list_no)
        ids = np.empty(n, np.int64)
        if n:
            check(self.lib.qk_group_get_list(self.h, int(list_no), None, _ptr(ids), QK_MEM_HOST))
        return ids

    def get_list_device(self, list_no):
        """(vectors [n, d] as a CUDA tensor on the LEAD's device, written there by the owner; ids [n] as a host array)"""
        import torch
        n = self.list_size(list_no)
        vecs = torch.empty((n, self.d), dtype=torch.float32, device=torch.device("cuda", self.device))
        ids = np.empty(n, np.int64)
        if n:
            check(self.lib.qk_group_get_list(self.h, int(list_no), _ptr(vecs), None, QK_MEM_DEVICE))
            check(self.lib.qk_group_get_list(self.h, int(list_no), None, _ptr(ids), QK_MEM_HOST))
        return vecs, ids

    def get_lists_device(self, list_nos):
        import torch
        nos = np.ascontiguousarray(list_nos, dtype=np.int64).reshape(-1)
        sizes = self.list_sizes(nos)
        vecs = torch.empty((int(sizes.sum()), self.d), dtype=torch.float32, device=torch.device("cuda", self.device))
        if vecs.shape[0]:
            check(self.lib.qk_group_get_lists(self.h, _ptr(nos), nos.shape[0], _ptr(vecs), None, QK_MEM_DEVICE))
        return vecs, sizes

    def get_vector(self, vid):
        out = np.empty(self.d, np.float32)
        found = C.c_int()
        check(self.lib.qk_group_get_vector(self.h, int(vid), _ptr(out), C.byref(found)))
        return out if found.value else None

    def refine_lists(self, list_nos, centroids, metric, refinement_iterations=0):
        list_nos = np.ascontiguousarray(list_nos, dtype=np.int64)
        c = _f32(centroids)
        c = c.clone() if _is_torch(c) else c.copy()
        check(self.lib.qk_group_refine_lists(self.h, _ptr(list_nos), list_nos.shape[0], _ptr(c), metric_code(metric),
                                             int(refinement_iterations), _mem_of(c)))
        return c

    def device_bytes(self):
        return self.lib.qk_group_device_bytes(self.h)

    def counters(self):
        """Store.counters() summed over the members"""
        tot = np.zeros(8, np.int64)
        for i in range(self.size()):
            out = np.zeros(8, np.int64)
            check(self.lib.qk_store_counters(self.member_handles(i)[1], _ptr(out), 8))
            tot += out
        return dict(zip(Store.COUNTER_NAMES, (int(v) for v in tot)))

    # ---- search over the members ------------------------------------------------------------------------------------------
    def search(self, parent, x, nprobe, k, metric, timing=False, out=None):
        """QueryCoordinator::search with workers.  parent: the parent's Store (replicated per member by the library)."""
        x = _f32(x)
        Q = x.shape[0]
        if out is None:
            out_i = _empty_like_mem((Q, k), np.int64, x)
            out_d = _empty_like_mem((Q, k), np.float32, x)
        else:
            out_i, out_d = out
        t = QkTiming()
        check(self.lib.qk_group_search(self.h, parent.h, _ptr(x), Q, int(nprobe), int(k), metric_code(metric), _ptr(out_i),
                                       _ptr(out_d), _mem_of(x), C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)

    def search_aps(self, parent, x, k, metric, recall_target, recompute_threshold=0.001, use_precomputed=True,
                   initial_search_fraction=0.02, timing=False):
        """recall-target search over the members (qk_group_search_aps).  Returns (ids, dist, nscanned[, timing])."""
        x = _f32(x)
        Q = x.shape[0]
        k = max(int(k), 1)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        out_n = _empty_like_mem((Q,), np.int32, x)
        t = QkTiming()
        check(self.lib.qk_group_search_aps(self.h, parent.h, _ptr(x), Q, k, metric_code(metric), float(recall_target),
                                           float(recompute_threshold), int(bool(use_precomputed)), float(initial_search_fraction),
                                           _ptr(out_i), _ptr(out_d), _ptr(out_n), _mem_of(x), C.byref(t) if timing else None))
        return (out_i, out_d, out_n, timing_dict(t)) if timing else (out_i, out_d, out_n)

    def scan(self, x, pids, k, metric, timing=False):
        """scan_partitions with workers (worker_scan): pids [Q, P] (or [P]: the same set for every query), -1 = skip"""
        x, pids = _f32(x), _i64(pids)
        Q = x.shape[0]
        pids = _pids_rows(pids, Q)
        out_i = _empty_like_mem((Q, k), np.int64, x)
        out_d = _empty_like_mem((Q, k), np.float32, x)
        t = QkTiming()
        check(self.lib.qk_group_scan(self.h, _ptr(x), Q, _ptr(pids) if pids.shape[1] > 0 else None, int(pids.shape[1]), int(k),
                                     metric_code(metric), _ptr(out_i), _ptr(out_d), _mem_of(x, pids), C.byref(t) if timing else None))
        return (out_i, out_d, timing_dict(t)) if timing else (out_i, out_d)
