"""The tree simplifier (include/rto.h "simplifier"; csrc/simplify_kernels.hip, csrc/host/tree_simplify.cpp): drop unreachable
nodes, optionally kill leaves under a density threshold, merge every node whose N^3 leaves hold one record into its parent slot,
and compact -- the same bytes from the HIP kernels and from the host twin, and the same field at every point.  A tool path
(simplify_octree.py), not a frame path: the device call returns after its stream has drained."""
import ctypes as C

import numpy as np

from ._lib import CSimplifyStats, RtoError, check, lib
from .volrend import _stream_ptr

STAT_KEYS = ("reachable", "unreachable", "killed", "merged", "levels")


def _thresh(kill_thresh):
    return float("nan") if kill_thresh is None else float(kill_thresh)


def _stats_dict(st, cap_in, cap_out):
    d = {k: int(getattr(st, k)) for k in STAT_KEYS}
    d["capacity_in"], d["capacity"] = int(cap_in), int(cap_out)
    return d


def _shape_of(child_shape, data_shape):
    """(cap, N, D) of child [cap, N, N, N] and data [cap, N, N, N, D]"""
    if len(child_shape) != 4 or len(data_shape) != 5 or tuple(data_shape[:4]) != tuple(child_shape) \
            or child_shape[1] != child_shape[2] or child_shape[2] != child_shape[3]:
        raise RtoError(-1, "child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s"
                       % (list(child_shape), list(data_shape)))
    return int(child_shape[0]), int(child_shape[1]), int(data_shape[4])


class Simplifier:
    """rto_simplifier: owns the scratch of the device entry (about 8 N^3 + 16 bytes per node), which grows on demand and is
    reused across calls.  One instance serves one stream at a time."""

    def __init__(self, device=0):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_simplifier_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def simplify(self, child, data, kill_thresh=None, stream=None, want_node_map=True):
        """child: a contiguous torch int32 tensor [cap,N,N,N], data: a contiguous half tensor [cap,N,N,N,D], both on this
        device -> (child_out, data_out, node_map or None, stats): device tensors cut to the new capacity (views of buffers of
        the old one) and a dict.  Synchronises the stream."""
        import torch
        for t, dt, what in ((child, torch.int32, "child must be a contiguous int32 device tensor"),
                            (data, torch.float16, "data must be a contiguous float16 device tensor")):
            if not (hasattr(t, "data_ptr") and t.is_cuda and t.dtype == dt and t.is_contiguous()):
                raise RtoError(-1, what)
        cap, N, D = _shape_of(child.shape, data.shape)
        child_out = torch.empty_like(child)
        data_out = torch.empty_like(data)
        node_map = torch.empty((max(cap, 1),), dtype=torch.int64, device=child.device) if want_node_map else None
        out_cap, st = C.c_int64(0), CSimplifyStats()
        check(lib().rto_tree_simplify(self._h, _stream_ptr(stream), C.c_void_p(child.data_ptr()), C.c_void_p(data.data_ptr()), cap,
                                      N, D, _thresh(kill_thresh), C.c_void_p(child_out.data_ptr()), C.c_void_p(data_out.data_ptr()),
                                      C.byref(out_cap), C.c_void_p(node_map.data_ptr()) if want_node_map else None, C.byref(st)))
        k = out_cap.value
        return child_out[:k], data_out[:k], (node_map[:k] if want_node_map else None), _stats_dict(st, cap, k)

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_simplifier_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def simplify_tree_host(child, data, kill_thresh=None):
    """The host twin on numpy arrays: no device is touched.  -> (child, data, node_map, stats)"""
    child = np.ascontiguousarray(child)
    data = np.ascontiguousarray(data)
    if child.dtype != np.int32 or data.dtype != np.float16:
        raise RtoError(-1, "child must be int32 and data float16")
    cap, N, D = _shape_of(child.shape, data.shape)
    child_out, data_out = np.empty_like(child), np.empty_like(data)
    node_map = np.empty((max(cap, 1),), np.int64)
    out_cap, st = C.c_int64(0), CSimplifyStats()
    check(lib().rto_tree_simplify_host(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), cap, N, D, _thresh(kill_thresh),
                                       C.c_void_p(child_out.ctypes.data), C.c_void_p(data_out.ctypes.data), C.byref(out_cap),
                                       C.c_void_p(node_map.ctypes.data), C.byref(st)))
    k = out_cap.value
    return child_out[:k].copy(), data_out[:k].copy(), node_map[:k].copy(), _stats_dict(st, cap, k)


def simplify_tree(child, data, kill_thresh=None, backend="hip", simplifier=None, stream=None):
    """(child int32 [cap',N,N,N], data float16 [cap',N,N,N,D], node_map int64 [cap'], stats dict) as numpy arrays.  child / data:
    numpy arrays or torch tensors.  kill_thresh None: lossless.  backend "hip": the kernels (`simplifier`: a Simplifier to reuse,
    else one is made for the call); "cpu": the host twin, which never touches a GPU."""
    if backend == "cpu":
        if hasattr(child, "data_ptr"):
            child, data = child.detach().cpu().numpy(), data.detach().cpu().numpy()
        return simplify_tree_host(child, data, kill_thresh)
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    import torch
    dev = "cuda:%d" % (simplifier.device if simplifier is not None else 0)
    if not hasattr(child, "data_ptr"):
        child, data = np.ascontiguousarray(child), np.ascontiguousarray(data)
        if child.dtype != np.int32 or data.dtype != np.float16:
            raise RtoError(-1, "child must be int32 and data float16")
        child, data = torch.from_numpy(child), torch.from_numpy(data)
    child, data = child.to(dev).contiguous(), data.to(dev).contiguous()
    s = simplifier if simplifier is not None else Simplifier(child.device.index or 0)
    try:
        c, d, m, stats = s.simplify(child, data, kill_thresh, stream)
        return c.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy(), stats
    finally:
        if simplifier is None:
            s.free()
