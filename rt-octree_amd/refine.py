"""The tree refiner (include/rto.h "refiner"; csrc/refine_kernels.hip, csrc/host/tree_refine.cpp): split the K leaves with the
largest keys into nodes of N^3 leaves that hold the leaf's record -- svox's N3Tree.refine(sel=...), the one structural step that
makes a tree finer.  The field is unchanged at every point; new nodes are appended; `slot_src` carries anything stored per slot
(the fit's float32 params, leaf weights) across the refinement by one gather.  The same bytes from the HIP kernels and from the
host twin.  A tool path (refine_octree.py, optimize_octree.py --refine_rounds), not a frame path."""
import ctypes as C

import numpy as np

from ._lib import CRefineStats, RtoError, check, lib
from .simplify import _shape_of
from .volrend import _stream_ptr

STAT_KEYS = ("reachable", "candidates", "selected", "levels", "cut_key")


def _stats_dict(st, cap_in, cap_out):
    d = {k: int(getattr(st, k)) for k in STAT_KEYS}
    d["capacity_in"], d["capacity"] = int(cap_in), int(cap_out)
    return d


def keys_from_weights(w):
    """The uint32 bit patterns of float32 weights (numpy array or torch tensor) clamped to [0, 1], a NaN to 0: for non-negative
    floats the bits order as unsigned integers the way the values do.  Nothing else is computed.  A torch tensor comes back as
    int32 (torch has no uint32 arithmetic; the kernels read the words as unsigned)."""
    if hasattr(w, "data_ptr"):
        import torch
        if w.dtype != torch.float32:
            raise RtoError(-1, "weights must be float32")
        return torch.where(w > 0, torch.clamp(w, max=1.0), torch.zeros_like(w)).contiguous().view(torch.int32)
    w = np.asarray(w)
    if w.dtype != np.float32:
        raise RtoError(-1, "weights must be float32")
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(np.where(w > 0, np.minimum(w, np.float32(1)), np.float32(0))).view(np.uint32)


def keys_from_density(data, sigma_thresh=0.0):
    """"Densest first": per slot the float32 bits of the density half (the last of the D) of data float16 [cap,N,N,N,D], and 0
    where the density is NaN or not > sigma_thresh -> uint32 [cap,N,N,N] (numpy)."""
    data = np.asarray(data)
    if data.dtype != np.float16 or data.ndim != 5:
        raise RtoError(-1, "data must be float16 [capacity,N,N,N,D]")
    sigma = np.ascontiguousarray(data[..., -1].astype(np.float32))
    with np.errstate(invalid="ignore"):
        live = sigma > np.float32(sigma_thresh)
    return np.where(live, sigma.view(np.uint32), np.uint32(0)).astype(np.uint32)


def _as_key(key, shape):
    if key is None:
        return None
    if hasattr(key, "data_ptr"):
        key = key.detach().cpu().numpy()
    key = np.ascontiguousarray(key)
    if key.dtype == np.int32 or key.dtype == np.float32:
        key = key.view(np.uint32)
    if key.dtype != np.uint32 or key.size != int(np.prod(shape)):
        raise RtoError(-1, "key must hold one uint32 per slot of child %s" % (list(shape),))
    return key


class Refiner:
    """rto_refiner: owns the scratch of the device entries (8 bytes per slot and 8 per node), which grows on demand and is
    reused across calls.  One instance serves one stream at a time."""

    def __init__(self, device=0):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_refiner_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def plan(self, child, key=None, key_thresh=1, max_new=-1, max_level=31, stream=None):
        """Pass 1 -> (capacity of the result, stats dict).  child: a contiguous torch int32 tensor [cap,N,N,N]; key: a contiguous
        int32 tensor (the uint32 words) with one element per slot, or None (every key is 1).  Synchronises the stream once."""
        import torch
        if not (hasattr(child, "data_ptr") and child.is_cuda and child.dtype == torch.int32 and child.is_contiguous() and child.dim() == 4
                and child.shape[1] == child.shape[2] == child.shape[3]):
            raise RtoError(-1, "child must be a contiguous int32 device tensor [capacity,N,N,N]")
        if key is not None and not (hasattr(key, "data_ptr") and key.is_cuda and key.dtype == torch.int32 and key.is_contiguous()
                                    and key.numel() == child.numel()):
            raise RtoError(-1, "key must be a contiguous int32 device tensor (the uint32 words) with one element per slot")
        if stream is None:
            stream = torch.cuda.current_stream(child.device)
        cap, st = C.c_int64(0), CRefineStats()
        check(lib().rto_tree_refine_plan(self._h, _stream_ptr(stream), C.c_void_p(child.data_ptr()),
                                         C.c_void_p(key.data_ptr()) if key is not None else None, int(child.shape[0]), int(child.shape[1]),
                                         int(key_thresh), int(max_new), int(max_level), C.byref(cap), C.byref(st)))
        return cap.value, _stats_dict(st, child.shape[0], cap.value)

    def write(self, child, data, capacity, stream=None, want_slot_src=True):
        """Pass 2 of the last plan -> (child_out, data_out, slot_src or None): device tensors of `capacity` nodes.  Enqueued on the
        stream and not waited for."""
        import torch
        if not (hasattr(data, "data_ptr") and data.is_cuda and data.dtype == torch.float16 and data.is_contiguous()):
            raise RtoError(-1, "data must be a contiguous float16 device tensor")
        cap, N, D = _shape_of(child.shape, data.shape)
        if stream is None:
            stream = torch.cuda.current_stream(child.device)
        child_out = torch.empty((capacity, N, N, N), dtype=torch.int32, device=child.device)
        data_out = torch.empty((capacity, N, N, N, D), dtype=torch.float16, device=child.device)
        slot_src = torch.empty((capacity, N, N, N), dtype=torch.int32, device=child.device) if want_slot_src else None
        check(lib().rto_tree_refine_write(self._h, _stream_ptr(stream), C.c_void_p(child.data_ptr()), C.c_void_p(data.data_ptr()), D,
                                          C.c_void_p(child_out.data_ptr()), C.c_void_p(data_out.data_ptr()),
                                          C.c_void_p(slot_src.data_ptr()) if want_slot_src else None))
        return child_out, data_out, slot_src

    def refine(self, child, data, key=None, key_thresh=1, max_new=-1, max_level=31, stream=None):
        """plan + write on device tensors -> (child_out, data_out, slot_src, stats)"""
        capacity, stats = self.plan(child, key, key_thresh, max_new, max_level, stream)
        return self.write(child, data, capacity, stream) + (stats,)

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_refiner_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def refine_tree_host(child, data, key=None, key_thresh=1, max_new=-1, max_level=31):
    """The host twin on numpy arrays: no device is touched.  -> (child, data, slot_src, stats)"""
    child = np.ascontiguousarray(child)
    data = np.ascontiguousarray(data)
    if child.dtype != np.int32 or data.dtype != np.float16:
        raise RtoError(-1, "child must be int32 and data float16")
    cap, N, D = _shape_of(child.shape, data.shape)
    key = _as_key(key, child.shape)
    kp = C.c_void_p(key.ctypes.data) if key is not None else None
    args = (C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), kp, cap, N, D, int(key_thresh), int(max_new), int(max_level))
    out_cap, st = C.c_int64(0), CRefineStats()
    check(lib().rto_tree_refine_host(*args, None, None, 0, C.byref(out_cap), None, C.byref(st)))
    k = out_cap.value
    child_out, data_out = np.empty((k, N, N, N), np.int32), np.empty((k, N, N, N, D), np.float16)
    slot_src = np.empty((k, N, N, N), np.int32)
    check(lib().rto_tree_refine_host(*args, C.c_void_p(child_out.ctypes.data), C.c_void_p(data_out.ctypes.data), k, C.byref(out_cap),
                                     C.c_void_p(slot_src.ctypes.data), C.byref(st)))
    return child_out, data_out, slot_src, _stats_dict(st, cap, k)


def refine_tree(child, data, key=None, key_thresh=1, max_new=-1, max_level=31, backend="hip", refiner=None, stream=None):
    """(child int32 [cap',N,N,N], data float16 [cap',N,N,N,D], slot_src int32 [cap',N,N,N], stats dict) as numpy arrays.  child /
    data / key: numpy arrays or torch tensors; key: one uint32 word per slot (keys_from_weights, keys_from_density) or None: every
    leaf within max_level is split.  backend "hip": the kernels (`refiner`: a Refiner to reuse, else one is made for the call);
    "cpu": the host twin, which never touches a GPU."""
    if backend == "cpu":
        if hasattr(child, "data_ptr"):
            child, data = child.detach().cpu().numpy(), data.detach().cpu().numpy()
        return refine_tree_host(child, data, key, key_thresh, max_new, max_level)
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    import torch
    dev = "cuda:%d" % (refiner.device if refiner is not None else 0)
    if not hasattr(child, "data_ptr"):
        child, data = np.ascontiguousarray(child), np.ascontiguousarray(data)
        if child.dtype != np.int32 or data.dtype != np.float16:
            raise RtoError(-1, "child must be int32 and data float16")
        child, data = torch.from_numpy(child), torch.from_numpy(data)
    _shape_of(child.shape, data.shape)
    if key is not None and not hasattr(key, "data_ptr"):
        key = torch.from_numpy(_as_key(key, child.shape).view(np.int32))
    if key is not None:
        if key.dtype == torch.float32:
            key = key.view(torch.int32)
        key = key.to(dev).contiguous()
    child, data = child.to(dev).contiguous(), data.to(dev).contiguous()
    r = refiner if refiner is not None else Refiner(child.device.index or 0)
    try:
        c, d, s, stats = r.refine(child, data, key, key_thresh, max_new, max_level, stream)
        if stream is not None:
            stream.synchronize()  # (the write is not waited for, and .cpu() waits for torch's current stream only)
        return c.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy(), stats
    finally:
        if refiner is None:
            r.free()
