"""The grid builder (include/rto.h "grid builder"; csrc/build_kernels.hip, csrc/host/grid_build.cpp): a dense grid of records
[R,R,R,D], R = 2^L, becomes the octree child[] / data[] whose uniform cells are leaves -- the same bytes from the HIP kernels and
from the host twin, and the bytes the simplifier leaves of the grid's full octree.  tree_to_grid is the way back: the tree
sampled at the voxel centres through rto_tree_query.  A tool path (grid_to_octree.py), not a frame path."""
import ctypes as C

import numpy as np

from ._lib import CGridBuildStats, RtoError, check, lib
from .volrend import _stream_ptr

STAT_KEYS = ("nodes", "killed", "levels")


def _thresh(kill_thresh):
    return float("nan") if kill_thresh is None else float(kill_thresh)


def _stats_dict(st):
    return {k: int(getattr(st, k)) for k in STAT_KEYS}


def _shape_of(shape):
    """(L, D) of a grid [R, R, R, D] with R = 2^L"""
    if len(shape) != 4 or shape[0] != shape[1] or shape[1] != shape[2]:
        raise RtoError(-1, "grid must be [R,R,R,D], not %s" % (list(shape),))
    R = int(shape[0])
    L = R.bit_length() - 1
    if R < 1 or (1 << L) != R:
        raise RtoError(-1, "the side of the grid must be a power of two, not %d" % R)
    return L, int(shape[3])


class TreeBuilder:
    """rto_tree_builder: owns the scratch of the device entries (5/7 of a byte per voxel), which grows on demand and is reused
    across calls.  One instance serves one stream at a time."""

    def __init__(self, device=0):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_tree_builder_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def build(self, grid, kill_thresh=None, stream=None):
        """grid: a contiguous torch half tensor [R,R,R,D] on this device -> (child int32 [nodes,2,2,2], data half
        [nodes,2,2,2,D], stats dict): device tensors.  The plan synchronises the stream once (the outputs cannot be sized
        before); the writing kernels are enqueued on it and not waited for."""
        import torch
        if not (hasattr(grid, "data_ptr") and grid.is_cuda and grid.dtype == torch.float16 and grid.is_contiguous()):
            raise RtoError(-1, "grid must be a contiguous float16 device tensor")
        L, D = _shape_of(grid.shape)
        if stream is None:
            stream = torch.cuda.current_stream(grid.device)
        cap, st = C.c_int64(0), CGridBuildStats()
        check(lib().rto_tree_build_plan(self._h, _stream_ptr(stream), C.c_void_p(grid.data_ptr()), L, D, _thresh(kill_thresh),
                                        C.byref(cap), C.byref(st)))
        child = torch.empty((cap.value, 2, 2, 2), dtype=torch.int32, device=grid.device)
        data = torch.empty((cap.value, 2, 2, 2, D), dtype=torch.float16, device=grid.device)
        check(lib().rto_tree_build_write(self._h, _stream_ptr(stream), C.c_void_p(child.data_ptr()), C.c_void_p(data.data_ptr())))
        return child, data, _stats_dict(st)

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_tree_builder_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_half_grid(grid):
    grid = np.asarray(grid)
    if grid.dtype == np.float32:
        with np.errstate(over="ignore"):
            grid = grid.astype(np.float16)
    if grid.dtype != np.float16:
        raise RtoError(-1, "grid must be float16 or float32, not %s" % grid.dtype)
    return np.ascontiguousarray(grid)


def build_tree_host(grid, kill_thresh=None):
    """The host twin on a numpy grid: no device is touched.  -> (child, data, stats)"""
    grid = _as_half_grid(grid)
    L, D = _shape_of(grid.shape)
    cap, st = C.c_int64(0), CGridBuildStats()
    check(lib().rto_tree_build_host(C.c_void_p(grid.ctypes.data), L, D, _thresh(kill_thresh), None, None, 0, C.byref(cap), C.byref(st)))
    child = np.empty((cap.value, 2, 2, 2), np.int32)
    data = np.empty((cap.value, 2, 2, 2, D), np.float16)
    check(lib().rto_tree_build_host(C.c_void_p(grid.ctypes.data), L, D, _thresh(kill_thresh), C.c_void_p(child.ctypes.data),
                                    C.c_void_p(data.ctypes.data), cap.value, C.byref(cap), C.byref(st)))
    return child, data, _stats_dict(st)


def build_tree(grid, kill_thresh=None, backend="hip", builder=None, stream=None):
    """(child int32 [nodes,2,2,2], data float16 [nodes,2,2,2,D], stats dict) as numpy arrays from a numpy grid [R,R,R,D], float16
    or float32 (rounded to fp16 by numpy first).  kill_thresh None: no voxel is killed.  backend "hip": the kernels (`builder`: a
    TreeBuilder to reuse, else one is made for the call); "cpu": the host twin, which never touches a GPU."""
    if backend == "cpu":
        return build_tree_host(grid, kill_thresh)
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    import torch
    grid = _as_half_grid(grid)
    _shape_of(grid.shape)
    b = builder if builder is not None else TreeBuilder(0)
    try:
        dev = torch.device("cuda", b.device)
        c, d, stats = b.build(torch.from_numpy(grid).to(dev), kill_thresh, stream)
        return c.cpu().numpy(), d.cpu().numpy(), stats
    finally:
        if builder is None:
            b.free()


def tree_to_grid(tree, L, chunk_points=1 << 22):
    """An uploaded N3Tree sampled at the R^3 voxel centres (i + 0.5) / R of tree space, R = 2^L, through rto_tree_query -> a half
    device tensor [R,R,R,D] (the query widens the leaf's halves to float32; narrowing them again is exact).  The centres lie
    half a voxel from any cell face of levels <= L, so for L <= 10 the float32 mapping to world space and back cannot move one
    across a face."""
    import torch
    L = int(L)
    if L < 1 or L > 10:
        raise RtoError(-1, "L must lie in 1 .. 10, not %d" % L)
    R = 1 << L
    dev = torch.device("cuda", tree.device)
    D = int(tree.data_dim)
    out = torch.empty((R, R, R, D), dtype=torch.float16, device=dev)
    centre = (torch.arange(R, dtype=torch.float64, device=dev) + 0.5) / R
    scale = torch.as_tensor(np.asarray(tree.scale, np.float64), device=dev)
    offset = torch.as_tensor(np.asarray(tree.offset, np.float64), device=dev)
    world = [(centre - offset[a]) / scale[a] for a in range(3)]  # tree = offset + scale * world
    slabs = max(1, min(R, int(chunk_points) // (R * R)))
    for x0 in range(0, R, slabs):
        x1 = min(R, x0 + slabs)
        pts = torch.stack(torch.meshgrid(world[0][x0:x1], world[1], world[2], indexing="ij"), -1).reshape(-1, 3)
        vals = tree.query(pts.to(torch.float32).contiguous(), values=True)["values"]
        out[x0:x1] = vals.reshape(x1 - x0, R, R, D).to(torch.float16)
    return out
