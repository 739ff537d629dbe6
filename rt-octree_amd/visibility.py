"""Per-leaf peak compositing weights over a set of cameras (include/rto.h "leaf weights"; csrc/leaf_weight_kernels.hip,
csrc/host/leaf_weights.cpp): for every leaf slot the largest T * (1 - exp(-sigma * delta)) any pixel's ray of any camera gives
it -- what the pruning step of PlenOctree extraction records.  A dense leaf buried behind an opaque surface has weight 0.  The
kernel and the host twin give the same bits; prune_octree.py is the tool built on them."""
import ctypes as C

import numpy as np

from ._lib import CCamera, RtoError, check, lib
from .volrend import Camera, RenderOptions, _stream_ptr


def _cam_array(cams):
    if isinstance(cams, Camera):
        cams = [cams]
    cams = list(cams)
    return (CCamera * max(len(cams), 1))(*[c.to_c() for c in cams]), len(cams)


def _options(options):
    return (RenderOptions() if options is None else options).to_c()


def leaf_weights(tree, cams, options=None, out=None, stream=None):
    """rto_tree_leaf_weights: the weights of the N3Tree `tree` over `cams` (a Camera or a sequence; any number, mixed sizes) as a
    float32 torch tensor [capacity, N, N, N] on the tree's device, indexed like the child array the tree was uploaded from.
    out: a tensor of an earlier call to accumulate into (max), else a zeroed one is made.  Of `options` (a RenderOptions; None:
    the defaults) step_size, sigma_thresh, stop_thresh and render_bbox are read.  Asynchronous on `stream` (default: torch's
    current stream); no sync."""
    import torch
    device = torch.device("cuda", tree.device)
    shape = (int(tree.capacity), int(tree.N), int(tree.N), int(tree.N))
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != shape
          or out.device != device):
        raise RtoError(-1, "out must be a contiguous float32 tensor of shape %s on %s" % (list(shape), device))
    arr, n = _cam_array(cams)
    co = _options(options)
    if stream is None:
        stream = torch.cuda.current_stream(device)
    check(lib().rto_tree_leaf_weights(tree._h, arr, n, C.byref(co), C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def leaf_weights_host(child, data, scale, offset, cams, options=None, ndc=None, threads=0, out=None):
    """rto_leaf_weights_host: the same weights from numpy arrays (child int32 [capacity,N,N,N], data float16 or uint16 bits
    [capacity,N,N,N,D]) as a numpy float32 array [capacity,N,N,N]; no device is touched.  ndc: (width, height, focal) of an NDC
    tree.  threads <= 0: one thread; the result does not depend on it.  out: an array of an earlier call to accumulate into."""
    child = np.ascontiguousarray(child)
    data = np.ascontiguousarray(data)
    if data.dtype == np.float16:
        data = data.view(np.uint16)
    if child.dtype != np.int32 or data.dtype != np.uint16:
        raise RtoError(-1, "child must be int32 and data float16")
    if child.ndim != 4 or data.ndim != 5 or data.shape[:4] != child.shape or not (child.shape[1] == child.shape[2] == child.shape[3]):
        raise RtoError(-1, "child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s"
                       % (list(child.shape), list(data.shape)))
    if out is None:
        out = np.zeros(child.shape, np.float32)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.shape == child.shape):
        raise RtoError(-1, "out must be a contiguous float32 array of shape %s" % (list(child.shape),))
    sc = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(scale, np.float32), (3,))])
    of = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(offset, np.float32), (3,))])
    nd = None if ndc is None else (C.c_float * 3)(*[float(x) for x in ndc])
    arr, n = _cam_array(cams)
    co = _options(options)
    check(lib().rto_leaf_weights_host(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), child.shape[0], child.shape[1],
                                      data.shape[4], sc, of, nd, arr, n, C.byref(co), int(threads), C.c_void_p(out.ctypes.data)))
    return out


def kill_unseen(child, data, weights, weight_thresh):
    """A copy of `data` (float16 [capacity,N,N,N,D]) in which the density half (the last of the D) is +0 for every leaf slot
    (child == 0) whose weight is < weight_thresh -- with weight_thresh == 0: whose weight is 0.  Nothing else changes."""
    child = np.asarray(child)
    data = np.asarray(data)
    weights = np.asarray(weights, np.float32)
    if data.dtype != np.float16 or data.ndim != 5 or data.shape[:4] != child.shape or weights.shape != child.shape:
        raise RtoError(-1, "data must be float16 [capacity,N,N,N,D], child and weights [capacity,N,N,N]")
    if not weight_thresh >= 0:
        raise RtoError(-1, "weight_thresh must be >= 0")
    th = np.float32(weight_thresh)
    dead = (child == 0) & ((weights == 0) if th == 0 else (weights < th))
    out = data.copy()
    out[..., -1].view(np.uint16)[dead] = 0
    return out
