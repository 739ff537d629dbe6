"""Fine-tuning a tree's leaf values against training images (include/rto.h "tree fit"; csrc/fit_kernels.hip,
csrc/host/fit_grad.cpp): the deterministic composited render of the field `params` over a fixed tree, its squared error against
target images, and the gradient with respect to params accumulated in 64-bit fixed point -- so that the kernel, the host twin
and any split of the cameras over calls give the same bytes.  The sparse step (csrc/fit_sparse_kernels.hip, csrc/host/fit_sparse.cpp):
the ray entry can mark the leaves it reached in a bitmap, touched_list turns the bitmap into a list, and step_sparse steps the
listed rows only, with SGD, RMSProp or Adam.  optimize_octree.py is the tool built on them."""
import ctypes as C

import numpy as np

from ._lib import RtoError, check, lib
from .visibility import _cam_array, _options
from .volrend import _stream_ptr

FIX_SCALE = 2.0 ** 36  # a grad / loss word counts units of 2^-36


def _ptr_array(ptrs, n):
    arr = (C.c_void_p * max(n, 1))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def _planes(cams, planes, n, what, is_ok, ptr_of, optional_entries):
    """the per-camera [H][W][3] float32 planes of a call -> a ctypes pointer array or None"""
    if planes is None:
        return None
    planes = list(planes)
    if len(planes) != n:
        raise RtoError(-1, "%s: %d planes for %d cameras" % (what, len(planes), n))
    ptrs = []
    for f, (c, p) in enumerate(zip(cams, planes)):
        if p is None and optional_entries:
            ptrs.append(None)
            continue
        if not is_ok(p) or tuple(p.shape) != (int(c.height), int(c.width), 3):
            raise RtoError(-1, "%s %d must be a contiguous float32 [%d, %d, 3]" % (what, f, c.height, c.width))
        ptrs.append(ptr_of(p))
    return _ptr_array(ptrs, n)


def _cam_list(cams):
    from .volrend import Camera
    return [cams] if isinstance(cams, Camera) else list(cams)


def fit_grad(tree, params, cams, targets=None, options=None, grad=None, stats=None, images=None, stream=None):
    """rto_tree_fit_grad on the N3Tree `tree`: params float32 [capacity,N,N,N,D], targets / images per camera float32 [H,W,3]
    (an entry of images may be None), grad int64 like params or None (forward only), stats int64 [2] or None -- torch tensors on
    the tree's device.  Accumulates into grad and stats.  Asynchronous on `stream` (default: torch's current stream); no sync."""
    import torch
    device = torch.device("cuda", tree.device)
    shape = (int(tree.capacity), int(tree.N), int(tree.N), int(tree.N), int(tree.data_dim))

    def on_device(t, dtype, shp=None):
        return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device == device
                and (shp is None or tuple(t.shape) == shp))

    if not on_device(params, torch.float32, shape):
        raise RtoError(-1, "params must be a contiguous float32 tensor of shape %s on %s" % (list(shape), device))
    if grad is not None and not on_device(grad, torch.int64, shape):
        raise RtoError(-1, "grad must be a contiguous int64 tensor of shape %s on %s" % (list(shape), device))
    if stats is not None and not on_device(stats, torch.int64, (2,)):
        raise RtoError(-1, "stats must be a contiguous int64 tensor of shape [2] on %s" % device)
    cams = _cam_list(cams)
    arr, n = _cam_array(cams)
    ok = lambda t: on_device(t, torch.float32)  # noqa: E731
    tg = _planes(cams, targets, n, "target", ok, lambda t: t.data_ptr(), False)
    im = _planes(cams, images, n, "image", ok, lambda t: t.data_ptr(), True)
    co = _options(options)
    if stream is None:
        stream = torch.cuda.current_stream(device)
    check(lib().rto_tree_fit_grad(tree._h, C.c_void_p(params.data_ptr()), arr, tg, im, n, C.byref(co),
                                  C.c_void_p(grad.data_ptr()) if grad is not None else None,
                                  C.c_void_p(stats.data_ptr()) if stats is not None else None, _stream_ptr(stream)))
    return grad


def fit_grad_rays(tree, params, origins, dirs, targets=None, options=None, grad=None, stats=None, out=None, stream=None, touched=None):
    """rto_tree_fit_grad_rays: fit_grad on n rays of the caller's.  origins / dirs [n,3] (dirs of any length), targets [n,3] or
    None (a NaN masks its ray), out [n,3] or None (where the composited colours go): contiguous float32 torch tensors on the
    tree's device, or numpy arrays (copied over; pass a tensor for `out`) -- volrend._ray_tensor's rules.  volrend.camera_rays(cam)
    gives the rays on which this is fit_grad on the camera, bit for bit.  params, grad, stats as fit_grad takes them.
    Accumulates into grad and stats.  Asynchronous on `stream` (default: torch's current stream); no sync.
    touched: None, or the bitmap of the sparse step, an int32 tensor [touched_words(slots)] on the device: the call goes through
    rto_tree_fit_grad_rays_touched (grad is then required) and sets the bit of every leaf its backward march reached."""
    import torch
    from .volrend import _ray_tensor
    device = torch.device("cuda", tree.device)
    shape = (int(tree.capacity), int(tree.N), int(tree.N), int(tree.N), int(tree.data_dim))

    def on_device(t, dtype, shp):
        return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device == device and tuple(t.shape) == shp

    if not on_device(params, torch.float32, shape):
        raise RtoError(-1, "params must be a contiguous float32 tensor of shape %s on %s" % (list(shape), device))
    if grad is not None and not on_device(grad, torch.int64, shape):
        raise RtoError(-1, "grad must be a contiguous int64 tensor of shape %s on %s" % (list(shape), device))
    if stats is not None and not on_device(stats, torch.int64, (2,)):
        raise RtoError(-1, "stats must be a contiguous int64 tensor of shape [2] on %s" % device)
    words = touched_words(shape[0] * shape[1] ** 3)
    if touched is not None and not on_device(touched, torch.int32, (words,)):
        raise RtoError(-1, "touched must be a contiguous int32 tensor of shape [%d] on %s" % (words, device))
    n = int(origins.shape[0])
    o = _ray_tensor(origins, "origins", 3, n, device)
    d = _ray_tensor(dirs, "dirs", 3, n, device)
    tg = None if targets is None else _ray_tensor(targets, "targets", 3, n, device)
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch tensor: it is written")
    ou = None if out is None else _ray_tensor(out, "out", 3, n, device)
    if n == 0:  # (an empty tensor has no address to pass; the entry launches nothing)
        return grad
    co = _options(options)
    if stream is None:
        stream = torch.cuda.current_stream(device)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    if touched is not None:
        check(lib().rto_tree_fit_grad_rays_touched(tree._h, ptr(params), ptr(o), ptr(d), ptr(tg), ptr(ou), n, C.byref(co), ptr(grad),
                                                   ptr(stats), ptr(touched), _stream_ptr(stream)))
        return grad
    check(lib().rto_tree_fit_grad_rays(tree._h, ptr(params), ptr(o), ptr(d), ptr(tg), ptr(ou), n, C.byref(co), ptr(grad), ptr(stats),
                                       _stream_ptr(stream)))
    return grad


KINDS = {"sgd": 0, "rmsprop": 1, "adam": 2}  # RTO_FIT_SGD, RTO_FIT_RMSPROP, RTO_FIT_ADAM


def touched_words(slots):
    """words of the touched bitmap of `slots` = capacity * N^3 leaves"""
    return (int(slots) + 31) // 32


def touched_block_words():
    """bitmap words per workgroup of the device list (RTO_FIT_TOUCHED_BLOCK_WORDS)"""
    return int(lib().rto_fit_touched_block_words())


def touched_scratch_bytes(slots):
    """bytes of scratch touched_list needs on the device"""
    n = int(lib().rto_fit_touched_scratch_bytes(int(slots)))
    if n < 0:
        raise RtoError(-1, "slots must be in [0, 2^31)")
    return n


def fit_optim(kind="sgd", lr=0.0, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, t=1):
    """the rto_fit_optim of step t (1-based) of an optimiser: bias1 / bias2 = float32(1 - float32(beta)^t), computed here in
    double from the float32 betas, so that every backend gets the same floats"""
    from ._lib import CFitOptim
    if kind not in KINDS:
        raise RtoError(-1, "optimizer must be one of %s, not %r" % (sorted(KINDS), kind))
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return CFitOptim(KINDS[kind], float(lr), float(grad_scale), b1, b2, float(np.float32(eps)),
                     float(np.float32(1.0 - b1 ** int(t))), float(np.float32(1.0 - b2 ** int(t))))


def touched_list(touched, slots, list_, count, scratch, clear=True, stream=None):
    """rto_fit_touched_list: the set slots of the bitmap `touched` (int32 [touched_words(slots)]) in ascending order to `list_`
    (int32 [list_capacity]), their number to count (int64 [1]); scratch: a uint8 tensor of touched_scratch_bytes(slots) bytes.
    clear: the bitmap is zeroed in the same pass.  Tensors of one device.  Asynchronous; no sync."""
    import torch
    for t, dt, what in ((touched, torch.int32, "touched"), (list_, torch.int32, "list"), (count, torch.int64, "count"),
                        (scratch, torch.uint8, "scratch")):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.is_cuda and t.device == touched.device):
            raise RtoError(-1, "%s must be a contiguous %s tensor on the device of touched" % (what, dt))
    if touched.numel() != touched_words(slots) or count.numel() != 1:
        raise RtoError(-1, "touched must hold %d words and count one" % touched_words(slots))
    if stream is None:
        stream = torch.cuda.current_stream(touched.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
    check(lib().rto_fit_touched_list(ptr(touched) or C.c_void_p(scratch.data_ptr()), int(slots), int(bool(clear)), ptr(list_), list_.numel(),
                                     ptr(count), ptr(scratch), scratch.numel(), _stream_ptr(stream)))
    return list_


def step_sparse(params, grad, list_, count, optim, m=None, v=None, stream=None):
    """rto_fit_step_sparse: the step of `optim` (fit_optim(...)) over the rows of params / grad / m / v that list_ (int32) names,
    count (int64 [1]) of them, read on the device; the rows' grad words are zeroed.  m: Adam's first moment, v: RMSProp's and
    Adam's second, float32 like params.  Asynchronous; no sync."""
    import torch
    if not (isinstance(params, torch.Tensor) and isinstance(grad, torch.Tensor) and params.dtype == torch.float32 and grad.dtype == torch.int64
            and params.is_contiguous() and grad.is_contiguous() and params.shape == grad.shape and params.device == grad.device
            and params.dim() >= 1):
        raise RtoError(-1, "params (float32) and grad (int64) must be contiguous tensors of one shape and device")
    for t, what in ((m, "m"), (v, "v")):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.shape == params.shape
                                  and t.device == params.device):
            raise RtoError(-1, "%s must be a contiguous float32 tensor like params" % what)
    if not (isinstance(list_, torch.Tensor) and list_.dtype == torch.int32 and list_.is_contiguous() and list_.device == params.device
            and isinstance(count, torch.Tensor) and count.dtype == torch.int64 and count.numel() == 1 and count.device == params.device):
        raise RtoError(-1, "list (int32) and count (int64 [1]) must be contiguous tensors on the device of params")
    row = int(params.shape[-1])
    if stream is None:
        stream = torch.cuda.current_stream(params.device)
    ptr = lambda t: None if t is None or not t.numel() else C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().rto_fit_step_sparse(ptr(params), ptr(grad), ptr(m), ptr(v), params.numel() // row, row, ptr(list_), ptr(count), list_.numel(),
                                    C.byref(optim), _stream_ptr(stream)))
    return params


def sgd_step(params, grad, lr, stream=None):
    """rto_fit_sgd_step: params -= lr * grad (fixed point -> float), grad = 0; torch tensors of one device and one shape"""
    import torch
    if not (isinstance(params, torch.Tensor) and isinstance(grad, torch.Tensor) and params.dtype == torch.float32 and grad.dtype == torch.int64
            and params.is_contiguous() and grad.is_contiguous() and params.shape == grad.shape and params.device == grad.device):
        raise RtoError(-1, "params (float32) and grad (int64) must be contiguous tensors of one shape and device")
    if stream is None:
        stream = torch.cuda.current_stream(params.device)
    check(lib().rto_fit_sgd_step(C.c_void_p(params.data_ptr()), C.c_void_p(grad.data_ptr()), params.numel(), float(lr), _stream_ptr(stream)))
    return params


def fit_grad_host(child, data, params, scale, offset, data_format, cams, targets=None, options=None, ndc=None, threads=0, grad=None,
                  stats=None, images=None):
    """rto_fit_grad_host: the same from numpy arrays (child int32 [capacity,N,N,N], data float16 -- the support --, params
    float32 [capacity,N,N,N,D], targets / images float32 [H,W,3] per camera, grad int64 like params or None, stats int64 [2] or
    None); no device is touched.  threads <= 0: one thread; the result does not depend on it."""
    child = np.ascontiguousarray(child)
    data = np.ascontiguousarray(data)
    if data.dtype == np.float16:
        data = data.view(np.uint16)
    if child.dtype != np.int32 or data.dtype != np.uint16:
        raise RtoError(-1, "child must be int32 and data float16")
    if child.ndim != 4 or data.ndim != 5 or data.shape[:4] != child.shape or not (child.shape[1] == child.shape[2] == child.shape[3]):
        raise RtoError(-1, "child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s" % (list(child.shape), list(data.shape)))

    def on_host(a, dtype, shp=None):
        return isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and (shp is None or a.shape == shp)

    if not on_host(params, np.float32, data.shape):
        raise RtoError(-1, "params must be a contiguous float32 array of shape %s" % (list(data.shape),))
    if grad is not None and not (on_host(grad, np.int64, data.shape) and grad.flags.writeable):
        raise RtoError(-1, "grad must be a contiguous int64 array of shape %s" % (list(data.shape),))
    if stats is not None and not on_host(stats, np.int64, (2,)):
        raise RtoError(-1, "stats must be a contiguous int64 array of shape [2]")
    sc = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(scale, np.float32), (3,))])
    of = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(offset, np.float32), (3,))])
    nd = None if ndc is None else (C.c_float * 3)(*[float(x) for x in ndc])
    cams = _cam_list(cams)
    arr, n = _cam_array(cams)
    ok = lambda a: on_host(a, np.float32)  # noqa: E731
    tg = _planes(cams, targets, n, "target", ok, lambda a: a.ctypes.data, False)
    im = _planes(cams, images, n, "image", lambda a: ok(a) and a.flags.writeable, lambda a: a.ctypes.data, True)
    co = _options(options)
    check(lib().rto_fit_grad_host(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), C.c_void_p(params.ctypes.data), child.shape[0],
                                  child.shape[1], data.shape[4], str(data_format).encode(), sc, of, nd, arr, tg, im, n, C.byref(co),
                                  int(threads), C.c_void_p(grad.ctypes.data) if grad is not None else None,
                                  C.c_void_p(stats.ctypes.data) if stats is not None else None))
    return grad


def _host_rays(a, name, n, written=False):
    """a contiguous float32 numpy array [n, 3]: volrend._ray_tensor's rules on the host"""
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array" % name)
    if a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != (n, 3) or (written and not a.flags.writeable):
        raise RtoError(-1, "%s must be a contiguous float32 array of shape %s" % (name, [n, 3]))
    return a


def fit_grad_rays_host(child, data, params, scale, offset, data_format, origins, dirs, targets=None, options=None, ndc=None, threads=0,
                       grad=None, stats=None, out=None, touched=None):
    """rto_fit_grad_rays_host: fit_grad_rays from numpy arrays (the tree's as fit_grad_host takes them; origins, dirs, targets, out
    float32 [n,3]); no device is touched.  threads <= 0: one thread; the result does not depend on it.  touched: None, or the
    bitmap, uint32 [touched_words(slots)]: the call goes through rto_fit_grad_rays_touched_host."""
    child = np.ascontiguousarray(child)
    data = np.ascontiguousarray(data)
    if data.dtype == np.float16:
        data = data.view(np.uint16)
    if child.dtype != np.int32 or data.dtype != np.uint16:
        raise RtoError(-1, "child must be int32 and data float16")
    if child.ndim != 4 or data.ndim != 5 or data.shape[:4] != child.shape or not (child.shape[1] == child.shape[2] == child.shape[3]):
        raise RtoError(-1, "child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s" % (list(child.shape), list(data.shape)))

    def on_host(a, dtype, shp):
        return isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.shape == shp

    if not on_host(params, np.float32, data.shape):
        raise RtoError(-1, "params must be a contiguous float32 array of shape %s" % (list(data.shape),))
    if grad is not None and not (on_host(grad, np.int64, data.shape) and grad.flags.writeable):
        raise RtoError(-1, "grad must be a contiguous int64 array of shape %s" % (list(data.shape),))
    if stats is not None and not on_host(stats, np.int64, (2,)):
        raise RtoError(-1, "stats must be a contiguous int64 array of shape [2]")
    n = int(np.shape(origins)[0]) if np.ndim(origins) else 0
    o = _host_rays(origins, "origins", n)
    d = _host_rays(dirs, "dirs", n)
    tg = None if targets is None else _host_rays(targets, "targets", n)
    ou = None if out is None else _host_rays(out, "out", n, written=True)
    sc = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(scale, np.float32), (3,))])
    of = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(offset, np.float32), (3,))])
    nd = None if ndc is None else (C.c_float * 3)(*[float(x) for x in ndc])
    co = _options(options)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if touched is not None:
        words = touched_words(child.size)
        if not (on_host(touched, np.uint32, (words,)) and touched.flags.writeable):
            raise RtoError(-1, "touched must be a contiguous uint32 array of shape [%d]" % words)
        check(lib().rto_fit_grad_rays_touched_host(ptr(child), ptr(data), ptr(params), child.shape[0], child.shape[1], data.shape[4],
                                                   str(data_format).encode(), sc, of, nd, ptr(o), ptr(d), ptr(tg), ptr(ou), n, C.byref(co),
                                                   int(threads), ptr(grad), ptr(stats), ptr(touched)))
        return grad
    check(lib().rto_fit_grad_rays_host(ptr(child), ptr(data), ptr(params), child.shape[0], child.shape[1], data.shape[4],
                                       str(data_format).encode(), sc, of, nd, ptr(o), ptr(d), ptr(tg), ptr(ou), n, C.byref(co), int(threads),
                                       ptr(grad), ptr(stats)))
    return grad


def sgd_step_host(params, grad, lr):
    """rto_fit_sgd_step_host on numpy arrays (float32 / int64, one shape)"""
    if not (isinstance(params, np.ndarray) and isinstance(grad, np.ndarray) and params.dtype == np.float32 and grad.dtype == np.int64
            and params.flags.c_contiguous and grad.flags.c_contiguous and params.shape == grad.shape):
        raise RtoError(-1, "params (float32) and grad (int64) must be contiguous arrays of one shape")
    check(lib().rto_fit_sgd_step_host(C.c_void_p(params.ctypes.data), C.c_void_p(grad.ctypes.data), params.size, float(lr)))
    return params


def touched_list_host(touched, slots, list_, count, clear=True):
    """rto_fit_touched_list_host on numpy arrays: touched uint32 [touched_words(slots)], list_ uint32, count uint64 [1]"""
    for a, dt, what in ((touched, np.uint32, "touched"), (list_, np.uint32, "list"), (count, np.uint64, "count")):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.flags.writeable):
            raise RtoError(-1, "%s must be a contiguous writable %s array" % (what, np.dtype(dt).name))
    if touched.size != touched_words(slots) or count.size != 1:
        raise RtoError(-1, "touched must hold %d words and count one" % touched_words(slots))
    keep = np.zeros(1, np.uint32)  # (an empty array has no address to pass)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib().rto_fit_touched_list_host(ptr(touched if touched.size else keep), int(slots), int(bool(clear)),
                                          ptr(list_) if list_.size else None, list_.size, ptr(count)))
    return list_


def step_sparse_host(params, grad, list_, count, optim, m=None, v=None):
    """rto_fit_step_sparse_host on numpy arrays (params / m / v float32, grad int64, one shape; list_ uint32; count uint64 [1])"""
    if not (isinstance(params, np.ndarray) and isinstance(grad, np.ndarray) and params.dtype == np.float32 and grad.dtype == np.int64
            and params.flags.c_contiguous and grad.flags.c_contiguous and params.shape == grad.shape and params.ndim >= 1):
        raise RtoError(-1, "params (float32) and grad (int64) must be contiguous arrays of one shape")
    for a, what in ((m, "m"), (v, "v")):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.shape == params.shape):
            raise RtoError(-1, "%s must be a contiguous float32 array like params" % what)
    if not (isinstance(list_, np.ndarray) and list_.dtype == np.uint32 and list_.flags.c_contiguous and isinstance(count, np.ndarray)
            and count.dtype == np.uint64 and count.size == 1):
        raise RtoError(-1, "list (uint32) and count (uint64 [1]) must be contiguous arrays")
    row = int(params.shape[-1])
    ptr = lambda a: None if a is None or not a.size else C.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib().rto_fit_step_sparse_host(ptr(params), ptr(grad), ptr(m), ptr(v), params.size // row, row, ptr(list_), ptr(count), list_.size,
                                         C.byref(optim)))
    return params


def _loss_of(words):
    """(sum of the rays' squared errors, rays) from the two stats words"""
    return float(int(words[0])) / FIX_SCALE, int(words[1])


class TreeFit:
    """The state of a fit on the device: the N3Tree (topology and support), params (float32, made from the float16 `data` the tree
    was uploaded from), grad and stats.  accumulate() adds a batch's gradient and loss, step() takes the SGD step and clears the
    gradient, loss() reads and clears the loss (it synchronises), render() is the deterministic render of params.

    optimizer "sgd" (the default), "rmsprop" or "adam"; sparse: step only the leaves the batches since the last step reached (the
    touched bitmap, its list, rto_fit_step_sparse); an optimiser other than "sgd" implies it.  Under sparse, accumulate_rays marks,
    and accumulate(cams, targets) goes through volrend.camera_rays and the ray entry: by the identity of include/rto.h that gives
    the camera entry's bytes.  step(lr, grad_scale) lists with clear, steps, and advances t; the moments of a leaf no batch
    reached do not decay.  The bitmap, the list (one entry per slot), the scratch and m / v are allocated once, here.  With the
    defaults nothing changes: the same calls, the same bytes.  A new TreeFit starts with zero moments and t = 0, so
    refine_fit, which builds one per round, restarts the optimiser's state at every refinement."""

    def __init__(self, tree, data, options=None, optimizer="sgd", sparse=False, beta1=0.9, beta2=0.999, eps=1e-8):
        import torch
        self.tree = tree
        self.options = options
        device = torch.device("cuda", tree.device)
        data = np.ascontiguousarray(data)
        shape = (int(tree.capacity), int(tree.N), int(tree.N), int(tree.N), int(tree.data_dim))
        if data.dtype != np.float16 or data.shape != shape:
            raise RtoError(-1, "data must be the float16 array %s the tree was uploaded from" % (list(shape),))
        self.params = torch.from_numpy(data.astype(np.float32)).to(device)
        self.grad = torch.zeros(shape, dtype=torch.int64, device=device)
        self.stats = torch.zeros(2, dtype=torch.int64, device=device)
        if optimizer not in KINDS:
            raise RtoError(-1, "optimizer must be one of %s, not %r" % (sorted(KINDS), optimizer))
        self.optimizer, self.sparse, self.t = optimizer, bool(sparse) or optimizer != "sgd", 0
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.touched = self.m = self.v = None
        if self.sparse:
            self.slots = shape[0] * shape[1] ** 3
            self.touched = torch.zeros(touched_words(self.slots), dtype=torch.int32, device=device)
            self.list = torch.empty(self.slots, dtype=torch.int32, device=device)
            self.count = torch.zeros(1, dtype=torch.int64, device=device)
            self.scratch = torch.empty(touched_scratch_bytes(self.slots), dtype=torch.uint8, device=device)
            if optimizer == "adam":
                self.m = torch.zeros(shape, dtype=torch.float32, device=device)
            if optimizer != "sgd":
                self.v = torch.zeros(shape, dtype=torch.float32, device=device)

    def accumulate(self, cams, targets, stream=None):
        if self.sparse:
            from .volrend import camera_rays
            for c, tg in zip(_cam_list(cams), list(targets)):
                o, d = camera_rays(c)
                self.accumulate_rays(o, d, tg.reshape(-1, 3), stream=stream)
            return
        fit_grad(self.tree, self.params, cams, targets, self.options, grad=self.grad, stats=self.stats, stream=stream)

    def step(self, lr, grad_scale=1.0, stream=None):
        if not self.sparse:
            if grad_scale != 1.0:
                raise RtoError(-1, "the dense step takes no grad_scale: fold it into lr, or make the fit sparse")
            sgd_step(self.params, self.grad, lr, stream=stream)
            return
        self.t += 1
        o = fit_optim(self.optimizer, lr, grad_scale, self.beta1, self.beta2, self.eps, self.t)
        touched_list(self.touched, self.slots, self.list, self.count, self.scratch, clear=True, stream=stream)
        step_sparse(self.params, self.grad, self.list, self.count, o, m=self.m, v=self.v, stream=stream)

    def evaluate(self, cams, targets, stream=None):
        """(loss, rays) of params over a set of views: forward only, through stats (which it clears)"""
        fit_grad(self.tree, self.params, cams, targets, self.options, stats=self.stats, stream=stream)
        return self.loss()

    def loss(self, reset=True):
        """(sum over the rays since the last reset of |out - target|^2, their number)"""
        words = self.stats.cpu().numpy()
        if reset:
            self.stats.zero_()
        return _loss_of(words)

    def render(self, cams, stream=None):
        """the composited images of params: a list of float32 [H,W,3] tensors"""
        import torch
        cams = _cam_list(cams)
        images = [torch.empty((int(c.height), int(c.width), 3), dtype=torch.float32, device=self.params.device) for c in cams]
        fit_grad(self.tree, self.params, cams, None, self.options, images=images, stream=stream)
        return images

    def accumulate_rays(self, origins, dirs, targets, stream=None):
        """accumulate() on rays of the caller's (fit_grad_rays): [n,3] tensors on the device, or numpy arrays"""
        fit_grad_rays(self.tree, self.params, origins, dirs, targets, self.options, grad=self.grad, stats=self.stats, stream=stream,
                      touched=self.touched)

    def evaluate_rays(self, origins, dirs, targets, stream=None):
        """(loss, rays) of params over the rays: forward only, through stats (which it clears)"""
        fit_grad_rays(self.tree, self.params, origins, dirs, targets, self.options, stats=self.stats, stream=stream)
        return self.loss()

    def render_rays(self, origins, dirs, stream=None):
        """the composited colours of params along the rays: a float32 [n,3] tensor"""
        import torch
        out = torch.empty((int(origins.shape[0]), 3), dtype=torch.float32, device=self.params.device)
        fit_grad_rays(self.tree, self.params, origins, dirs, None, self.options, out=out, stream=stream)
        return out

    def data_half(self):
        """params rounded to float16 (to nearest even) as a numpy array: what a tree file stores"""
        return self.params.cpu().numpy().astype(np.float16)


class HostTreeFit:
    """TreeFit on the host twin (no device): the same methods, the same bytes.  targets are numpy arrays."""

    def __init__(self, child, data, scale, offset, data_format, options=None, ndc=None, threads=0, optimizer="sgd", sparse=False, beta1=0.9,
                 beta2=0.999, eps=1e-8):
        self.child = np.ascontiguousarray(child)
        self.data = np.ascontiguousarray(data)
        if self.data.dtype != np.float16:
            raise RtoError(-1, "data must be float16")
        self.scale, self.offset, self.data_format, self.options, self.ndc, self.threads = scale, offset, data_format, options, ndc, threads
        self.params = self.data.astype(np.float32)
        self.grad = np.zeros(self.data.shape, np.int64)
        self.stats = np.zeros(2, np.int64)
        if optimizer not in KINDS:
            raise RtoError(-1, "optimizer must be one of %s, not %r" % (sorted(KINDS), optimizer))
        self.optimizer, self.sparse, self.t = optimizer, bool(sparse) or optimizer != "sgd", 0
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.touched = self.m = self.v = None
        if self.sparse:
            self.slots = self.child.size
            self.touched = np.zeros(touched_words(self.slots), np.uint32)
            self.list = np.zeros(self.slots, np.uint32)
            self.count = np.zeros(1, np.uint64)
            if optimizer == "adam":
                self.m = np.zeros(self.data.shape, np.float32)
            if optimizer != "sgd":
                self.v = np.zeros(self.data.shape, np.float32)

    def _call(self, cams, targets, **kw):
        fit_grad_host(self.child, self.data, self.params, self.scale, self.offset, self.data_format, cams, targets, self.options, ndc=self.ndc,
                      threads=self.threads, **kw)

    def accumulate(self, cams, targets):
        if self.sparse:
            from .volrend import camera_rays
            for c, tg in zip(_cam_list(cams), list(targets)):
                o, d = camera_rays(c)
                self.accumulate_rays(o, d, np.ascontiguousarray(tg).reshape(-1, 3))
            return
        self._call(cams, targets, grad=self.grad, stats=self.stats)

    def step(self, lr, grad_scale=1.0):
        if not self.sparse:
            if grad_scale != 1.0:
                raise RtoError(-1, "the dense step takes no grad_scale: fold it into lr, or make the fit sparse")
            sgd_step_host(self.params, self.grad, lr)
            return
        self.t += 1
        o = fit_optim(self.optimizer, lr, grad_scale, self.beta1, self.beta2, self.eps, self.t)
        touched_list_host(self.touched, self.slots, self.list, self.count, clear=True)
        step_sparse_host(self.params, self.grad, self.list, self.count, o, m=self.m, v=self.v)

    def evaluate(self, cams, targets):
        self._call(cams, targets, stats=self.stats)
        return self.loss()

    def loss(self, reset=True):
        words = self.stats.copy()
        if reset:
            self.stats[:] = 0
        return _loss_of(words)

    def render(self, cams):
        cams = _cam_list(cams)
        images = [np.empty((int(c.height), int(c.width), 3), np.float32) for c in cams]
        self._call(cams, None, images=images)
        return images

    def _call_rays(self, origins, dirs, targets, **kw):
        fit_grad_rays_host(self.child, self.data, self.params, self.scale, self.offset, self.data_format, origins, dirs, targets, self.options,
                           ndc=self.ndc, threads=self.threads, **kw)

    def accumulate_rays(self, origins, dirs, targets):
        self._call_rays(origins, dirs, targets, grad=self.grad, stats=self.stats, touched=self.touched)

    def evaluate_rays(self, origins, dirs, targets):
        self._call_rays(origins, dirs, targets, stats=self.stats)
        return self.loss()

    def render_rays(self, origins, dirs):
        out = np.empty((int(origins.shape[0]), 3), np.float32)
        self._call_rays(origins, dirs, None, out=out)
        return out

    def data_half(self):
        return self.params.astype(np.float16)
