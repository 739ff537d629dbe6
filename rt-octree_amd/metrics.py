"""Image metrics on the device (include/rto.h "image metrics", csrc/metrics_kernels.hip): per-frame MSE, PSNR, SMAPE and SSIM
of a predicted against a true image -- what the reference's test loop scores every frame with (denoiser/runner.py:126-160,
denoiser/metrics.py:7-9, 61-79; SSIM as pytorch_msssim.ssim(X, Y, data_range=1)) -- in float64, in a fixed summation order, and
the PNG reader that brings a dataset's ground truth in."""
import collections
import ctypes as C

import numpy as np

from ._lib import RtoError, check, lib
from .volrend import _stream_ptr

IMAGE_RGBA32F, IMAGE_RGBA8 = 0, 1  # RTO_IMAGE_*
TRUTH_OVER_BACKGROUND = 1  # RTO_METRICS_TRUTH_OVER_BACKGROUND

FrameMetrics = collections.namedtuple("FrameMetrics", ["mse", "psnr", "smape", "ssim"])


def _describe(t, name):
    """(pointer, format, (n, H, W)) of a device image: a torch tensor or anything with the CUDA array interface, float32 or
    uint8, [n,H,W,4] or [H,W,4], contiguous"""
    if hasattr(t, "data_ptr"):
        import torch
        if not t.is_cuda:
            raise RtoError(-1, "%s is not a device tensor" % name)
        if not t.is_contiguous():
            raise RtoError(-1, "%s must be contiguous" % name)
        if t.dtype == torch.float32:
            fmt = IMAGE_RGBA32F
        elif t.dtype == torch.uint8:
            fmt = IMAGE_RGBA8
        else:
            raise RtoError(-1, "%s must be float32 or uint8, not %s" % (name, t.dtype))
        ptr, shape = t.data_ptr(), tuple(int(s) for s in t.shape)
    elif hasattr(t, "__cuda_array_interface__"):
        a = t.__cuda_array_interface__
        if a.get("strides") is not None:
            raise RtoError(-1, "%s must be contiguous" % name)
        fmt = {"<f4": IMAGE_RGBA32F, "|u1": IMAGE_RGBA8}.get(a["typestr"])
        if fmt is None:
            raise RtoError(-1, "%s must be float32 or uint8, not %s" % (name, a["typestr"]))
        ptr, shape = int(a["data"][0]), tuple(int(s) for s in a["shape"])
    else:
        raise TypeError("%s: expected a device tensor" % name)
    if len(shape) == 3:
        shape = (1,) + shape
    if len(shape) != 4 or shape[3] != 4:
        raise RtoError(-1, "%s must be [n,H,W,4] or [H,W,4], not %s" % (name, list(shape)))
    return ptr, fmt, shape[:3]


class ImageMetrics:
    """rto_metrics: owns the partial-sum scratch of the metric kernels; one instance serves one stream at a time.

    compute(pred, truth) -> a list of n FrameMetrics(mse, psnr, smape, ssim), floats (synchronises the stream);
    compute_async(pred, truth, out=...) fills a float64 [n,4] device tensor without synchronising.
    pred / truth: device tensors, float32 or uint8 (value / 255 in float32), [n,H,W,4] or [H,W,4]; only r, g, b are measured.
    over_background = b: the true image's rgb becomes rgb * a + b * (1 - a) first, in float32 (denoiser/dataset.py:82-84)."""

    def __init__(self, device=0):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_metrics_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def _args(self, pred, truth, over_background):
        pp, pf, ps = _describe(pred, "pred")
        tp, tf, ts = _describe(truth, "truth")
        if ps != ts:
            raise RtoError(-1, "pred is %s and truth is %s" % (list(ps), list(ts)))
        flags, bg = (0, 0.0) if over_background is None else (TRUTH_OVER_BACKGROUND, float(over_background))
        n, H, W = ps
        return C.c_void_p(pp), pf, C.c_void_p(tp), tf, n, H, W, flags, C.c_float(bg)

    def compute(self, pred, truth, over_background=None, stream=None):
        a = self._args(pred, truth, over_background)
        out = np.empty((a[4], 4), np.float64)
        check(lib().rto_metrics_compute(self._h, _stream_ptr(stream), *a, C.c_void_p(out.ctypes.data)))
        return [FrameMetrics(*(float(v) for v in row)) for row in out]

    def compute_async(self, pred, truth, over_background=None, stream=None, out=None):
        import torch
        a = self._args(pred, truth, over_background)
        if out is None:
            out = torch.empty((a[4], 4), dtype=torch.float64, device="cuda:%d" % self.device)
        if out.dtype != torch.float64 or tuple(out.shape) != (a[4], 4) or not out.is_contiguous() or not out.is_cuda:
            raise RtoError(-1, "out must be a contiguous float64 device tensor [%d,4]" % a[4])
        check(lib().rto_metrics_compute_async(self._h, _stream_ptr(stream), *a, C.c_void_p(out.data_ptr())))
        return out

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_metrics_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def read_png(path):
    """rto_image_read_png: an 8-bit RGB or RGBA, non-interlaced PNG -> uint8 [H,W,4] (alpha 255 for RGB).  Anything else raises
    RtoError with a message that names the file."""
    w, h = C.c_int(0), C.c_int(0)
    p = str(path).encode()
    check(lib().rto_image_read_png(p, C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 4), np.uint8)
    check(lib().rto_image_read_png(p, C.byref(w), C.byref(h), C.c_void_p(out.ctypes.data), out.nbytes))
    if (h.value, w.value) != out.shape[:2]:
        raise RtoError(-5, "PNG %s changed while it was read" % path)
    return out
