"""The median-cut quantiser (include/rto.h "quantiser"; csrc/quantize_kernels.hip, csrc/host/median_cut.cpp): m rows of three
fp16 values -> a palette of 2^bits colours and the palette index of every row, the same bits from the HIP kernels and from the
host twin.  A tool path (compress_octree.py), not a frame path: the device call returns after its stream has drained."""
import ctypes as C

import numpy as np

from ._lib import RtoError, check, lib
from .volrend import _stream_ptr


class Quantizer:
    """rto_quantizer: owns the scratch of the device entry (about 24 bytes per row), which grows on demand and is reused
    across calls.  One instance serves one stream at a time."""

    def __init__(self, device=0):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_quantizer_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def median_cut(self, rows, bits=16, stream=None):
        """rows: a contiguous torch half tensor [m, 3] on this device -> (palette half [2^bits, 3], ids [m] int16 tensor holding
        the uint16 patterns), device tensors.  Synchronises the stream."""
        import torch
        if not (hasattr(rows, "data_ptr") and rows.is_cuda and rows.dtype == torch.float16 and rows.dim() == 2
                and rows.shape[1] == 3 and rows.is_contiguous()):
            raise RtoError(-1, "rows must be a contiguous float16 device tensor [m, 3]")
        if not 1 <= int(bits) <= 16:
            raise RtoError(-1, "bits must be in 1 .. 16, not %d" % bits)
        m = int(rows.shape[0])
        palette = torch.empty((1 << int(bits), 3), dtype=torch.float16, device=rows.device)
        ids = torch.empty((max(m, 1),), dtype=torch.int16, device=rows.device)
        check(lib().rto_quantize_median_cut(self._h, _stream_ptr(stream), C.c_void_p(rows.data_ptr()), m, int(bits),
                                            C.c_void_p(palette.data_ptr()), C.c_void_p(ids.data_ptr())))
        return palette, ids[:m]

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_quantizer_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def quantize_median_cut_host(rows, bits=16):
    """The host twin on a numpy float16 [m, 3] array: no device is touched."""
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.float16 or rows.ndim != 2 or rows.shape[1] != 3:
        raise RtoError(-1, "rows must be a float16 array [m, 3]")
    if not 1 <= int(bits) <= 16:
        raise RtoError(-1, "bits must be in 1 .. 16, not %d" % bits)
    m = rows.shape[0]
    palette = np.zeros((1 << int(bits), 3), np.float16)
    ids = np.zeros((max(m, 1),), np.uint16)
    check(lib().rto_quantize_median_cut_host(C.c_void_p(rows.ctypes.data), m, int(bits), C.c_void_p(palette.ctypes.data),
                                             C.c_void_p(ids.ctypes.data)))
    return palette, ids[:m]


def quantize_median_cut(rows, bits=16, backend="hip", quantizer=None, stream=None):
    """(palette float16 [2^bits, 3], ids uint16 [m]) as numpy arrays.  rows: a numpy float16 [m, 3] array or a torch half tensor.
    backend "hip": the kernels (device memory is torch tensors; `quantizer`: a Quantizer to reuse, else one is made for the
    call); "cpu": the host twin, which never touches a GPU."""
    if backend == "cpu":
        if hasattr(rows, "data_ptr"):
            rows = rows.detach().cpu().numpy()
        return quantize_median_cut_host(rows, bits)
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    import torch
    if not hasattr(rows, "data_ptr"):
        rows = np.ascontiguousarray(rows)
        if rows.dtype != np.float16:
            raise RtoError(-1, "rows must be float16")
        rows = torch.from_numpy(rows)
    if not rows.is_cuda:
        rows = rows.to("cuda:%d" % (quantizer.device if quantizer is not None else 0))
    rows = rows.contiguous()
    q = quantizer if quantizer is not None else Quantizer(rows.device.index or 0)
    try:
        palette, ids = q.median_cut(rows, bits, stream)
        return palette.cpu().numpy(), ids.cpu().numpy().view(np.uint16)
    finally:
        if quantizer is None:
            q.free()
