"""What the models of the layer passes (grid_ref, mesh_ref; DESIGN.md section 7f "Layer pass") share: the pixel's ray, the merge,
the cases' camera, the calls every pass refuses.  A numpy restatement: nothing here is taken from the package under test."""
import copy
import ctypes as C

import numpy as np

f32 = np.float32


def pixel_dirs(W, H, fx, fy, m):
    """M xyz of every pixel [H * W, 3]: the ray of ray_setup before it normalises (float32, left to right) for the 12-float transform m"""
    m = np.asarray(m, f32).reshape(-1)
    x = np.broadcast_to(np.arange(W, dtype=np.int64).astype(f32)[None, :], (H, W)).reshape(-1)
    y = np.broadcast_to(np.arange(H, dtype=np.int64).astype(f32)[:, None], (H, W)).reshape(-1)
    xyz0 = (x - f32(0.5) * f32(W)) / f32(fx)
    xyz1 = -(y - f32(0.5) * f32(H)) / f32(fy)
    xyz2 = f32(-1.0)
    return np.stack([(m[c] * xyz0 + m[3 + c] * xyz1) + m[6 + c] * xyz2 for c in range(3)], 1).astype(f32)


def unit_dirs(W, H, fx, fy, m):
    """ray_setup's unit world directions [H * W, 3]"""
    dw = pixel_dirs(W, H, fx, fy, m)
    inv = f32(1) / np.sqrt((dw[:, 0] * dw[:, 0] + dw[:, 1] * dw[:, 1]) + dw[:, 2] * dw[:, 2])
    return dw * inv[:, None]


def merge_layers(depth, col, old_depth, old_col):
    """RTO_GRID_MERGE / RTO_MESH_MERGE: the GL depth test of (depth, col) against what the buffers hold.  A hit replaces both
    where the existing depth is greater than its own; a NaN or <= 0 existing depth never is (a hit's depth is > 0)."""
    with np.errstate(invalid="ignore"):
        take = np.isfinite(depth) & (old_depth > depth)
    return np.where(take, depth, old_depth), np.where(take[..., None], col, old_col)


class Cam:
    """(the models take anything with width, height, fx, fy, transform; c2w is for the float64 geometries)"""
    def __init__(self, W, H, pose, fx):
        self.width, self.height = W, H
        self.fx = self.fy = float(fx)
        self.c2w = np.asarray(pose, np.float64)[:3, :4]
        self.transform = np.ascontiguousarray(np.asarray(pose, f32)[:3, :4].T).reshape(-1)


def invalid_layer_calls(raw, params, h, cam, depth, color):
    """the RTO_E_INVALID calls common to every layer pass as (what, thunk -> rc).  raw(h, cams, n, p, depth, color) -> rc: the
    pass's C entry point; params(**kw): its C params; h: a handle, real or fake; cam: a camera of the package's"""
    other, zero_f = copy.copy(cam), copy.copy(cam)
    other.width = cam.width + 8
    zero_f.fx = 0.0
    bad_flag, merge, ok = params(), params(), params()
    bad_flag.flags, merge.flags = 2, 1
    nan = float("nan")
    return [
        ("null handle", lambda: raw(None, [cam], 1, ok, depth, color)),
        ("null cams", lambda: raw(h, None, 1, ok, depth, color)),
        ("null params", lambda: raw(h, [cam], 1, None, depth, color)),
        ("both outputs null", lambda: raw(h, [cam], 1, ok, None, None)),
        ("n < 0", lambda: raw(h, [cam], -1, ok, depth, color)),
        ("line_px 0", lambda: raw(h, [cam], 1, params(line_px=0.0), depth, color)),
        ("line_px nan", lambda: raw(h, [cam], 1, params(line_px=nan), depth, color)),
        ("unknown flag", lambda: raw(h, [cam], 1, bad_flag, depth, color)),
        ("merge without depth", lambda: raw(h, [cam], 1, merge, None, color)),
        ("colour misaligned", lambda: raw(h, [cam], 1, ok, depth, C.c_void_p(C.cast(color, C.c_void_p).value + 8))),
        ("cameras of differing size", lambda: raw(h, [cam, other], 2, ok, depth, color)),
        ("fx 0", lambda: raw(h, [zero_f], 1, ok, depth, color)),
    ]
