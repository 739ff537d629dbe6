"""An independent restatement, in numpy float32 operation by operation, of what the renderer computes for SG / ASG
PlenOctrees (lumisphere.hpp:14-37): the view direction of a pixel (screen2worlddir + v_normalize + the rot_dirs
rotation, as oracle/rto_oracle.c:505-547 states them), the lobe basis, the library's deterministic expf and the shading
of one hit leaf (rt_core.cuh:277-325).  Every float32 product and sum is rounded on its own (numpy does not contract)."""
import ctypes as C
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
LOBE_FLOATS = {"SG": 4, "ASG": 11}
BASIS_MAX = 25

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = C.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]


def det_expf(x):
    """The library's expf (rto_device_math.h det_expf = oracle orc_det_expf) in float64 numpy: Cody-Waite reduction,
    degree-11 polynomial, scale by 2^k, one rounding to float32 -- subnormal and zero results included."""
    x = np.asarray(x, f32)
    xd = np.where(np.isfinite(x), x, 0).astype(f64)  # (non-finite arguments take the special cases below)
    z = xd * 1.4426950408889634
    kd = (z + 6755399441055744.0) - 6755399441055744.0
    r = (xd - kd * 0.693147180558298016) - kd * 1.6465949582897082e-12
    p = np.full_like(r, 1.0 / 39916800.0)
    for c in (1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0,
              1.0 / 6.0, 0.5, 1.0, 1.0):
        p = p * r + c
    k = kd.astype(np.int64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = (p * np.ldexp(1.0, k)).astype(f32)
    out = np.where(x > f32(88.72283935546875), f32(np.inf), out)
    out = np.where(x < f32(-103.97208404541016), f32(0.0), out)
    return np.where(np.isnan(x), x, out).astype(f32)


def dot3(d, m):
    """_dot3 (common.cuh:47-51): d0*m0 + d1*m1 + d2*m2, left to right; d [n,3], m [3] -> [n]"""
    m = np.asarray(m, f32)
    return (d[:, 0] * m[0] + d[:, 1] * m[1]) + d[:, 2] * m[2]


def lobe_basis(kind, lobes, d):
    """[n, B] basis of the rotated view directions d [n,3] float32 (maybe_precalc_basis, SG / ASG branch)."""
    lobes = np.asarray(lobes, f32).reshape(-1, LOBE_FLOATS[kind])
    B = lobes.shape[0]
    fB = f32(B)
    out = np.zeros((d.shape[0], B), f32)
    with np.errstate(over="ignore", under="ignore"):
        for i, p in enumerate(lobes):
            if kind == "SG":
                out[:, i] = det_expf(p[0] * (dot3(d, p[1:4]) - f32(1.0))) / fB
            else:
                S, dx, dy = dot3(d, p[8:11]), dot3(d, p[2:5]), dot3(d, p[5:8])
                out[:, i] = S * det_expf(-p[0] * dx * dx - p[1] * dy * dy) / fB
    return out


def rotate(vdir, rot_dirs):
    """rodrigues(opt.rot_dirs, vdir) (volrend.cu:58-73): float terms, the last one times the double (1.0 - cos)."""
    a = np.asarray(rot_dirs, f32)
    angle = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    if float(angle) < 1e-6:
        return vdir
    k = a / angle
    c, s = f32(_libm.cosf(float(angle))), f32(_libm.sinf(float(angle)))
    v0, v1, v2 = vdir[:, 0], vdir[:, 1], vdir[:, 2]
    cross = [k[1] * v2 - k[2] * v1, k[2] * v0 - k[0] * v2, k[0] * v1 - k[1] * v0]
    dot = (k[0] * v0 + k[1] * v1) + k[2] * v2
    omc = 1.0 - f64(c)
    out = np.empty_like(vdir)
    for i in range(3):
        out[:, i] = ((vdir[:, i] * c + cross[i] * s).astype(f64) + (k[i] * dot).astype(f64) * omc).astype(f32)
    return out


def basis(kind, lobes, vdir, rot_dirs=(0, 0, 0), basis_minmax=(0, BASIS_MAX - 1)):
    """ray_basis: the [n, 25] basis the kernels evaluate for unrotated view directions vdir [n,3]."""
    vdir = np.asarray(vdir, f32)
    b = lobe_basis(kind, lobes, rotate(vdir, rot_dirs))
    out = np.zeros((vdir.shape[0], BASIS_MAX), f32)
    out[:, : b.shape[1]] = b
    idx = np.arange(BASIS_MAX)
    out[:, (idx < basis_minmax[0]) | (idx > basis_minmax[1])] = 0
    return out


def pixel_vdir(W, H, fx, fy, transform12, xs, ys):
    """screen2worlddir (volrend.cu:23-34) + v_normalize for pixels (xs, ys): [n,3] float32"""
    m = np.asarray(transform12, f32).reshape(-1)
    x = np.asarray(xs).astype(f32)
    y = np.asarray(ys).astype(f32)
    X = (x - f32(0.5) * f32(W)) / f32(fx)
    Y = -(y - f32(0.5) * f32(H)) / f32(fy)
    Z = f32(-1.0)
    d = np.stack([(m[0] * X + m[3] * Y) + m[6] * Z, (m[1] * X + m[4] * Y) + m[7] * Z, (m[2] * X + m[5] * Y) + m[8] * Z], 1)
    inv = f32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (d * inv[:, None]).astype(f32)


def shade_leaf(basis_fn, coeffs, cnt=1.0):
    """rt_core.cuh:286-325 for one hit leaf per row: basis_fn [n,25], coeffs [n, 3B] (float32 from fp16) -> rgb [n,3].
    Only B in {4, 9, 16, 25} sums past the DC term (the reference's switch); the groups in its order."""
    n, D = coeffs.shape
    B = D // 3
    groups = {25: [range(16, 25), range(9, 16), range(4, 9), range(1, 4)], 16: [range(9, 16), range(4, 9), range(1, 4)],
              9: [range(4, 9), range(1, 4)], 4: [range(1, 4)]}.get(B, [])
    cnt = f32(cnt)
    rgb = np.empty((n, 3), f32)
    with np.errstate(over="ignore", under="ignore"):
        for c in range(3):
            tv = coeffs[:, c * B:(c + 1) * B].astype(f32)
            tmp = basis_fn[:, 0] * tv[:, 0]
            for g in groups:
                acc = None
                for k in g:
                    t = basis_fn[:, k] * tv[:, k]
                    acc = t if acc is None else acc + t
                tmp = tmp + acc
            rgb[:, c] = cnt / (f32(1.0) + det_expf(-tmp))
    return rgb
