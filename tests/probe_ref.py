"""The operator's probe (volrend.cu:100-134, 215-231) restated in numpy float32, operation by operation: which pixels lie in
the lumisphere's disc and what colour each has.  The leaf's coefficients come from the host arrays through the oracle's
orc_query, the SH basis from orc_sh_basis, the SG / ASG basis from tests/sg_asg_ref.py, the exponential from orc_det_expf.
One deviation from the reference, as the library documents it: the sum over basis functions runs over
max(lo, 0) .. min(hi, basis_dim - 1) rather than basis_minmax[0] .. basis_minmax[1] whatever the tree's basis_dim."""
import ctypes as C

import numpy as np

import orc
import sg_asg_ref

f32 = np.float32


def disc(W, H, disp):
    """-> (mask [H, W] bool, cen0 [H, W] f32, cen1 [H, W] f32, c [H, W] f32) for probe_disp_size = disp"""
    x = np.arange(W, dtype=np.int64)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=np.int64)[:, None].repeat(W, 1)
    inside = (y < disp + 5) & (x >= W - disp - 5)
    xx = (x - (W - disp) + 5).astype(f32)
    yy = (y - 5).astype(f32)
    half = f32(0.5) * f32(disp)
    cen0 = -(xx / half - f32(1.0))
    cen1 = yy / half - f32(1.0)
    c = cen0 * cen0 + cen1 * cen1
    return inside & (c <= f32(1.0)), cen0.astype(f32), cen1.astype(f32), c.astype(f32)


def leaf_coeffs(ht, point):
    """float32 [data_dim - 1]: the coefficients of the leaf orc_query reaches from xyz = offset + scale * point"""
    p = np.asarray(point, f32)
    xyz = (ht.offset + ht.scale * p).astype(f32)
    buf = (C.c_float * 3)(*[float(v) for v in xyz])
    cube, lv = C.c_float(), C.c_int()
    slot = orc.lib().orc_query(C.byref(ht.c), buf, C.byref(cube), C.byref(lv))
    dd = ht.data_dim
    row = ht.data.reshape(-1)[slot * dd: slot * dd + dd - 1]
    return np.array([orc.lib().orc_half2float(int(h)) for h in row], f32)


def _sh_basis(basis_dim, dirs):
    out = np.zeros((dirs.shape[0], 25), f32)
    fn = orc.lib().orc_sh_basis
    b = (C.c_float * 25)()
    for i, d in enumerate(dirs):
        for k in range(25):
            b[k] = 0.0
        fn(C.c_int(basis_dim), (C.c_float * 3)(float(d[0]), float(d[1]), float(d[2])), b)
        out[i] = np.frombuffer(b, f32)
    return out


def colours(ht, point, transform12, W, H, disp, basis_minmax=(0, 24), lobes=None):
    """-> (mask [H, W], rgb [n, 3] f32 for the mask's pixels in row-major order)"""
    mask, cen0, cen1, c = disc(W, H, disp)
    coeff = leaf_coeffs(ht, point)
    n = int(mask.sum())
    if ht.basis_dim < 0:  # RGBA: the first three coefficients as they are
        return mask, np.broadcast_to(coeff[:3], (n, 3)).copy()
    c0, c1 = cen0[mask], cen1[mask]
    c2 = -np.sqrt(f32(1.0) - c[mask])
    m = np.asarray(transform12, f32).reshape(-1)
    dirs = np.stack([(m[0] * c0 + m[3] * c1) + m[6] * c2, (m[1] * c0 + m[4] * c1) + m[7] * c2,
                     (m[2] * c0 + m[5] * c1) + m[8] * c2], 1).astype(f32)
    B = ht.basis_dim
    if ht.format == 1:
        basis = _sh_basis(B, dirs)
    else:
        basis = sg_asg_ref.basis({2: "SG", 3: "ASG"}[ht.format], lobes, dirs)
    lo, hi = max(int(basis_minmax[0]), 0), min(int(basis_minmax[1]), B - 1)
    expf = orc.lib().orc_det_expf
    rgb = np.empty((n, 3), f32)
    with np.errstate(over="ignore", under="ignore"):
        for t in range(3):
            tmp = np.zeros(n, f32)
            for i in range(lo, hi + 1):
                tmp = tmp + basis[:, i] * coeff[t * B + i]
            e = np.array([expf(float(-v)) for v in tmp], f32)
            rgb[:, t] = f32(1.0) / (f32(1.0) + e)
    return mask, rgb


def outputs(rgb):
    """what a disc pixel holds (volrend.cu:174-212, nalpha = 0): aux [n, 8] and the image's [n, 4]"""
    one = np.ones((rgb.shape[0], 1), f32)
    v = np.concatenate([rgb, one], 1)
    return np.concatenate([v, v * v], 1).astype(f32), v
