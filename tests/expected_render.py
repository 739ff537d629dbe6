"""An INDEPENDENT float64 statement of what the regular-tracking estimator must converge to.

Test infrastructure.  Nothing here is derived from rt_core.cuh's loop structure, from oracle/ or from
the HIP kernels; it is the volume-rendering equation for a piecewise-constant medium (a PlenOctree),
written down from the paper's model, plus the two modelling facts the reference documents:

  * a ray visits the octree leaf by leaf; after a leaf it re-starts `step_size` (tree units) beyond
    the leaf's exit point, and that extra length counts as optical depth of
    the leaf just left;
  * leaves with sigma <= sigma_thresh are empty space (appendix B 1).

For a ray crossing segments j = 1..n of length d_j (world units) with density s_j and view-dependent
colour c_j:

    tau_j  = s_j * d_j                        optical depth of segment j
    T_j    = exp(-sum_{i<j} tau_i)            transmittance in front of it
    p_j    = T_j * (1 - exp(-tau_j))          probability that a free-flight sample ends in j
    E[rgb] = sum_j p_j c_j + bg * T_{n+1}     (the estimator composites the background)
    E[a]   = 1 - T_{n+1} = 1 - exp(-tau_total)

Tracking draws free-flight distances d = -log(1 - u) (unit-rate exponential in optical depth) and
returns the colour of the segment where the accumulated optical depth first reaches d; SPP such
samples are averaged.  So one sample is the categorical variable X = c_j w.p. p_j, bg w.p. T_{n+1},
and a mean of n independent samples has variance (E[X^2] - E[X]^2) / n per channel.

The colour of a leaf: sigmoid(sum_k Y_k(view dir) * coeff[channel][k]) with Y_k the real spherical
harmonics (Condon-Shortley phase kept), evaluated here with scipy.  For SG and ASG trees Y_k is the
k-th lobe of the tree's lumisphere (lumisphere.hpp:14-37; the lobes are SynthTree.extra), d the view
direction, B the number of lobes:

    SG  lobe {lambda, mu}:                          Y_k(d) = exp(lambda (mu . d - 1)) / B
    ASG lobe {lambda_x, lambda_y, mu_x, mu_y, mu_z}: Y_k(d) = (mu_z . d) exp(-lambda_x (mu_x . d)^2 - lambda_y (mu_y . d)^2) / B

(the reference's text divides every lobe by B and does NOT clamp the ASG's smooth term mu_z . d at
zero, as the ASG literature does: a lobe facing away contributes negatively.  The reference decides.)

Three more facts about rays, each read from the reference's text and not from the oracle:

  * depth limit (`t_max`: the world distance from the origin, along the unit direction, where the ray
    ends).  rt_core.cuh:208-217 turns it into tree units and takes the smaller of it and the box exit
    as the END OF THE MARCH: `tmax = min(tmax, tmax_bg)`; the march (:241) is `while (t < tmax)` with t
    the point where the ray ENTERS the next leaf, and the leaf's whole crossing (plus step_size) is
    then added as optical depth (:249-253).  So a leaf the ray enters before the cut counts WHOLE, even
    where it reaches beyond the cut, and a leaf entered at or behind the cut does not count at all:
    the cut is never inside a segment, it removes whole segments.  The conversion uses the same
    world_per_tree factor as the segment lengths.
  * directions need not be unit vectors: the ray is its origin and the direction's line
    (volrend.cu:32 normalises), and t_max is measured along the unit direction.
  * NDC trees (LLFF scenes; volrend.cu:35-56): the ray is warped as the NeRF paper's appendix C
    states -- the origin is moved along the ray to the near plane z = -1, then with o, d the shifted
    origin and the direction, a_x = 2 focal / width, a_y = 2 focal / height:
        o' = (-a_x o_x / o_z, -a_y o_y / o_z, 1 + 2 / o_z)
        d' = (-a_x (d_x / d_z - o_x / o_z), -a_y (d_y / d_z - o_y / o_z), -2 / o_z)
    and (o', d') is an ordinary ray of the tree's world from then on (lengths, hence optical depth,
    are measured there).  The VIEW direction of the colour stays the unwarped d: volrend.cu:140 copies
    it before the warp of :141, and :155-159 rotates and passes that copy.

The background may be one brightness or an (r, g, b) per ray; alpha does not depend on it.
"""
import numpy as np

_CORNER_ORDER = "x major: child index = 4*ix + 2*iy + iz"


def real_sh(dirs, basis_dim):
    """Real spherical harmonics Y_0..Y_{basis_dim-1} of unit vectors `dirs` [n,3] (float64), ordered
    (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), ...; from scipy's complex harmonics."""
    import scipy.special as sp
    d = np.asarray(dirs, np.float64)
    theta, phi = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
    out = []
    lmax = int(round(np.sqrt(basis_dim))) - 1
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            if hasattr(sp, "sph_harm_y"):
                y = sp.sph_harm_y(l, abs(m), theta, phi)
            else:
                y = sp.sph_harm(abs(m), l, phi, theta)
            out.append(y.real if m == 0 else np.sqrt(2.0) * (y.imag if m < 0 else y.real))
    return np.stack(out, 1)[:, :basis_dim]


def rotate_axis_angle(v, aa):
    """v rotated about the axis aa/|aa| by the angle |aa| (rotation-matrix form, float64)."""
    aa = np.asarray(aa, np.float64)
    ang = np.linalg.norm(aa)
    if ang < 1e-6:
        return np.asarray(v, np.float64)
    k = aa / ang
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    return Rm @ np.asarray(v, np.float64)


class Scene:
    """A PlenOctree as plain float64 numpy: child [cap,8] (relative node offsets, 0 = leaf),
    values [cap,8,data_dim]."""

    def __init__(self, child, data, scale, offset, data_format, extra=None):
        self.child = np.asarray(child).reshape(-1, 8).astype(np.int64)
        self.val = np.asarray(data).astype(np.float64).reshape(self.child.shape[0], 8, -1)
        self.scale = np.asarray(scale, np.float64)
        self.offset = np.asarray(offset, np.float64)
        self.rgba = data_format.upper().startswith("RGBA")
        self.basis_dim = 0 if self.rgba else (self.val.shape[-1] - 1) // 3
        self.kind = "".join(ch for ch in data_format.upper() if ch.isalpha())  # RGBA, SH, SG or ASG
        self.lobes = None if extra is None else np.asarray(extra, np.float64).reshape(self.basis_dim, -1)
        assert self.kind in ("RGBA", "SH") or self.lobes is not None, "an SG / ASG scene needs its lobes"

    @classmethod
    def of(cls, tree):
        """from a SynthTree"""
        return cls(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, tree.extra)

    def locate(self, p):
        """Leaf containing the tree-space point p in [0,1)^3 -> (node, child index, cell lo corner, cell size)."""
        node, lo, size = 0, np.zeros(3), 1.0
        while True:
            size *= 0.5
            bits = (p >= lo + size).astype(np.int64)
            ci = int(4 * bits[0] + 2 * bits[1] + bits[2])
            lo = lo + bits * size
            off = self.child[node, ci]
            if off == 0:
                return node, ci, lo, size
            node += off


def lobe_values(kind, lobes, dirs):
    """[n, B] float64: the SG / ASG lobes (rows of `lobes`, [B,4] / [B,11]) at the unit vectors `dirs` [n,3]; the formulas
    of the module docstring.  The one float64 closed form of the suite (tests/test_sg_asg.py pins the float32 restatement
    to it)."""
    lob = np.asarray(lobes, np.float64)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    B = lob.shape[0]
    if kind == "SG":
        return np.exp(lob[:, 0] * (d @ lob[:, 1:4].T - 1.0)) / B
    assert kind == "ASG", kind
    smooth, dx, dy = d @ lob[:, 8:11].T, d @ lob[:, 2:5].T, d @ lob[:, 5:8].T
    return smooth * np.exp(-lob[:, 0] * dx * dx - lob[:, 1] * dy * dy) / B


def ray_segments(scene, origin_world, dir_world, step_size=1e-4, sigma_thresh=1e-2, bbox=(0, 0, 0, 1, 1, 1), t_max=None,
                 with_t=False):
    """Leaf segments of one ray, front to back: list of (node, child, world length, sigma).  Empty
    leaves (sigma <= sigma_thresh) are skipped.  The ray re-starts step_size beyond each leaf's exit.
    bbox is the crop box, in TREE units.  t_max: the ray ends at that world distance from its origin
    (whole segments only, see the module docstring).  with_t: a fifth entry, the world distance from
    the origin at which the ray enters the segment."""
    dw = np.asarray(dir_world, np.float64)
    dw = dw / np.linalg.norm(dw)
    o = scene.offset + scene.scale * np.asarray(origin_world, np.float64)
    d = scene.scale * dw
    world_per_tree = 1.0 / np.linalg.norm(d)  # world length of one tree-space unit along the ray
    d = d * world_per_tree
    lo, hi = np.asarray(bbox[:3], np.float64) + 1e-6, np.asarray(bbox[3:], np.float64) - 1e-6
    tmin, tmax = 0.0, 1e4
    for a in range(3):
        if abs(d[a]) < 1e-12:
            if not (lo[a] <= o[a] <= hi[a]):
                return []
            continue
        t1, t2 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        tmin, tmax = max(tmin, min(t1, t2)), min(tmax, max(t1, t2))
    if t_max is not None:
        tmax = min(tmax, float(t_max) / world_per_tree)
    if tmax < 0 or tmin > tmax:
        return []
    segs = []
    t = tmin
    while t < tmax:
        p = np.clip(o + t * d, 0.0, 1.0 - 1e-6)
        node, ci, cell_lo, size = scene.locate(p)
        t_exit = np.inf
        for a in range(3):  # distance to the cell's exit face along the ray
            if d[a] > 1e-12:
                t_exit = min(t_exit, (cell_lo[a] + size - p[a]) / d[a])
            elif d[a] < -1e-12:
                t_exit = min(t_exit, (cell_lo[a] - p[a]) / d[a])
        dt = t_exit + step_size
        sigma = scene.val[node, ci, -1]
        if sigma > sigma_thresh:
            seg = (node, ci, dt * world_per_tree, sigma)
            segs.append(seg + (t * world_per_tree,) if with_t else seg)
        t += dt
    return segs


def t_max_in_widest_gap(scene, origin_world, dir_world, min_gap=0.0, **kw):
    """A depth limit (world units) in the middle of the widest stretch of empty space between two media of the ray, or
    None where the ray has no such stretch wider than min_gap (world units): a cut there removes the media behind it
    whatever is done about a cut that falls inside a leaf."""
    segs = ray_segments(scene, origin_world, dir_world, with_t=True, **kw)
    best, where = min_gap, None
    for a, b in zip(segs[:-1], segs[1:]):
        gap = b[4] - (a[4] + a[2])
        if gap > best:
            best, where = gap, a[4] + a[2] + 0.5 * gap
    return where


def view_basis(scene, view_dir, basis_minmax=(0, 24)):
    """the basis functions of the scene at one view direction, those outside basis_minmax zeroed (None for RGBA)"""
    if scene.rgba:
        return None
    B = scene.basis_dim
    vd = np.asarray(view_dir, np.float64)
    vd = vd / np.linalg.norm(vd)
    Y = real_sh(vd[None], B)[0] if scene.kind == "SH" else lobe_values(scene.kind, scene.lobes, vd[None])[0]
    mask = (np.arange(B) >= basis_minmax[0]) & (np.arange(B) <= basis_minmax[1])
    return Y * mask


def leaf_colour(scene, node, ci, view_dir, basis_minmax=(0, 24), basis=None):
    v = scene.val[node, ci]
    if scene.rgba:
        return v[:3].copy()
    B = scene.basis_dim
    Y = view_basis(scene, view_dir, basis_minmax) if basis is None else basis
    return 1.0 / (1.0 + np.exp(-(v[:3 * B].reshape(3, B) @ Y)))


def expected_sample(scene, origin_world, dir_world, bg=1.0, view_dir=None, **kw):
    """Mean and variance of ONE free-flight sample of the ray: (mean[4], var[4]) for r, g, b (background
    composited; bg a brightness or an (r, g, b)) and alpha."""
    view_dir = dir_world if view_dir is None else view_dir
    basis_minmax = kw.pop("basis_minmax", (0, 24))
    segs = ray_segments(scene, origin_world, dir_world, **kw)
    basis = view_basis(scene, view_dir, basis_minmax) if segs else None
    bg = np.broadcast_to(np.asarray(bg, np.float64), (3,))
    T = 1.0
    m1, m2, a = np.zeros(3), np.zeros(3), 0.0
    for node, ci, length, sigma in segs:
        p = T * (1.0 - np.exp(-sigma * length))
        c = leaf_colour(scene, node, ci, view_dir, basis_minmax, basis)
        m1 += p * c
        m2 += p * c * c
        a += p
        T *= np.exp(-sigma * length)
    m1 += bg * T
    m2 += bg * bg * T
    mean = np.concatenate([m1, [a]])
    var = np.concatenate([m2 - m1 * m1, [a * (1.0 - a)]])
    return mean, np.maximum(var, 0.0)


def pinhole_ray(c2w, W, H, fx, fy, x, y):
    """Pixel (x, y) of a pinhole camera looking along -z with +y up, pixel centres at integer coordinates
    measured from (W/2, H/2) (the convention of the reference's headless renderer)."""
    c2w = np.asarray(c2w, np.float64)
    d_cam = np.array([(x - 0.5 * W) / fx, -(y - 0.5 * H) / fy, -1.0])
    d = c2w[:3, :3] @ d_cam
    return c2w[:3, 3], d / np.linalg.norm(d)


def ndc_warp(origin, direction, ndc):
    """The NDC ray (o', d') of a world ray, ndc = (width, height, focal); NeRF appendix C with the near plane at 1."""
    w, h, focal = (float(v) for v in ndc)
    o = np.asarray(origin, np.float64)
    d = np.asarray(direction, np.float64)
    o = o + (-(1.0 + o[2]) / d[2]) * d  # onto the near plane z = -1
    ax, ay = 2.0 * focal / w, 2.0 * focal / h
    o2 = np.array([-ax * o[0] / o[2], -ay * o[1] / o[2], 1.0 + 2.0 / o[2]])
    d2 = np.array([-ax * (d[0] / d[2] - o[0] / o[2]), -ay * (d[1] / d[2] - o[1] / o[2]), -2.0 / o[2]])
    return o2, d2 / np.linalg.norm(d2)


def expected_rays(scene, origins, dirs, t_max=None, background=None, bg=1.0, rot_dirs=None, ndc=None, **kw):
    """-> mean [n,4], var [n,4] of one sample of each of n arbitrary rays (origins, dirs [n,3]; dirs of any length), with a
    depth limit t_max [n] (world units; None or inf: none) and a backdrop background [n,3] per ray (None: bg)."""
    origins = np.asarray(origins, np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    n = origins.shape[0]
    mean, var = np.zeros((n, 4)), np.zeros((n, 4))
    for i in range(n):
        d = dirs[i] / np.linalg.norm(dirs[i])
        vd = d if rot_dirs is None else rotate_axis_angle(d, rot_dirs)
        o = origins[i]
        if ndc is not None:
            o, d = ndc_warp(o, d, ndc)
        tm = None if t_max is None or not np.isfinite(t_max[i]) else float(t_max[i])
        back = bg if background is None else background[i]
        mean[i], var[i] = expected_sample(scene, o, d, bg=back, view_dir=vd, t_max=tm, **kw)
    return mean, var


def expected_frame(scene, c2w, W, H, fx, fy, bg=1.0, rot_dirs=None, ndc=None, **kw):
    """-> mean [4,H,W], var [4,H,W] of one sample per pixel; ndc = (width, height, focal) for an NDC tree"""
    mean = np.zeros((4, H, W))
    var = np.zeros((4, H, W))
    for y in range(H):
        for x in range(W):
            o, d = pinhole_ray(c2w, W, H, fx, fy, x, y)
            vd = d if rot_dirs is None else rotate_axis_angle(d, rot_dirs)
            if ndc is not None:
                o, d = ndc_warp(o, d, ndc)
            mean[:, y, x], var[:, y, x] = expected_sample(scene, o, d, bg=bg, view_dir=vd, **kw)
    return mean, var
