"""The model of rto_draw_grid_layers (grid_kernels.hip) and an independent geometry to judge it by.

grid_depth restates the kernel in numpy float32, operation by operation (numpy's float32 +, -, *, /, sqrt are IEEE, rounded once,
as the kernel's are with contraction off): the GPU tests compare bit for bit.  wire_segments / rho_min / hit_distance are a
float64 geometry of their own -- the deduplicated edges of the truncated cells in world space, built from child[] -- against
which the CPU tests check that the rule draws the wires, only the wires, and the front-most ones."""
import functools

import numpy as np

import layer_ref as L
from rt_octree_amd import synth

f32 = np.float32
INF = f32(np.inf)


# ------------------------------------------------------------------ the rule, float32
def _fmin(a, b):
    return np.where(a < b, a, b)  # a < b ? a : b


def _fmax(a, b):
    return np.where(a > b, a, b)


def leaf_level(child8, pos):
    """levels of child[] visited from the root to the leaf that holds pos ([n, 3] float32 in [0, 1 - 1e-6]): bit 23 - l of the
    24-bit fixed point is the child digit at level l (exact)"""
    q = (pos * f32(16777216.0)).astype(np.uint32)
    n = pos.shape[0]
    node = np.zeros(n, np.int64)
    level = np.zeros(n, np.int32)
    live = np.ones(n, bool)
    for l in range(24):
        b = np.uint32(23 - l)
        digit = (((q[:, 0] >> b) & 1) << 2) | (((q[:, 1] >> b) & 1) << 1) | ((q[:, 2] >> b) & 1)
        c = child8[node, digit]
        level[live] = l + 1
        live = live & (c != 0)
        if not live.any():
            break
        node = np.where(live, node + c, node)
    return level


def _pick(v, a):
    return np.take_along_axis(v, a[:, None], 1)[:, 0]


def _edge_test(p, tau, a, cs, dw, sc, ds, kk):
    """grid_edge_test: p [n, 3] local face points on faces of normal axis a [n] -> the smallest dc among the edges hit, +inf"""
    best = np.full(p.shape[0], INF, f32)
    tw = tau * ds
    dn = _pick(dw, a)
    scn = np.broadcast_to(sc[None, :], p.shape)
    for s in range(2):
        j = np.where(a == 0, 1, 0) if s == 0 else np.where(a == 2, 1, 2)
        k = 3 - a - j
        p_j = _pick(p, j)
        b = np.where(p_j >= f32(0.5), f32(1), f32(0))
        pj = ((p_j - b) / cs) / _pick(scn, j)
        dj = _pick(dw, j)
        q = dj * dj + dn * dn
        perp = (np.abs(pj) * np.abs(dn)) / np.sqrt(q)
        ts = (-(pj * dj)) / q
        dc = tw + ts
        r = kk * dc
        pk = _pick(p, k) + ((ts * _pick(dw, k)) * _pick(scn, k)) * cs
        wk = (r * _pick(scn, k)) * cs
        ok = (dc > 0) & (perp <= r) & (pk >= -wk) & (pk <= f32(1) + wk)
        best = np.where(ok & (dc < best), dc, best)
    return best


camera_dirs = L.unit_dirs  # ray_setup's unit world directions [H * W, 3]


def grid_depth(tree, cam, max_depth, line_px):
    """depth [H, W] float32 of one frame: the world distance along the pixel's unit ray to the grid line, +inf without one.
    cam: anything with width, height, fx, fy, transform (12 floats, column-major)"""
    with np.errstate(all="ignore"):
        return _grid_depth(tree, cam, max_depth, line_px)


def _grid_depth(tree, cam, max_depth, line_px):
    W, H = int(cam.width), int(cam.height)
    m = np.asarray(cam.transform, f32).reshape(-1)
    child8 = np.asarray(tree.child).reshape(-1, 8)
    off, sc = np.asarray(tree.offset, f32), np.asarray(tree.scale, f32)
    dw = camera_dirs(W, H, cam.fx, cam.fy, m)
    n = dw.shape[0]
    cen = np.broadcast_to((off + sc * m[9:12]).astype(f32)[None, :], (n, 3))
    d = dw * sc[None, :]
    ds = f32(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d * ds[:, None]
    t1 = (f32(0) - cen) / d
    t2 = (f32(1) - cen) / d
    tn, tf = _fmin(t1, t2), _fmax(t1, t2)
    tmin, axp = tn[:, 0].copy(), np.zeros(n, np.int64)
    for i in (1, 2):
        up = tn[:, i] > tmin
        tmin = np.where(up, tn[:, i], tmin)
        axp = np.where(up, i, axp)
    tmax = _fmin(_fmin(tf[:, 0], tf[:, 1]), tf[:, 2])
    inside = ~(tmin > 0)
    tmin = np.where(inside, f32(0), tmin).astype(f32)
    axp = np.where(inside, -1, axp)
    kk = (f32(0.5) * f32(line_px)) / f32(cam.fx)
    lmax = min(int(max_depth), 22) + 1
    depth = np.full(n, INF, f32)
    t = tmin.copy()
    live = t < tmax
    for _ in range(3 * (1 << lmax) + 8):
        i = np.flatnonzero(live)
        if i.size == 0:
            break
        di, ti = d[i], t[i]
        pos = _fmax(_fmin(cen[i] + ti[:, None] * di, f32(1.0) - f32(1e-6)), f32(0))
        L = np.minimum(leaf_level(child8, pos), lmax)
        cs = np.ldexp(f32(1), L).astype(f32)
        u = pos * cs[:, None]
        u = u - np.floor(u)
        tu = np.where(di == 0, INF, (np.where(di > 0, f32(1), f32(0)) - u) / di).astype(f32)
        tsl, axo = tu[:, 0].copy(), np.zeros(i.size, np.int64)
        for c in (1, 2):
            lo = tu[:, c] < tsl
            tsl = np.where(lo, tu[:, c], tsl)
            axo = np.where(lo, c, axo)
        e = u + tsl[:, None] * di
        te = ti + tsl / cs
        a_in = axp[i]
        best = np.where(a_in >= 0, _edge_test(u, ti, np.maximum(a_in, 0), cs, dw[i], sc, ds[i], kk), INF)
        best = _fmin(best, _edge_test(e, te, axo, cs, dw[i], sc, ds[i], kk))
        hit = best < INF
        depth[i[hit]] = best[hit]
        t[i] = te + f32(1e-5)
        axp[i] = axo
        live[i] = ~hit & (t[i] < tmax[i])
    return depth.reshape(H, W)


def grid_layers(tree, cams, max_depth, line_px, color=(0.0, 0.0, 0.0), background=1.0):
    """(depth [n, H, W], color [n, H, W, 4]) of rto_draw_grid_layers without RTO_GRID_MERGE"""
    depth = np.stack([grid_depth(tree, c, max_depth, line_px) for c in cams])
    line = np.isfinite(depth)
    col = np.empty(depth.shape + (4,), f32)
    col[..., :3] = np.where(line[..., None], np.asarray(color, f32), f32(background))
    col[..., 3] = 1.0
    return depth, col


merge_layers = L.merge_layers  # RTO_GRID_MERGE


# ------------------------------------------------------------------ the cases of the issue
class Cam(L.Cam):
    def __init__(self, W, H, pose, fx=None):
        super().__init__(W, H, pose, synth.blender_focal(W) if fx is None else fx)


@functools.lru_cache(maxsize=None)
def shape(name):
    """-> (SynthTree, max_depth, W, H).  A: every cell at the cap (no T-junctions); B: leaves of mixed levels; C: B's tree
    anisotropic and off centre, the box's silhouette in view"""
    if name == "A":
        return synth.make_tree(depth_limit=4, basis_dim=9), 1, 160, 120
    t = synth.make_tree(depth_limit=5, basis_dim=9)
    if name == "C":
        sc = (np.asarray(t.scale, f32) * np.array([1.0, 0.8, 1.3], f32)).astype(f32)
        t = synth.SynthTree(t.child, t.data, np.broadcast_to(sc, (3,)).copy(), np.array([0.45, 0.5, 0.56], f32), t.data_format,
                            t.depth_limit, t.stats, t.extra)
    return t, 2, 200, 160


CASES = [(s, p, lp) for s in "ABC" for p in (0, 5) for lp in (1.0, 2.5)]


def case_cam(name, pose):
    _, _, W, H = shape(name)
    return Cam(W, H, synth.orbit_poses(16)[pose])


@functools.lru_cache(maxsize=None)
def case_depth(name, pose, line_px):
    """the model's depth of one case, computed once and shared (read-only)"""
    tree, D, _, _ = shape(name)
    d = grid_depth(tree, case_cam(name, pose), D, line_px)
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------ the geometry, float64
def wire_segments(tree, max_depth):
    """[S, 2, 3] world-space end points of the edges of the cells (the leaves cut off at level max_depth + 1), cut into pieces
    one finest cell long and deduplicated, so that an edge shared by cells of any levels appears once"""
    child8 = np.asarray(tree.child).reshape(-1, 8)
    top = max_depth + 1
    cells = []
    stack = [(0, 0, 0, 0, 0)]  # node, its level (root 0), its integer corner at that level
    while stack:
        node, lvl, ix, iy, iz = stack.pop()
        for digit in range(8):
            cx, cy, cz = 2 * ix + (digit >> 2), 2 * iy + ((digit >> 1) & 1), 2 * iz + (digit & 1)
            skip = int(child8[node, digit])
            if skip == 0 or lvl + 1 >= top:
                cells.append((lvl + 1, cx, cy, cz))
            else:
                stack.append((node + skip, lvl + 1, cx, cy, cz))
    pieces = set()
    for lvl, cx, cy, cz in cells:
        side = 1 << (top - lvl)  # in finest cells
        base = (cx * side, cy * side, cz * side)
        for ax in range(3):
            o1, o2 = [a for a in range(3) if a != ax]
            for c1 in (0, side):
                for c2 in (0, side):
                    for s in range(side):
                        p = list(base)
                        p[o1] += c1
                        p[o2] += c2
                        p[ax] += s
                        pieces.add((ax, p[0], p[1], p[2]))
    P = np.array(sorted(pieces), np.int64)
    a = P[:, 1:].astype(np.float64)
    b = a.copy()
    b[np.arange(len(P)), P[:, 0]] += 1.0
    seg = np.stack([a, b], 1) / float(1 << top)
    off, sc = np.asarray(tree.offset, np.float64), np.asarray(tree.scale, np.float64)
    return (seg - off) / sc, len(cells)


def rays64(cam):
    """(origin [3], unit directions [H * W, 3]) in float64"""
    W, H = cam.width, cam.height
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W)).reshape(-1)
    y = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W)).reshape(-1)
    xyz = np.stack([(x - 0.5 * W) / cam.fx, -(y - 0.5 * H) / cam.fy, -np.ones_like(x)], 1)
    d = xyz @ cam.c2w[:, :3].T
    return cam.c2w[:, 3].copy(), d / np.linalg.norm(d, axis=1, keepdims=True)


def rho_min(S, cam, line_px, sure=0.5, chunk=256):
    """per pixel, over all segments: the smallest rho = distance / (0.5 line_px t_s / fx) at the closest approach of the
    pixel's ray (parameter t_s > 0) to the segment, and the smallest t_s among the segments with rho < sure (+inf: none).
    -> (rho [H, W], t_front [H, W])"""
    o, d = rays64(cam)
    A, v = S[:, 0], S[:, 1] - S[:, 0]
    c = (v * v).sum(1)
    w0 = o[None, :] - A
    e = (v * w0).sum(1)
    rho_out = np.empty(d.shape[0])
    t_out = np.empty(d.shape[0])
    for c0 in range(0, d.shape[0], chunk):
        dd = d[c0:c0 + chunk]
        b = dd @ v.T                       # d . v           [p, s]
        dterm = dd @ w0.T                  # d . (o - A)
        den = c[None, :] - b * b
        ok = den > 1e-14 * c[None, :]
        s = np.clip(np.where(ok, (e[None, :] - b * dterm) / np.where(ok, den, 1.0), 0.0), 0.0, 1.0)
        t = s * b - dterm                  # the ray parameter nearest to the segment point A + s v
        P = A[None, :, :] + s[:, :, None] * v[None, :, :]
        tt = np.maximum(t, 1e-12)
        dist = np.linalg.norm(o[None, None, :] + tt[:, :, None] * dd[:, None, :] - P, axis=2)
        rho = np.where(t > 0, dist / (0.5 * line_px * tt / cam.fx), np.inf)
        rho_out[c0:c0 + chunk] = rho.min(1)
        t_out[c0:c0 + chunk] = np.where(rho < sure, tt, np.inf).min(1)
    return rho_out.reshape(cam.height, cam.width), t_out.reshape(cam.height, cam.width)


def hit_distance(S, cam, depth, line_px, chunk=2048):
    """for the line pixels (finite depth): the distance of the hit point o + depth * dir from the nearest segment, in units of
    the line's half width there, r = 0.5 line_px depth / fx"""
    o, d = rays64(cam)
    dep = np.asarray(depth, np.float64).reshape(-1)
    mask = np.isfinite(dep)
    P = o[None, :] + dep[mask, None] * d[mask]
    A, v = S[:, 0], S[:, 1] - S[:, 0]
    vv = (v * v).sum(1)
    out = np.empty(P.shape[0])
    for c0 in range(0, P.shape[0], chunk):
        p = P[c0:c0 + chunk]
        s = np.clip(((p[:, None, :] - A[None]) * v[None]).sum(2) / vv[None], 0.0, 1.0)
        out[c0:c0 + chunk] = np.linalg.norm(p[:, None, :] - (A[None] + s[:, :, None] * v[None]), axis=2).min(1)
    return out / (0.5 * line_px * dep[mask] / cam.fx)


def chord_over_r(tree, cam, line_px):
    """[H, W]: the length of the ray's chord through the tree's box in world units over r at the entry point (0.5 line_px t_entry
    / fx); 0 for a ray that misses the box"""
    o, d = rays64(cam)
    off, sc = np.asarray(tree.offset, np.float64), np.asarray(tree.scale, np.float64)
    cen, dt = off + sc * o, d * sc  # (dt unnormalised: t stays the world distance)
    with np.errstate(all="ignore"):
        t1, t2 = (0.0 - cen) / dt, (1.0 - cen) / dt
    tmin = np.maximum(np.minimum(t1, t2).max(1), 0.0)
    tmax = np.maximum(t1, t2).min(1)
    with np.errstate(all="ignore"):
        q = np.where(tmax > tmin, (tmax - tmin) / (0.5 * line_px * tmin / cam.fx), 0.0)
    return q.reshape(cam.height, cam.width)
