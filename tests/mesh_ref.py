"""The model of rto_draw_mesh_layers / rto_meshes_trace_rays (csrc/rto_mesh_trace.h) and an independent
float64 geometry to judge it by.

bake restates host/mesh_build.cpp's world-space records (double precision, rounded to float once).  trace restates the rule in
numpy float32, operation by operation (numpy's float32 +, -, *, /, sqrt are IEEE, rounded once, as the kernels' are with
contraction off) and BRUTE FORCE: every primitive against every ray, in draw order, no BVH -- the walk of the library may only
skip primitives that cannot win, so equality with this model proves that it culls nothing.  tri64 / seg64 are a float64 geometry
of their own: exact barycentrics and the closest approach of a ray to a segment."""
import functools

import numpy as np

import grid_ref as G
import layer_ref as L
from rt_octree_amd import Mesh, synth

f32 = np.float32
INF = f32(np.inf)
KIND, UNLIT, ID = 27, 28, 29


# ------------------------------------------------------------------ the bake (host/mesh_build.cpp)
def model_matrix(m):
    r = np.asarray(m.rotation, f32).astype(np.float64)
    ang = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    M = np.eye(3)
    if not ang < 1e-3:
        a = r / ang
        c, s = np.cos(ang), np.sin(ang)
        k = 1.0 - c
        X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        for i in range(3):
            for j in range(3):
                M[i, j] = ((c if i == j else 0.0) + k * (a[i] * a[j])) + s * X[i, j]
    return M * float(f32(m.scale))


def estimate_normals(vert, faces):
    """mesh.cpp estimate_normals as mesh_estimate_normals does it: double accumulation in face order"""
    v = np.asarray(vert, f32).astype(np.float64)
    n = len(v)
    faces = np.arange(n // 3 * 3).reshape(-1, 3) if faces is None else np.asarray(faces, np.int64)
    acc = np.zeros((n, 3))
    for f in faces:
        a, b = v[f[1], :3] - v[f[0], :3], v[f[2], :3] - v[f[0], :3]
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        for j in range(3):
            acc[f[j]] += c
    ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
    out = np.asarray(vert, f32).copy()
    with np.errstate(all="ignore"):
        out[:, 6:] = np.where(ln[:, None] > 0, acc / ln[:, None], 0.0).astype(f32)
    return out


def bake(meshes):
    """[n, 32] float32 records in draw order (mesh order, then face order): csrc/rto_mesh_trace.h's layout"""
    recs = []
    for m in meshes:
        if not m.visible:
            continue
        vert = m.vert
        if m.estimate and m.face_size == 3:
            vert = estimate_normals(vert, m.faces)
        M = model_matrix(m)
        v = vert.astype(np.float64)
        t = np.asarray(m.translation, f32).astype(np.float64)
        w = vert.copy()
        for c in range(3):
            w[:, c] = (((M[c, 0] * v[:, 0] + M[c, 1] * v[:, 1]) + M[c, 2] * v[:, 2]) + t[c]).astype(f32)
        q = np.stack([(M[c, 0] * v[:, 6] + M[c, 1] * v[:, 7]) + M[c, 2] * v[:, 8] for c in range(3)], 1)
        ln = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        with np.errstate(all="ignore"):
            w[:, 6:] = np.where(ln[:, None] > 0, q / ln[:, None], 0.0).astype(f32)
        fs = m.face_size
        faces = np.arange(len(w) // fs * fs).reshape(-1, fs) if m.faces is None else m.faces.astype(np.int64)
        rec = np.zeros((len(faces), 32), f32)
        for j in range(fs):
            rec[:, 3 * j:3 * j + 3] = w[faces[:, j], :3]
            rec[:, 9 + 3 * j:12 + 3 * j] = w[faces[:, j], 3:6]
            rec[:, 18 + 3 * j:21 + 3 * j] = w[faces[:, j], 6:]
        words = rec.view(np.uint32)
        words[:, KIND] = fs
        words[:, UNLIT] = int(m.unlit)
        recs.append(rec)
    if not recs:
        return np.zeros((0, 32), f32)
    out = np.concatenate(recs)
    out.view(np.uint32)[:, ID] = np.arange(len(out), dtype=np.uint32)
    return out


# ------------------------------------------------------------------ the rule, float32, brute force
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _fmin(a, b):
    return np.where(a < b, a, b)


def _fmax(a, b):
    return np.where(a > b, a, b)


def hit_triangle(o, d, p0, p1, p2):
    """mesh_hit_triangle for rays o, d [n, 3] -> (t [n] (+inf: none), u, v)"""
    e1, e2, tv = p1 - p0, p2 - p0, o - p0
    e1, e2 = np.broadcast_to(e1, d.shape), np.broadcast_to(e2, d.shape)
    pv = np.stack([d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1], d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2],
                   d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]], 1)
    det = _dot(e1, pv)
    inv = f32(1) / det
    u = _dot(tv, pv) * inv
    qv = np.stack([tv[:, 1] * e1[:, 2] - tv[:, 2] * e1[:, 1], tv[:, 2] * e1[:, 0] - tv[:, 0] * e1[:, 2],
                   tv[:, 0] * e1[:, 1] - tv[:, 1] * e1[:, 0]], 1)
    v = _dot(d, qv) * inv
    t = _dot(e2, qv) * inv
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= f32(1)) & (t > 0)
    return np.where(hit, t, INF).astype(f32), u, v


def hit_segment(o, d, a, b, spread):
    """mesh_hit_segment -> (tc [n] (+inf: none), s)"""
    w = np.broadcast_to(b - a, d.shape)
    w0 = a - o
    A, bd, f, g = _dot(w, w), _dot(w, d), _dot(w0, d), _dot(w0, w)
    den = A - bd * bd
    s = np.where(den > 0, (bd * f - g) / den, f32(0)).astype(f32)
    s = _fmin(_fmax(s, f32(0)), f32(1))
    c = w0 + s[:, None] * w
    tc = _dot(c, d)
    diff = c - tc[:, None] * d
    dist = np.sqrt(_dot(diff, diff))
    hit = (tc > 0) & (dist <= f32(spread) * tc)
    return np.where(hit, tc, INF).astype(f32), s


def shade(rec, kind, unlit, u, v, d):
    """mesh_shade for the rays that hit record `rec` -> rgb [n, 3]"""
    c0, c1, c2 = rec[9:12], rec[12:15], rec[15:18]
    if kind != 3:
        s0 = f32(1) - u
        return s0[:, None] * c0 + u[:, None] * c1
    b0 = (f32(1) - u) - v
    rgb = (b0[:, None] * c0 + u[:, None] * c1) + v[:, None] * c2
    if unlit:
        return rgb
    n = (b0[:, None] * rec[18:21] + u[:, None] * rec[21:24]) + v[:, None] * rec[24:27]
    i1 = f32(1) / np.sqrt((f32(0.5) * f32(0.5) + f32(0.2) * f32(0.2)) + f32(1) * f32(1))
    i2 = f32(1) / np.sqrt((f32(0.5) * f32(0.5) + f32(1) * f32(1)) + f32(0.5) * f32(0.5))
    l1 = np.array([f32(0.5) * i1, f32(0.2) * i1, f32(1) * i1], f32)
    l2 = np.array([f32(-0.5) * i2, f32(-1) * i2, f32(-0.5) * i2], f32)
    dn = _dot(np.broadcast_to(l1, n.shape), n)
    diffuse = f32(0.7) * _fmax(dn, f32(0))
    diffuse2 = f32(0.2) * _fmax(_dot(np.broadcast_to(l2, n.shape), n), f32(0))
    rf = (f32(2) * dn)[:, None] * n - l1
    sp = _fmax(-_dot(d, rf), f32(0))
    for _ in range(5):
        sp = sp * sp
    shade_ = ((f32(0.3) + diffuse) + diffuse2) + f32(0.6) * sp
    return rgb * shade_[:, None]


def normalize_dirs(origins, dirs):
    """mesh_ray_from -> (d [n, 3], ok [n])"""
    o, g = np.asarray(origins, f32), np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        inv = f32(1) / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        d = (g * inv[:, None]).astype(f32)
    ok = np.isfinite(d).all(1) & np.isfinite(o).all(1) & (d != 0).any(1)
    return d, ok


def trace(prims, origins, dirs, line_spread, point_spread, background, want_index=False):
    """(t [n], rgb [n, 3]) of rto_meshes_trace_rays: the nearest primitive, among equal depths the lowest index"""
    with np.errstate(all="ignore"):
        return _trace(prims, origins, dirs, line_spread, point_spread, background, want_index)


def _trace(prims, origins, dirs, line_spread, point_spread, background, want_index):
    o = np.ascontiguousarray(origins, f32).reshape(-1, 3)
    d, ok = normalize_dirs(o, np.ascontiguousarray(dirs, f32).reshape(-1, 3))
    n = len(o)
    best = np.full(n, INF, f32)
    who = np.full(n, -1, np.int64)
    bu, bv = np.zeros(n, f32), np.zeros(n, f32)
    words = prims.view(np.uint32)
    for i in range(len(prims)):  # draw order: `t < best` keeps the lowest index among equal depths
        r = prims[i]
        kind = int(words[i, KIND])
        if kind == 3:
            t, u, v = hit_triangle(o, d, r[0:3], r[3:6], r[6:9])
        else:
            t, u = hit_segment(o, d, r[0:3], r[3:6] if kind == 2 else r[0:3], line_spread if kind == 2 else point_spread)
            v = bv
        take = ok & (t < best)
        best = np.where(take, t, best)
        who = np.where(take, i, who)
        bu, bv = np.where(take, u, bu).astype(f32), np.where(take, v, bv).astype(f32)
    rgb = np.full((n, 3), f32(background), f32)
    for i in np.unique(who[who >= 0]):
        k = np.flatnonzero(who == i)
        rgb[k] = shade(prims[i], int(words[i, KIND]), int(words[i, UNLIT]), bu[k], bv[k], d[k])
    return (best, rgb, who) if want_index else (best, rgb)


def camera_rays(cam):
    """(origins, dirs) [H * W, 3] float32 of a camera's pixels: ray_setup's M xyz before normalising (volrend.camera_rays)"""
    W, H = int(cam.width), int(cam.height)
    m = np.asarray(cam.transform, f32).reshape(-1)
    return np.broadcast_to(m[9:12], (H * W, 3)).copy(), L.pixel_dirs(W, H, cam.fx, cam.fy, m)


def spread(px, fx):
    return (f32(0.5) * f32(px)) / f32(fx)


def layers(prims, cam, line_px=1.0, point_px=1.0, background=1.0, want_index=False):
    """(depth [H, W], color [H, W, 4]) of one frame of rto_draw_mesh_layers without RTO_MESH_MERGE"""
    o, g = camera_rays(cam)
    res = trace(prims, o, g, spread(line_px, cam.fx), spread(point_px, cam.fx), background, want_index)
    H, W = int(cam.height), int(cam.width)
    col = np.ones((H, W, 4), f32)
    col[..., :3] = res[1].reshape(H, W, 3)
    out = (res[0].reshape(H, W), col)
    return out + (res[2].reshape(H, W),) if want_index else out


merge_layers = L.merge_layers  # RTO_MESH_MERGE


# ------------------------------------------------------------------ the scenes of the issue
def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.1, 1.0, (n, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (meshes, W, H).  S1: a lit cube, a polyline of 5 points, 8 points and a camera frustum, each rotated, translated and
    scaled; S2: Sphere(15, 30) (840 triangles) with per-vertex colours, lit, squeezed anisotropically and off centre; S3: two
    coincident triangles of different colours and a segment in their plane"""
    if name == "S1":
        rng = np.random.default_rng(11)
        cube = Mesh.Cube((0.2, 0.7, 0.9)).placed((0.3, -0.5, 0.4), (0.35, -0.2, 0.1), 0.9)
        lines = Mesh.Lines(rng.uniform(-1.0, 1.0, (5, 3)), (0.9, 0.1, 0.1)).placed((0.0, 0.7, -0.2), (-0.3, 0.3, 0.4), 1.1)
        lines.vert[:, 3:6] = _colors(5, 12)
        pts = Mesh.Points(rng.uniform(-1.0, 1.0, (8, 3)), (0.1, 0.6, 0.1)).placed((0.5, 0.1, 0.1), (0.1, 0.2, -0.3), 0.8)
        fr = Mesh.CameraFrustum(40.0, 64.0, 48.0, -0.6, (0.0, 0.0, 0.0)).placed((1.1, 0.4, -0.6), (-0.6, -0.5, 0.5), 1.7)
        return (cube, lines, pts, fr), 64, 48
    if name == "S2":
        sp = Mesh.Sphere(15, 30)
        sp.vert[:, :3] *= np.array([1.0, 0.8, 1.3], f32)
        sp.vert[:, 3:6] = _colors(len(sp.vert), 21)
        return (sp.placed((0.2, 0.3, -0.4), (0.15, -0.1, 0.2), 0.85),), 96, 72
    if name == "S3":
        p = np.array([[-0.9, -0.7, 0.1], [0.9, -0.6, -0.2], [0.1, 0.9, 0.3]], f32)
        a = Mesh._from_points(p, (1.0, 0.0, 0.0), (0, 0, 1), None, 3, True, "A")
        b = Mesh._from_points(p, (0.0, 0.0, 1.0), (0, 0, 1), None, 3, True, "B")
        seg = Mesh.Line(0.5 * (p[0] + p[1]) * f32(1.2), p[2] * f32(1.2), (0.0, 1.0, 0.0))
        return (a, b, seg), 32, 24
    raise KeyError(name)


SCENES = ("S1", "S2", "S3")
POSES = (0, 5, "inside")


def scene_cam(name, pose):
    """poses 0 and 5 of grid_ref's 16-pose orbit, or "inside": a camera inside S2's sphere (used for every scene)"""
    _, W, H = scene(name)
    if pose == "inside":
        return G.Cam(W, H, synth.look_at_c2w((0.2, -0.15, 0.3), (0.9, 0.6, -0.2)))
    return G.Cam(W, H, synth.orbit_poses(16)[pose])


@functools.lru_cache(maxsize=None)
def scene_prims(name):
    p = bake(scene(name)[0])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def scene_layers(name, pose, line_px, background=1.0):
    """the model's (depth, colour, winner) of one case, computed once and shared (read-only); point_px = line_px"""
    out = layers(scene_prims(name), scene_cam(name, pose), line_px, line_px, background, want_index=True)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the geometry, float64
def tri64(prims, cam):
    """exact ray-triangle geometry for the triangles of prims: (ids [T], t [P, T], margin [P, T]) -- margin = min(u, v, 1 - u - v),
    the signed barycentric distance from the nearest edge (> 0 inside); -inf for a ray parallel to the plane"""
    ids = np.flatnonzero(prims.view(np.uint32)[:, KIND] == 3)
    o, d = G.rays64(cam)
    P = prims[ids].astype(np.float64)
    p0, e1, e2 = P[:, 0:3], P[:, 3:6] - P[:, 0:3], P[:, 6:9] - P[:, 0:3]
    nrm = np.cross(e1, e2)                                    # [T, 3]
    den = d @ nrm.T                                           # [P, T]
    with np.errstate(all="ignore"):
        t = ((p0 - o[None, :]) * nrm).sum(1)[None, :] / den
        hit = o[None, None, :] + t[:, :, None] * d[:, None, :] - p0[None]      # [P, T, 3] in-plane offsets
        nn = (nrm * nrm).sum(1)
        u = (np.cross(hit, e2[None]) * nrm[None]).sum(2) / nn[None, :]
        v = (np.cross(e1[None], hit) * nrm[None]).sum(2) / nn[None, :]
        margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
    margin = np.where(np.isfinite(margin) & np.isfinite(t), margin, -np.inf)
    return ids, t, margin


def seg64(prims, cam, line_px, point_px):
    """per pixel over the segments and points of prims: rho = dist / (spread tc) at the closest approach (inf where tc <= 0)
    -> (ids [S], rho [P, S], tc [P, S])"""
    kinds = prims.view(np.uint32)[:, KIND]
    ids = np.flatnonzero(kinds != 3)
    o, d = G.rays64(cam)
    P = prims[ids].astype(np.float64)
    a = P[:, 0:3]
    w = np.where((kinds[ids] == 2)[:, None], P[:, 3:6] - a, 0.0)
    sp = np.where(kinds[ids] == 2, 0.5 * line_px / cam.fx, 0.5 * point_px / cam.fx)
    w0 = a - o[None, :]
    A, g = (w * w).sum(1), (w0 * w).sum(1)
    bd, f = d @ w.T, d @ w0.T
    den = A[None, :] - bd * bd
    with np.errstate(all="ignore"):
        s = np.clip(np.where(den > 1e-14 * A[None, :], (bd * f - g[None, :]) / den, 0.0), 0.0, 1.0)
        c = w0[None] + s[:, :, None] * w[None]
        tc = (c * d[:, None, :]).sum(2)
        dist = np.linalg.norm(c - tc[:, :, None] * d[:, None, :], axis=2)
        rho = np.where(tc > 0, dist / (sp[None, :] * tc), np.inf)
    return ids, rho, tc
