"""rto_meshes / rto_draw_mesh_layers / rto_meshes_trace_rays (include/rto.h "meshes"): triangles, lines and
points ray-traced into a depth and a colour layer.

mesh_ref.trace restates the rule in numpy float32, brute force; the library's walk of its BVH -- on the CPU through
rto_meshes_trace_rays_host, on the GPU through the kernels -- must equal it bit for bit, which proves that the boxes cull nothing.
The model itself is judged against a float64 geometry (mesh_ref.tri64 / seg64) on the scenes S1-S3 x poses 0, 5 and a camera
inside S2's sphere.  Measured with this model (worst of the nine triangle cases): relative depth error over the sure pixels
1.586e-06 (S2, pose 0; the test asserts 4x that); undecided pixels 0.065 % of the frame (S1) against the 1 % cap; no sure pixel
missed, hit on another triangle, or hit where it is surely outside.  Lines and points (S1): the largest rho on a line pixel 0.9996,
no pixel with rho < 0.5 missed."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_ref as G
import layer_ref
import mesh_ref as M
import rt_octree_amd as R
from helpers import assert_bits_equal, check_33_cameras_in_one_call, gpu_torch as _torch, rcam_of as _rcam
from rt_octree_amd import _lib, synth

E_INVALID, E_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# the worst relative depth error of the model against the float64 geometry over the sure pixels of all cases, as measured (see
# the docstring); the test asserts 4x that
WORST_DEPTH_ERR = 1.586e-6


def _host_set(name):
    return R.MeshSet(list(M.scene(name)[0]), device=None)


# ------------------------------------------------------------------ CPU
def test_mesh_symbols_are_exported_and_the_defaults_are_right():
    hdr = open(os.path.join(ROOT, "include", "rto.h")).read()
    assert "#define RTO_MESH_MERGE 1" in hdr and "typedef struct rto_mesh_params" in hdr and "typedef struct rto_mesh_desc" in hdr
    L = R.lib()
    for name in ("rto_meshes_create", "rto_meshes_get_info", "rto_meshes_free", "rto_mesh_params_default", "rto_draw_mesh_layers",
                 "rto_meshes_trace_rays", "rto_meshes_trace_rays_host"):
        assert ("int %s(" % name in hdr or "void %s(" % name in hdr) and name in _lib.SYMBOLS and hasattr(L, name), name
    assert len(L.rto_draw_mesh_layers.argtypes) == 7
    p = _lib.CMeshParams()
    o = R.RenderOptions(background_brightness=0.25).to_c()
    L.rto_mesh_params_default(C.byref(p), C.byref(o))
    assert (p.line_px, p.point_px, p.background, p.flags) == (1.0, 1.0, 0.25, 0)
    L.rto_mesh_params_default(C.byref(p), None)
    assert (p.line_px, p.point_px, p.background, p.flags) == (1.0, 1.0, 1.0, 0)
    g = R.MeshParams(R.RenderOptions(background_brightness=0.5), line_px=2.5)
    assert (g.line_px, g.point_px, g.background) == (2.5, 1.0, 0.5)
    assert R.MESH_MERGE == 1 and g.to_c(merge=True).flags == 1
    assert hasattr(R.RenderContext, "show_meshes") and callable(R.draw_mesh_layers) and callable(R.trace_mesh_rays)


def _raw_draw(h, cams, n, p, depth, color):
    arr = (_lib.CCamera * max(1, len(cams)))(*[c.to_c() for c in cams]) if cams is not None else None
    return R.lib().rto_draw_mesh_layers(h, arr, n, C.byref(p) if p is not None else None, depth, color, None)


def _invalid_draws(h, cam, depth, color):
    """every RTO_E_INVALID of rto_draw_mesh_layers as (what, thunk -> rc); h: a device set's handle or a fake one"""
    def params(**kw):
        return R.MeshParams(**kw).to_c()

    return layer_ref.invalid_layer_calls(_raw_draw, params, h, cam, depth, color) + [
        ("point_px < 0", lambda: _raw_draw(h, [cam], 1, params(point_px=-1.0), depth, color)),
        ("point_px inf", lambda: _raw_draw(h, [cam], 1, params(point_px=float("inf")), depth, color)),
        ("background nan", lambda: _raw_draw(h, [cam], 1, params(background=float("nan")), depth, color)),
    ]


def _rays_c(o, d, n, ls=0.0, ps=0.0, bg=1.0):
    r = _lib.CMeshRays()
    r.origins, r.dirs, r.n, r.line_spread, r.point_spread, r.background = o, d, n, ls, ps, bg
    return r


def test_mesh_argument_checks_run_before_any_device_use():
    fake = C.create_string_buffer(256)  # never dereferenced: every check below returns first
    h = C.cast(fake, C.c_void_p)
    cam = R.Camera(32, 24, 40.0, 40.0)
    L = R.lib()
    for what, call in _invalid_draws(h, cam, h, h):
        assert call() == E_INVALID, what
        assert L.rto_last_error().decode().startswith("rto_draw_mesh_layers:"), what
    # a host-only set cannot be drawn or traced on a GPU
    hs = _host_set("S3")
    assert _raw_draw(hs._h, [cam], 1, R.MeshParams().to_c(), h, h) == E_INVALID and "host-only" in L.rto_last_error().decode()
    p = h.value
    nan = float("nan")
    for fn, tail in ((L.rto_meshes_trace_rays, (None,)), (L.rto_meshes_trace_rays_host, ())):
        name = "rto_meshes_trace_rays" if tail else "rto_meshes_trace_rays_host"
        for what, args in [
            ("null set", (None, C.byref(_rays_c(p, p, 1)), h, h)),
            ("null rays", (h, None, h, h)),
            ("both outputs null", (h, C.byref(_rays_c(p, p, 1)), None, None)),
            ("n < 0", (h, C.byref(_rays_c(p, p, -1)), h, h)),
            ("null origins", (h, C.byref(_rays_c(None, p, 1)), h, h)),
            ("null dirs", (h, C.byref(_rays_c(p, None, 1)), h, h)),
            ("spread < 0", (h, C.byref(_rays_c(p, p, 1, ls=-1.0)), h, h)),
            ("spread nan", (h, C.byref(_rays_c(p, p, 1, ps=nan)), h, h)),
            ("background inf", (h, C.byref(_rays_c(p, p, 1, bg=float("inf"))), h, h)),
        ]:
            assert fn(*(args + tail)) == E_INVALID, (name, what)
            assert L.rto_last_error().decode().startswith(name + ":"), (name, what)
    assert L.rto_meshes_trace_rays(hs._h, C.byref(_rays_c(p, p, 1)), h, h, None) == E_INVALID


def _create_rc(mesh, **over):
    d, keep = mesh.desc()
    for k, v in over.items():
        if k in ("rotation", "translation"):
            for i in range(3):
                getattr(d, k)[i] = v[i]
        else:
            setattr(d, k, v)
    h = C.c_void_p(None)
    rc = R.lib().rto_meshes_create(C.byref(d), 1, -1, C.byref(h))
    if rc == 0:
        R.lib().rto_meshes_free(h)
    return rc


def test_meshes_create_refusals_and_empty_sets():
    L = R.lib()
    cube = R.Mesh.Cube()
    h = C.c_void_p(None)
    d, _keep = cube.desc()
    nan = float("nan")
    assert L.rto_meshes_create(None, 1, -1, C.byref(h)) == E_INVALID
    assert L.rto_meshes_create(C.byref(d), 1, -1, None) == E_INVALID
    assert L.rto_meshes_create(C.byref(d), -1, -1, C.byref(h)) == E_INVALID
    assert _create_rc(cube) == 0
    assert _create_rc(cube, face_size=0) == E_INVALID and _create_rc(cube, face_size=4) == E_INVALID
    assert _create_rc(cube, scale=nan) == E_INVALID and _create_rc(cube, scale=float("inf")) == E_INVALID
    assert _create_rc(cube, rotation=(0.0, nan, 0.0)) == E_INVALID and _create_rc(cube, translation=(float("inf"), 0.0, 0.0)) == E_INVALID
    assert _create_rc(cube, vert=None) == E_INVALID
    bad = R.Mesh.Cube()
    bad.vert[7, 1] = nan
    assert _create_rc(bad) == E_INVALID and "non-finite position" in L.rto_last_error().decode()
    sp = R.Mesh.Sphere(4, 6)
    sp.faces[3, 1] = len(sp.vert)
    assert _create_rc(sp) == E_INVALID and "face index" in L.rto_last_error().decode()
    # more than 2^30 primitives: refused on the counts alone, before any vertex or index is read (the pointers are fake)
    d.faces, d.n_faces = C.cast(C.create_string_buffer(64), C.c_void_p).value, (1 << 30) + 1
    assert L.rto_meshes_create(C.byref(d), 1, -1, C.byref(h)) == E_INVALID and "2^30" in L.rto_last_error().decode()
    # n == 0 and zero primitives: valid, empty sets; every ray misses them
    for meshes in ([], [R.Mesh.Points(np.zeros((0, 3)))]):
        ms = R.MeshSet(meshes, device=None)
        assert (ms.n_prims, ms.nodes, ms.device_bytes) == (0, 0, 0) and (ms.bounds[0] == 0).all() and (ms.bounds[1] == 0).all()
        t, rgb = ms.trace_rays_host(np.zeros((3, 3), f32), np.ones((3, 3), f32), 0.01, 0.01, 0.25)
        assert np.isposinf(t).all() and (rgb == 0.25).all()
    # an invisible mesh is not passed in
    hidden = R.Mesh.Cube()
    hidden.visible = False
    assert R.MeshSet([hidden, R.Mesh.Line((0, 0, 0), (1, 0, 0))], device=None).n_prims == 1


@pytest.mark.parametrize("name", M.SCENES)
def test_bake_and_bvh_layout(name):
    """the records equal mesh_ref.bake bit for bit (the model transform in double, rounded once); the BVH is depth-first with
    miss links, its leaves hold at most 4 records in draw order, every record once, every box holds its records, and a second
    build gives the same bytes"""
    ms = _host_set(name)
    prims, nodes = ms.download()
    want = M.scene_prims(name)
    ids = prims.view(np.uint32)[:, M.ID].astype(np.int64)
    assert sorted(ids) == list(range(len(want)))
    assert_bits_equal(prims[np.argsort(ids)], want, "baked records")
    kinds = want.view(np.uint32)[:, M.KIND]
    assert (ms.triangles, ms.segments, ms.points) == tuple(int((kinds == k).sum()) for k in (3, 2, 1))
    pos = want[:, :9].reshape(-1, 3, 3)
    used = np.arange(3)[None, :] < kinds[:, None]
    assert np.array_equal(ms.bounds[0], np.where(used[..., None], pos, np.inf).min((0, 1)))
    assert np.array_equal(ms.bounds[1], np.where(used[..., None], pos, -np.inf).max((0, 1)))
    words = nodes.view(np.uint32)
    n = len(nodes)
    assert n == ms.nodes
    seen = []

    def check(i):
        """-> (the node after node i's subtree, lo, hi, thick) from the records below it"""
        link = int(words[i, 3])
        miss = link & 0x3fffffff
        if link & 0x80000000:
            first, count = int(words[i, 7]) >> 2, (int(words[i, 7]) & 3) + 1
            assert miss == i + 1
            rec = prims[first:first + count]
            rid = ids[first:first + count]
            assert list(rid) == sorted(rid)
            seen.extend(range(first, first + count))
            k = rec.view(np.uint32)[:, M.KIND]
            p = rec[:, :9].reshape(-1, 3, 3)
            u = np.arange(3)[None, :] < k[:, None]
            lo, hi = np.where(u[..., None], p, np.inf).min((0, 1)), np.where(u[..., None], p, -np.inf).max((0, 1))
            thick = bool((k != 3).any())
        else:
            e1, lo1, hi1, t1 = check(i + 1)
            e2, lo2, hi2, t2 = check(e1)
            assert e2 == miss
            lo, hi, thick = np.minimum(lo1, lo2), np.maximum(hi1, hi2), t1 or t2
        assert np.array_equal(nodes[i, 0:3], lo) and np.array_equal(nodes[i, 4:7], hi) and bool(link & 0x40000000) == thick
        return miss, lo, hi, thick

    assert check(0)[0] == n and seen == list(range(len(want)))
    p2, n2 = _host_set(name).download()
    assert_bits_equal(p2, prims, "a second build: records")
    assert np.array_equal(n2.view(np.uint32), words)
    if name == "S2":
        assert ms.triangles == 840 and n >= 2 * 210 - 1  # several levels, leaves of at most 4


def test_estimate_normals_and_identity_transform():
    sp = R.Mesh.Sphere(6, 8)
    sp.estimate = True
    sp.placed((0.0005, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)  # |r| < 1e-3: the identity
    ms = R.MeshSet([sp], device=None)
    prims, _ = ms.download()
    prims = prims[np.argsort(prims.view(np.uint32)[:, M.ID])]
    assert_bits_equal(prims, M.bake([sp]), "estimated normals")
    assert np.array_equal(prims[:, 0:3], sp.vert[sp.faces[:, 0], :3]), "identity: positions untouched (-0 + 0 = +0 aside)"
    n = prims[:, 18:27].reshape(-1, 3)
    ln = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.allclose(ln[ln > 0], 1.0, atol=1e-6) and (ln > 0).mean() > 0.9


def _all_cases():
    return [(s, p, lp) for s in M.SCENES for p in M.POSES for lp in (1.0, 2.5)]


@pytest.mark.parametrize("name,pose,line_px", _all_cases())
def test_bvh_walk_on_the_cpu_equals_the_brute_force_model(name, pose, line_px):
    """every pixel's ray: the kernels' code on the host, through the BVH, against all primitives in draw order"""
    cam = M.scene_cam(name, pose)
    want_d, want_c, _ = M.scene_layers(name, pose, line_px, 0.75)
    o, g = M.camera_rays(cam)
    sp = M.spread(line_px, cam.fx)
    t, rgb = _host_set(name).trace_rays_host(o, g, sp, sp, 0.75)
    assert_bits_equal(t, want_d.reshape(-1), "depth")
    assert_bits_equal(rgb, want_c[..., :3].reshape(-1, 3), "colour")


def test_bvh_walk_on_random_and_degenerate_rays():
    """20 000 random rays through S2's bounds (origins inside and outside, unnormalised directions), S1's mix of kinds with wide
    spreads, and degenerate rays: a miss, whatever they would hit"""
    rng = np.random.default_rng(5)
    for name, n, ls, ps in (("S2", 20000, 0.0, 0.0), ("S1", 4000, 0.02, 0.05), ("S3", 2000, 0.0, 0.01)):
        ms = _host_set(name)
        lo, hi = ms.bounds
        ext = (hi - lo).astype(np.float64)
        a = lo + rng.uniform(-0.6, 1.6, (n, 3)) * ext
        b = lo + rng.uniform(0.0, 1.0, (n, 3)) * ext
        o, g = a.astype(f32), ((b - a) * rng.uniform(0.01, 100.0, (n, 1))).astype(f32)
        g[::7, rng.integers(0, 3)] = 0.0  # axis-parallel components
        t, rgb = ms.trace_rays_host(o, g, ls, ps, 0.5)
        want_t, want_c = M.trace(M.scene_prims(name), o, g, ls, ps, 0.5)
        assert np.isfinite(want_t).mean() > 0.1, name
        assert_bits_equal(t, want_t, name + ": depth of random rays")
        assert_bits_equal(rgb, want_c, name + ": colour of random rays")
    ms = _host_set("S2")
    c = (0.5 * (ms.bounds[0] + ms.bounds[1])).astype(f32)
    o = np.tile(c - np.array([3.0, 0.0, 0.0], f32), (7, 1))
    g = np.tile(np.array([1.0, 0.0, 0.0], f32), (7, 1))
    g[1] = 0.0
    g[2, 1] = np.nan
    g[3, 0] = np.inf
    g[4] = 1e-30   # the squared length underflows
    g[5] = 3e19    # ... overflows
    o[6, 2] = np.inf
    t, rgb = ms.trace_rays_host(o, g, 0.0, 0.0, 0.125)
    assert np.isfinite(t[0]) and (rgb[0] != 0.125).any()
    assert np.isposinf(t[1:]).all() and (rgb[1:] == 0.125).all()
    want_t, want_c = M.trace(M.scene_prims("S2"), o, g, 0.0, 0.0, 0.125)
    assert_bits_equal(t, want_t, "degenerate rays: depth")
    assert_bits_equal(rgb, want_c, "degenerate rays: colour")


def _sure_pixels(name, pose):
    """the float64 verdict on the triangles of a scene alone -> (inside [P] bool, its triangle [P], its distance [P], outside [P])"""
    prims = M.scene_prims(name)
    ids, t, margin = M.tri64(prims, M.scene_cam(name, pose))
    front = t > 0
    solid = front & (margin >= 1e-4)          # surely hit
    maybe = front & (margin > -1e-4)          # not surely missed
    tt = np.where(solid, t, np.inf)
    near = tt.argmin(1)                       # (the lowest index among equal distances: argmin takes the first)
    t_near = tt[np.arange(len(tt)), near]
    blocked = (maybe & ~solid & (t < t_near[:, None])).any(1)   # an undecided triangle in front of the nearest sure one
    inside = np.isfinite(t_near) & ~blocked
    outside = ~maybe.any(1)
    return inside, ids[near], t_near, outside


@pytest.mark.parametrize("name,pose", [(s, p) for s in M.SCENES for p in M.POSES])
def test_model_triangles_against_float64(name, pose):
    prims = M.scene_prims(name)
    tri = prims[prims.view(np.uint32)[:, M.KIND] == 3]
    tri_ids = np.flatnonzero(prims.view(np.uint32)[:, M.KIND] == 3)
    cam = M.scene_cam(name, pose)
    d, _c, who = M.layers(tri, cam, 1.0, 1.0, 1.0, want_index=True)
    d, who = d.reshape(-1), who.reshape(-1)
    inside, want_who, t64, outside = _sure_pixels(name, pose)
    undecided = ~inside & ~outside
    err = np.abs(d[inside].astype(np.float64) - t64[inside]) / t64[inside] if inside.any() else np.zeros(1)
    print("%s pose %s: %d sure inside, %d sure outside, %d undecided (%.3f %%), worst depth error %.3e" % (
        name, pose, inside.sum(), outside.sum(), undecided.sum(), 100.0 * undecided.mean(), err.max()))
    assert undecided.sum() <= 0.01 * undecided.size, "the band of undecided pixels is capped at 1 % of the frame"
    assert np.isfinite(d[inside]).all(), "a sure inside pixel is missed"
    assert np.array_equal(tri_ids[who[inside]], want_who[inside]), "a sure inside pixel shows another triangle"
    assert np.isposinf(d[outside]).all(), "a sure outside pixel is hit"
    assert err.max() <= 4.0 * WORST_DEPTH_ERR


@pytest.mark.parametrize("pose", M.POSES)
@pytest.mark.parametrize("line_px", [1.0, 2.5])
def test_model_lines_and_points_against_float64(pose, line_px):
    """S1's segments and points alone (nothing occludes them): the grid's two bounds"""
    prims = M.scene_prims("S1")
    thick = prims[prims.view(np.uint32)[:, M.KIND] != 3]
    cam = M.scene_cam("S1", pose)
    d, _c = M.layers(thick, cam, line_px, line_px, 1.0)
    line = np.isfinite(d.reshape(-1))
    _ids, rho, _tc = M.seg64(thick, cam, line_px, line_px)
    rmin = rho.min(1)
    print("S1 pose %s line_px %.1f: %d line pixels, largest rho on one %.4f, %d pixels with rho < 0.5" % (
        pose, line_px, line.sum(), rmin[line].max() if line.any() else 0.0, (rmin < 0.5).sum()))
    if pose != "inside":
        assert line.sum() > 50
    assert not (rmin[line] > 1.5).any(), "a line pixel further than 1.5 half widths from every segment"
    assert line[rmin < 0.5].all(), "a pixel within half a half width of a segment is no line pixel"
    # the whole scene is the nearer of its two halves
    tri = prims[prims.view(np.uint32)[:, M.KIND] == 3]
    dt, _ = M.layers(tri, cam, line_px, line_px, 1.0)
    full = M.scene_layers("S1", pose, line_px, 0.75)[0]
    assert_bits_equal(full, np.minimum(dt, d), "S1: the nearer of triangles and lines")


def test_tie_rule_lowest_index_wins():
    """S3: two coincident triangles; the lower-indexed one's colour wins everywhere they overlap, swapping them swaps the result"""
    a, b, seg = M.scene("S3")[0]
    cam = M.scene_cam("S3", 0)
    o, g = M.camera_rays(cam)
    sp = M.spread(1.0, cam.fx)
    out = {}
    for key, order in (("ab", [a, b, seg]), ("ba", [b, a, seg])):
        ms = R.MeshSet(order, device=None)
        t, rgb = ms.trace_rays_host(o, g, sp, sp, 1.0)
        mt, mrgb, who = M.trace(M.bake(order), o, g, sp, sp, 1.0, want_index=True)
        assert_bits_equal(t, mt, key + ": depth")
        assert_bits_equal(rgb, mrgb, key + ": colour")
        out[key] = (t, rgb, who)
    tri = out["ab"][2] == 0
    assert tri.sum() > 50 and not (out["ab"][2] == 1).any() and np.array_equal(out["ba"][2] == 0, tri)
    # (the interpolation weights sum to 1 only up to rounding: the winner's channel is 1 - a few ulp, the loser's exactly 0)
    ab, ba = out["ab"][1][tri], out["ba"][1][tri]
    assert (np.abs(ab[:, 0] - 1) < 1e-6).all() and (ab[:, 1:] == 0).all() and (np.abs(ba[:, 2] - 1) < 1e-6).all() and (ba[:, :2] == 0).all()
    assert_bits_equal(out["ab"][0], out["ba"][0], "the depth does not depend on the order")
    assert (out["ab"][2] == 2).any()  # the segment in their plane wins somewhere (outside the triangles, or nearer by rounding)


# ------------------------------------------------------------------ GPU
def _dev_set(name):
    return R.MeshSet(list(M.scene(name)[0]), device=0)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _want(name, poses, line_px, bg):
    d = np.stack([M.scene_layers(name, p, line_px, bg)[0] for p in poses])
    c = np.stack([M.scene_layers(name, p, line_px, bg)[1] for p in poses])
    return d, c


@pytest.mark.gpu
@pytest.mark.parametrize("line_px", [1.0, 2.5])
@pytest.mark.parametrize("name", M.SCENES)
def test_layers_equal_the_model_bit_for_bit(name, line_px):
    """one call of three cameras: orbit poses 0 and 5 and the camera inside S2's sphere"""
    ms = _dev_set(name)
    cams = [_rcam(M.scene_cam(name, p)) for p in M.POSES]
    want_d, want_c = _want(name, M.POSES, line_px, 0.75)
    d, c = R.draw_mesh_layers(ms, cams, R.MeshParams(line_px=line_px, point_px=line_px, background=0.75))
    _torch().cuda.synchronize()
    assert_bits_equal(_np(d), want_d, "depth")
    assert_bits_equal(_np(c), want_c, "colour")
    info = _lib.CMeshesInfo()
    assert R.lib().rto_meshes_get_info(ms._h, C.byref(info)) == 0
    assert info.device == 0 and info.device_bytes == 32 * info.nodes + 128 * (info.triangles + info.segments + info.points)


@pytest.mark.gpu
def test_33_cameras_in_one_call_equal_33_calls_and_n_0_writes_nothing():
    torch = _torch()
    ms = _dev_set("S1")
    W, H = 32, 24
    poses = synth.orbit_poses(33)
    cams = [_rcam(G.Cam(W, H, poses[i])) for i in range(33)]
    params = R.MeshParams(line_px=1.5, point_px=3.0, background=0.5)
    prims = M.scene_prims("S1")
    check_33_cameras_in_one_call(lambda c, **kw: R.draw_mesh_layers(ms, c, params, **kw), cams,
                                 lambda f: M.layers(prims, G.Cam(W, H, poses[f]), 1.5, 3.0, 0.5))
    buf = torch.full((16,), 7.0, device="cuda")
    assert _raw_draw(ms._h, [cams[0]], 0, params.to_c(), C.c_void_p(buf.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (buf == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", M.SCENES)
def test_rays_equal_the_layers_and_split_batches_give_the_same_bytes(name):
    torch = _torch()
    ms = _dev_set(name)
    gcam = M.scene_cam(name, 5)
    cam = _rcam(gcam)
    lp = 2.5
    want_d, want_c, _ = M.scene_layers(name, 5, lp, 0.75)
    o, g = R.camera_rays(cam)
    sp = float(M.spread(lp, cam.fx))
    t, rgb = R.trace_mesh_rays(ms, o, g, sp, sp, 0.75)
    d, c = R.draw_mesh_layers(ms, [cam], R.MeshParams(line_px=lp, point_px=lp, background=0.75))
    torch.cuda.synchronize()
    assert_bits_equal(_np(t), _np(d).reshape(-1), "rays vs layers: depth")
    assert_bits_equal(_np(rgb), _np(c)[0, ..., :3].reshape(-1, 3), "rays vs layers: colour")
    assert_bits_equal(_np(t), want_d.reshape(-1), "rays vs the model")
    k = len(o) // 3 + 5
    t1, c1 = R.trace_mesh_rays(ms, o[:k], g[:k], sp, sp, 0.75)
    t2, c2 = R.trace_mesh_rays(ms, o[k:], g[k:], sp, sp, 0.75)
    assert_bits_equal(np.concatenate([_np(t1), _np(t2)]), _np(t), "a split batch: depth")
    assert_bits_equal(np.concatenate([_np(c1), _np(c2)]), _np(rgb), "a split batch: colour")
    # degenerate rays
    bad = np.tile(g[len(g) // 2], (6, 1)).astype(f32)
    ob = np.tile(o[0], (6, 1)).astype(f32)
    bad[1] = 0.0
    bad[2, 1] = np.nan
    bad[3, 0] = np.inf
    bad[4] = 1e-30
    ob[5, 2] = np.inf
    tb, cb = R.trace_mesh_rays(ms, ob, bad, sp, sp, 0.125)
    torch.cuda.synchronize()
    assert np.isposinf(_np(tb)[1:]).all() and (_np(cb)[1:] == 0.125).all()
    wt, wc = M.trace(M.scene_prims(name), ob, bad, sp, sp, 0.125)
    assert_bits_equal(_np(tb), wt, "degenerate rays: depth")
    assert_bits_equal(_np(cb), wc, "degenerate rays: colour")


def _prefill(want_d, seed):
    """existing depth: nearer than the mesh, farther than it, 0, -1, NaN and +inf, and a colour to go with it"""
    rng = np.random.default_rng(seed)
    base = np.where(np.isfinite(want_d), want_d, f32(4.0))
    old = (base * rng.choice(np.array([0.5, 1.5], f32), want_d.shape)).astype(f32)
    k = rng.integers(0, 12, want_d.shape)
    old[k == 0] = 0.0
    old[k == 1] = -1.0
    old[k == 2] = np.nan
    old[k == 3] = np.inf
    col = rng.uniform(0.0, 1.0, want_d.shape + (4,)).astype(f32)
    return old, col


@pytest.mark.gpu
def test_merge_is_the_depth_test_against_what_the_buffers_hold():
    torch = _torch()
    ms = _dev_set("S1")
    cams = [_rcam(M.scene_cam("S1", p)) for p in (0, 5)]
    new_d, new_c = _want("S1", (0, 5), 2.5, 0.3)
    old_d, old_c = _prefill(new_d, 3)
    want_d, want_c = M.merge_layers(new_d, new_c, old_d, old_c)
    with np.errstate(invalid="ignore"):
        taken = np.isfinite(new_d) & (old_d > new_d)
        dead = ~(old_d > 0)
    assert taken.sum() > 200 and (np.isfinite(new_d) & ~taken & ~dead).sum() > 200 and (np.isfinite(new_d) & dead).sum() > 50
    params = R.MeshParams(line_px=2.5, point_px=2.5, background=0.3)
    d, c = torch.from_numpy(old_d).cuda(), torch.from_numpy(old_c).cuda()
    R.draw_mesh_layers(ms, cams, params, depth=d, color=c, merge=True)
    torch.cuda.synchronize()
    assert_bits_equal(_np(d), want_d, "merged depth (untouched pixels keep their bytes)")
    assert_bits_equal(_np(c), want_c, "merged colour")
    d = torch.from_numpy(old_d).cuda()
    R.draw_mesh_layers(ms, cams, params, depth=d, color=False, merge=True)
    torch.cuda.synchronize()
    assert_bits_equal(_np(d), want_d, "merged depth without a colour buffer")


def _upload(tree):
    return R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra)


@pytest.mark.gpu
def test_meshes_then_the_grid_merged_equal_the_nearer_of_the_two_models():
    torch = _torch()
    tree = synth.make_tree(depth_limit=5, basis_dim=9)
    dt = _upload(tree)
    ms = _dev_set("S1")
    gcams = [M.scene_cam("S1", p) for p in (0, 5)]
    cams = [_rcam(c) for c in gcams]
    d, c = R.draw_mesh_layers(ms, cams, R.MeshParams(line_px=1.0, background=0.6))
    R.draw_grid_layers(dt, cams, R.GridParams(max_depth=2, line_px=1.0, color=[0.0, 0.0, 0.0], background=0.6), depth=d, color=c, merge=True)
    torch.cuda.synchronize()
    md, mc = _want("S1", (0, 5), 1.0, 0.6)
    gd, gc = G.grid_layers(tree, gcams, 2, 1.0, color=(0.0, 0.0, 0.0), background=0.6)
    want_d, want_c = G.merge_layers(gd, gc, md, mc)
    assert (np.isfinite(gd) & (gd < md)).sum() > 200 and (np.isfinite(md) & (md < gd)).sum() > 200
    assert_bits_equal(_np(d), want_d, "meshes, then the grid merged: depth")
    assert_bits_equal(_np(c), want_c, "meshes, then the grid merged: colour")
    assert_bits_equal(_np(d), np.minimum(md, gd), "the per-pixel nearer of the two")


def _frame_rgba(aux):
    """aux [8, H, W] -> (r, g, b, alpha) [H * W, 4]"""
    return np.ascontiguousarray(np.asarray(aux)[:4].reshape(4, -1).T)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 6])
def test_frames_over_the_mesh_layers_equal_rays_limited_by_the_mesh_trace(spp):
    """show_meshes + launch_renderer (single frame, and 4 frames batched) == rto_launch_rays with t_max / background taken from
    rto_meshes_trace_rays; rto_denoise then returns finite pixels"""
    torch = _torch()
    from rt_octree_amd import denoiser
    tree = synth.make_tree(depth_limit=5, basis_dim=9)
    dt = _upload(tree)
    ms = _dev_set("S1")
    W, H = M.scene("S1")[1:]
    poses = synth.orbit_poses(16)
    cams = [_rcam(G.Cam(W, H, poses[p])) for p in (0, 5, 9, 13)]
    opt = R.RenderOptions(spp=spp, denoise=False, background_brightness=0.8)

    def rays_of(cam, ctx):
        o, g = R.camera_rays(cam)
        sp = float(M.spread(1.0, cam.fx))
        t, rgb = R.trace_mesh_rays(ms, o, g, sp, sp, 0.8)
        return _np(R.render_rays(dt, o, g, opt, ctx, t_max=t, background=rgb)), _np(t)

    ctx = R.RenderContext(W, H)
    ctx.rng_seed()
    ctx.rng_advance()
    d, c = ctx.show_meshes(ms, cams[0], opt, tree=dt)
    assert ctx.layers() == (d.data_ptr(), c.data_ptr()) and not ctx.offscreen
    R.launch_renderer(dt, cams[0], opt, ctx, offscreen=False)
    aux = ctx.download_aux()
    want, t = rays_of(cams[0], ctx)
    assert_bits_equal(_np(d)[0].reshape(-1), t, "the layer show_meshes drew vs the ray trace")
    assert_bits_equal(_frame_rgba(aux), want, "single frame over the meshes vs rto_launch_rays")
    assert np.isfinite(t).sum() > 300 and (want[np.isfinite(t), 3] < 1).any()

    jumps = [3, 1, 4, 2]
    bctx = R.RenderContext(W, H, frames=4)
    bctx.rng_seed()
    bctx.show_meshes(ms, cams, opt, tree=dt)
    R.launch_renderer_batch(dt, cams, opt, bctx, rng_jumps=jumps)
    torch.cuda.synchronize()
    baux = torch.as_tensor(bctx.batch_views()[0], device="cuda:0").cpu().numpy()
    one = R.RenderContext(W, H)
    for f in range(4):
        one.rng_seed()
        one.rng_advance(jumps[f] << 32)
        assert_bits_equal(_frame_rgba(baux[f]), rays_of(cams[f], one)[0], "batched frame %d over the meshes vs rto_launch_rays" % f)

    torch.manual_seed(3)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval())
    dn = R.RenderOptions(spp=spp, denoise=True, background_brightness=0.8)
    R.launch_renderer_batch(dt, cams, dn, bctx, rng_jumps=jumps)
    bctx.select_frame(0)
    net.denoise(bctx, n=4)
    torch.cuda.synchronize()
    image = torch.as_tensor(bctx.batch_views()[2], device="cuda:0").cpu().numpy()
    assert image.shape == (4, H, W, 4) and np.isfinite(image).all()


@pytest.mark.gpu
def test_an_empty_set_draws_background_and_refusals_leave_the_buffers_untouched():
    torch = _torch()
    cam = _rcam(M.scene_cam("S3", 0))
    empty = R.MeshSet([], device=0)
    d, c = R.draw_mesh_layers(empty, [cam], R.MeshParams(background=0.4))
    torch.cuda.synchronize()
    assert np.isposinf(_np(d)).all() and (_np(c)[..., :3] == f32(0.4)).all() and (_np(c)[..., 3] == 1).all()
    o, g = R.camera_rays(cam)
    t, rgb = R.trace_mesh_rays(empty, o, g, 0.01, 0.01, 0.4)
    assert np.isposinf(_np(t)).all() and (_np(rgb) == f32(0.4)).all()
    ms = _dev_set("S3")
    depth = torch.full((2, cam.height, cam.width), 3.25, device="cuda")
    color = torch.full((2, cam.height, cam.width, 4), -7.5, device="cuda")
    for what, call in _invalid_draws(ms._h, cam, C.c_void_p(depth.data_ptr()), C.c_void_p(color.data_ptr())):
        assert call() == E_INVALID, what
    torch.cuda.synchronize()
    assert (depth == 3.25).all() and (color == -7.5).all(), "a refused call wrote to its buffers"
    # meshes are in world space: show_meshes refuses an NDC tree as the grid does
    tree = synth.make_tree(depth_limit=4, basis_dim=9)
    ndc = _upload(tree)
    ndc.set_ndc(40.0, 30.0, 35.0)
    ctx = R.RenderContext(cam.width, cam.height)
    with pytest.raises(R.RtoError) as e:
        ctx.show_meshes(ms, cam, R.RenderOptions(), tree=ndc)
    assert e.value.code == E_UNSUPPORTED and ctx.layers() == (None, None)


@pytest.mark.gpu
def test_cli_draw_writes_what_the_python_route_renders(tmp_path):
    """volrend_headless --draw drawlist.npz --grid 2 and --draw a.obj --draw b.npz: the PNGs decode to the RGBA8 of
    RenderContext.show_meshes (+ show_grid merged over them) + launch_renderer with the CLI's per-pose RNG"""
    import subprocess
    from PIL import Image
    binary = os.path.join(ROOT, "rt-octree_amd", "bin", "volrend_headless")
    tree = synth.make_tree(depth_limit=5, basis_dim=9, seed=7)
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(2)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    op = synth.write_opt_json(str(tmp_path / "opt.json"), denoise=False, spp=6)
    rng = np.random.default_rng(2)
    dl = str(tmp_path / "drawlist.npz")
    np.savez(dl, cams="camerafrustum", cams__focal_length=60.0, cams__image_width=96.0, cams__image_height=64.0, cams__z=-0.5,
             cams__r=rng.uniform(-1, 1, (6, 3)), cams__t=rng.uniform(-1, 1, (6, 3)), cams__connect=1,
             ball="sphere", ball__rings=6, ball__sectors=8, ball__scale=0.4, ball__translation=np.array([0.3, 0.2, 0.6]))
    obj = str(tmp_path / "a.obj")
    open(obj, "w").write("v -1 -1 0.2 1 0 0\nv 1 -1 0.2 0 1 0\nv 0 1 0.4 0 0 1\nf 1 2 3\n")
    W, H = 96, 64
    dt = _upload(tree)
    opt = R.RenderOptions.from_json(op)
    for files, grid in (([dl], 2), ([obj, dl], None)):
        ms = R.MeshSet.load(files, device=0)
        assert ms.n_prims > 50
        if grid is not None:
            opt.show_grid, opt.grid_max_depth = True, grid
        want = []
        for i in range(2):
            ctx = R.RenderContext(W, H)
            ctx.rng_seed()
            for _ in range(i):
                ctx.rng_advance()
            cam = _rcam(G.Cam(W, H, poses[i]))
            d, _c = ctx.show_meshes(ms, cam, opt, tree=dt)
            assert np.isfinite(_np(d)).sum() > 100
            if grid is not None:
                ctx.show_grid(dt, cam, opt, merge=True)
            R.launch_renderer(dt, cam, opt, ctx)
            want.append(ctx.download_rgba8())
        for batch in ("1", "2"):
            out = str(tmp_path / ("out%s_%s" % (batch, grid)))
            cmd = [binary, tp, pp, "--options", op, "-w", str(W), "-h", str(H), "-o", out, "--warmup", "0", "--batch", batch]
            for f in files:
                cmd += ["--draw", f]
            if grid is not None:
                cmd += ["--grid", str(grid)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            for i in range(2):
                got = np.array(Image.open(os.path.join(out, "r_%d.png" % i)))
                assert got.shape == (H, W, 4) and np.array_equal(got, want[i]), (files, batch, i)
    r = subprocess.run([binary, "--help"], capture_output=True, text=True, timeout=60)
    assert "--draw" in r.stdout
