"""rto_launch_rays / volrend.render_rays: batches of arbitrary rays with a per-ray depth limit and backdrop.

The per-ray oracle here is the CPU oracle's orc_trace_ray (the march and shading of one ray, given tree-space dir / cen and the
view direction) plus a numpy restatement of what the frame path does around it: normalize3 of the direction, the NDC warp,
offset + scale * cen, the rot_dirs rotation of the view direction (the oracle applies it in its pixel harness only,
rto_oracle.c:530-548), the RNG jump of ray i to (first_ray + i) * spp and the composite over the backdrop.  The restatement is
itself pinned to orc_render_pixel on camera rays (CPU tests)."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import orc
import rt_octree_amd as R
from helpers import assert_bits_equal, rgba_tree
from rt_octree_amd import _lib, synth

E_INVALID, E_SPP, E_UNSUPPORTED, E_FORMAT = -1, -2, -3, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = C.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]


# ------------------------------------------------------------------ the per-ray oracle


def _trace_fn():
    L = orc.lib()
    fn = L.orc_trace_ray
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def _normalize3(d):
    with np.errstate(all="ignore"):
        n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        inv = f32(1) / n
        return d * inv[:, None]


def _rotate(vdir, rot_dirs):
    """rodrigues (volrend.cu:58-73) as the oracle's pixel harness evaluates it: float terms, the last one in double"""
    a = np.asarray(rot_dirs, f32)
    angle = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    if angle < 1e-6:
        return vdir
    k = a / angle
    cos, sin = f32(_libm.cosf(float(angle))), f32(_libm.sinf(float(angle)))
    v = vdir
    cross = np.stack([k[1] * v[:, 2] - k[2] * v[:, 1], k[2] * v[:, 0] - k[0] * v[:, 2], k[0] * v[:, 1] - k[1] * v[:, 0]], 1)
    dot = (k[0] * v[:, 0] + k[1] * v[:, 1]) + k[2] * v[:, 2]
    omc = 1.0 - np.float64(cos)
    out = np.empty_like(v)
    for i in range(3):
        head = (v[:, i] * cos + cross[:, i] * sin).astype(np.float64)
        out[:, i] = (head + (k[i] * dot).astype(np.float64) * omc).astype(f32)
    return out


def ray_setup(ht, origins, dirs, ndc=None):
    """what the frame path does to a ray before trace_ray: normalize3 of the direction, the NDC warp, cen = offset + scale * cen
    -> (dir, cen, vdir), float32 [n, 3] each; vdir is the unit direction before the warp (and before rot_dirs)"""
    origins = np.ascontiguousarray(origins, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    d = _normalize3(dirs)
    cen = origins.copy()
    vdir = d.copy()
    with np.errstate(all="ignore"):
        if ndc is not None:  # maybe_world2ndc (volrend.cu:35-56)
            w, h, focal = (f32(v) for v in ndc)
            t = -(f32(1) + cen[:, 2]) / d[:, 2]
            cen = cen + t[:, None] * d
            fw, fh = (f32(2) * focal) / w, (f32(2) * focal) / h
            d = np.stack([-fw * (d[:, 0] / d[:, 2] - cen[:, 0] / cen[:, 2]), -fh * (d[:, 1] / d[:, 2] - cen[:, 1] / cen[:, 2]),
                          f32(-2) / cen[:, 2]], 1)
            cen = np.stack([-fw * (cen[:, 0] / cen[:, 2]), -fh * (cen[:, 1] / cen[:, 2]), f32(1) + f32(2) / cen[:, 2]], 1)
            d = _normalize3(d)
        cen = ht.offset[None, :] + ht.scale[None, :] * cen
    return d, cen, vdir


def ray_oracle(ht, origins, dirs, spp, t_max=None, background=None, first_ray=0, bg=1.0, rng_base=None, ndc=None,
               draws=None, **optkw):
    """[n, 4] float32: what rto_launch_rays must return, ray by ray on the CPU.  draws: an int array [n] that receives the
    number of RNG draws each ray consumed"""
    origins = np.ascontiguousarray(origins, f32)
    n = origins.shape[0]
    opt = orc.default_options(spp=spp, background_brightness=bg, **optkw)
    d, cen, vdir = ray_setup(ht, origins, dirs, ndc)
    vdir = _rotate(vdir, optkw.get("rot_dirs", (0.0, 0.0, 0.0)))
    tm = np.full(n, 1e9, f32) if t_max is None else np.asarray(t_max, f32)
    back = np.full((n, 3), bg, f32) if background is None else np.asarray(background, f32)
    with np.errstate(invalid="ignore"):
        live = (tm > 0) & np.isfinite(d).all(1) & np.isfinite(cen).all(1) & (d != 0).any(1)
    d, cen, vdir = (np.ascontiguousarray(a, f32) for a in (d, cen, vdir))
    trace = _trace_fn()
    L = orc.lib()
    base = rng_base if rng_base is not None else orc.rng()
    out = np.zeros((n, 4), f32)
    o4 = (C.c_float * 4)()
    dbuf = (C.c_float * 3)()
    for i in np.flatnonzero(live):
        rng = orc.Pcg32(base.state, base.inc)
        delta = ((first_ray + int(i)) * spp) & 0xFFFFFFFFFFFFFFFF
        L.orc_pcg32_advance(C.byref(rng), delta - (1 << 64) if delta >= 1 << 63 else delta)
        dbuf[:] = d[i].tolist()
        o4[:] = [0.0] * 4
        rc = trace(C.byref(ht.c), dbuf, vdir[i].ctypes.data, cen[i].ctypes.data, C.byref(opt), float(tm[i]), o4, C.byref(rng), None)
        assert rc == 0
        out[i] = np.frombuffer(o4, f32)
        if draws is not None:
            k, probe = 0, orc.Pcg32(base.state, base.inc)
            L.orc_pcg32_advance(C.byref(probe), delta - (1 << 64) if delta >= 1 << 63 else delta)
            while probe.state != rng.state:
                L.orc_pcg32_next_uint(C.byref(probe))
                k += 1
                assert k <= spp
            draws[i] = k
    nalpha = f32(1) - out[:, 3]
    out[:, :3] += back * nalpha[:, None]
    return out


def _small(basis=9, seed=7, depth=6):
    return synth.make_tree(depth_limit=depth, basis_dim=basis, seed=seed)


def _cam(W, H, pose=1):
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(synth.orbit_poses(4)[pose])
    return cam


def _frame_planes(aux):
    return np.ascontiguousarray(aux[:4].reshape(4, -1).T)


# ------------------------------------------------------------------ CPU


def test_library_exports_rto_launch_rays():
    assert "rto_launch_rays" in _lib.SYMBOLS
    assert "int rto_launch_rays(" in open(os.path.join(ROOT, "include", "rto.h")).read()
    assert hasattr(R.lib(), "rto_launch_rays")


@pytest.mark.parametrize("rot", [None, (0.3, -0.2, 0.5)])
def test_ray_oracle_matches_the_pixel_oracle(rot):
    """camera_rays + the per-ray oracle == orc_render_pixel's aux planes 0..3 (with and without rot_dirs)"""
    t = _small()
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    cam = _cam(40, 30)
    kw = {} if rot is None else {"rot_dirs": rot}
    ocam = orc.camera(cam.width, cam.height, cam.fx, cam.fy, cam.transform.reshape(-1))
    aux, _, _ = orc.render_frame(ht, ocam, orc.default_options(spp=4, **kw), orc.rng(), want_stats=False)
    o, d = R.camera_rays(cam)
    got = ray_oracle(ht, o, d, 4, **kw)
    assert_bits_equal(got, _frame_planes(aux), "per-ray oracle vs pixel oracle")
    assert (got[:, 3] > 0).sum() > 100  # (the view holds the object)


def test_ray_oracle_matches_the_pixel_oracle_ndc():
    t = _small()
    ndc = (40.0, 30.0, 35.0)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)
    cam = _cam(40, 30)
    ocam = orc.camera(cam.width, cam.height, cam.fx, cam.fy, cam.transform.reshape(-1))
    aux, _, _ = orc.render_frame(ht, ocam, orc.default_options(spp=2), orc.rng(), want_stats=False)
    o, d = R.camera_rays(cam)
    assert_bits_equal(ray_oracle(ht, o, d, 2, ndc=ndc), _frame_planes(aux), "per-ray oracle vs pixel oracle (NDC)")


def test_camera_rays_layout():
    cam = _cam(7, 5)
    o, d = R.camera_rays(cam)
    assert o.shape == d.shape == (35, 3) and o.dtype == d.dtype == np.float32
    assert np.array_equal(o, np.broadcast_to(cam.transform[3], (35, 3)))
    m = cam.transform.reshape(-1)
    x, y = 3, 2  # pixel 17
    xyz = [(f32(x) - f32(0.5) * f32(7)) / f32(cam.fx), -(f32(y) - f32(0.5) * f32(5)) / f32(cam.fy), f32(-1)]
    want = [m[c] * xyz[0] + m[3 + c] * xyz[1] + m[6 + c] * xyz[2] for c in range(3)]
    assert np.array_equal(d[17], np.array(want, f32))


# bytes of scratch per lane recorded for render_rays (0 elsewhere): SPP 8 on the two-level image, and SPP 32 (render_fast<32> holds
# 32-160 too) -- so that a change of them is a decision, not an accident
RAYS_SCRATCH = {(8, 1): 8, (32, 1): 132, (32, 0): 136}


def test_rays_kernels_codegen():
    """every render_rays instantiation exists, keeps no private segment up to SPP 16 (see RAYS_SCRATCH) and reaches the waves
    per SIMD render_fast is built for; render_rays_generic keeps render_generic's private segment and all but one of its waves"""
    import shutil
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to cross-compile the kernels")
    from test_codegen import render_resources
    res = render_resources()
    for spp in (1, 2, 3, 4, 6, 8, 16, 32):
        fast = [v["occupancy"] for n, v in res.items() if n.startswith("_ZN3rto11render_fastILi%dELb0ELb1ELi" % spp)]
        assert len(fast) == 2, spp
        target = 5 if spp <= 8 else 4  # (the waves per SIMD both kernels are built for: RTO_FAST_WPS, 4 above SPP 8)
        for lobes in (0, 2, 3):
            for wide, stack in ((1, 1), (1, 0), (0, 0)):
                pre = "_ZN3rto11render_raysILi%dELb%dELi%dELi%dEEEvNS_7TreeDevENS_6OptDevENS_5Pcg32EPKNS_12PcgJumpEntryENS_8RayBatchE" % (
                    spp, wide, stack, lobes)
                assert pre in res, pre
                k = res[pre]
                assert k["scratch"] <= RAYS_SCRATCH.get((spp, wide), 0), (pre, k)
                assert k["occupancy"] >= min(target, min(fast)), (pre, k, fast)
        g = [v for n, v in res.items() if n.startswith("_ZN3rto19render_rays_genericILi%dEEE" % spp)]
        frame = [v for n, v in res.items() if n.startswith("_ZN3rto14render_genericILi%dEEE" % spp)]
        assert len(g) == 1 and len(frame) == 1
        # (three VGPRs more than render_generic -- the ray's loads and backdrop -- cost it one wave at SPP 3 and 32)
        assert g[0]["scratch"] <= frame[0]["scratch"] and g[0]["occupancy"] >= frame[0]["occupancy"] - 1, (spp, g, frame)


# ------------------------------------------------------------------ GPU


def _tree(kind, basis):
    t = _small(basis=basis if kind != "RGBA" else 9, seed=7)
    if kind == "RGBA":
        t = rgba_tree(t)
    elif kind in ("SG", "ASG"):
        t = synth.with_lobes(t, kind, seed=3)
    return t


def _dev(t, **kw):
    return R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format, extra_data=t.extra, **kw)


def _camera_equivalence(dt, cam, spp, kernel, **optkw):
    ctx = R.RenderContext(cam.width, cam.height)
    ctx.rng_seed()
    ctx.rng_advance()  # (a frame other than the first)
    ctx.set_kernel(kernel)
    opt = R.RenderOptions(spp=spp, denoise=False, **optkw)
    R.launch_renderer(dt, cam, opt, ctx)
    aux = ctx.download_aux()
    o, d = R.camera_rays(cam)
    got = R.render_rays(dt, o, d, opt, ctx).cpu().numpy()
    assert_bits_equal(got, _frame_planes(aux), "render_rays vs launch_renderer (spp %d, kernel %d)" % (spp, kernel))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind,basis", [("RGBA", -1), ("SH", 9), ("SH", 16), ("SG", 16), ("ASG", 16)])
@pytest.mark.parametrize("spp", [1, 6, 32])
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_camera_equivalence(kind, basis, spp, kernel):
    dt = _dev(_tree(kind, basis))
    got = _camera_equivalence(dt, _cam(72, 40), spp, kernel)
    assert (got[:, 3] > 0).sum() > 200


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_camera_equivalence_options_and_ndc(kernel):
    t = _small(basis=16, seed=11)
    dt = _dev(t)
    cam = _cam(64, 48, pose=2)
    _camera_equivalence(dt, cam, 6, kernel, rot_dirs=[0.4, -0.3, 0.9])
    _camera_equivalence(dt, cam, 4, kernel, render_bbox=[0.1, 0.0, 0.2, 0.9, 0.8, 1.0], basis_minmax=[1, 6])
    ndc = _dev(t)
    ndc.set_ndc(64.0, 48.0, 40.0)
    _camera_equivalence(ndc, cam, 6, kernel)


@pytest.mark.gpu
def test_fast_and_generic_kernels_agree_on_the_one_level_image_and_on_a_deep_tree():
    """the traversal images the default small tree does not take (it walks the two-level image with the register stack): the
    one-level image (WIDE = false) and a tree deep enough to keep its ancestor stack in LDS rows (STACK == 0) -- render_rays
    returns the generic kernel's bits on both"""
    from helpers import cameras
    from test_render_parity import _chain_tree

    def both(dt, cam, tuning=()):
        o, d = R.camera_rays(cam)
        bg = np.random.default_rng(2).uniform(0, 1, o.shape).astype(f32)
        out = []
        for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
            ctx = R.RenderContext(8, 8)
            ctx.rng_seed()
            ctx.set_kernel(kernel)
            for k, v in tuning:
                ctx.set_tuning(k, v)
            out.append(R.render_rays(dt, o, d, R.RenderOptions(spp=6), ctx, background=bg, first_ray=77).cpu().numpy())
        assert_bits_equal(out[0], out[1], "render_rays, fast vs generic")
        assert (out[0][:, 3] > 0).sum() >= 100
    # (slot-ordered records: a tree whose records follow the two-level image's entries has no one-level fallback; 2^6 entries:
    #  nothing fits, the launch takes the WIDE = false instantiation)
    both(_dev(_tree("SH", 9), compact_records=True), _cam(64, 48), tuning=(("wide_bits", 6),))
    deep = _dev(_chain_tree(13, seed=13))  # four pairs of levels below the grid
    assert (deep.max_depth - 6 + 1) // 2 > 2 and deep.wide_nodes > 0
    both(deep, cameras(56, 40, synth.look_at_c2w((2.2, 1.7, 1.9), target=(0.0, -0.1, 0.05)))[1])


def _world(t, p):
    """tree-space points -> world space (cen = offset + scale * world)"""
    return ((p - t.offset[None, :]) / t.scale[None, :]).astype(f32)


def _mixed_rays(t, n, seed):
    """origins inside and outside the box, random / axis-aligned / zero-component directions, rays that graze the faces"""
    rng = np.random.default_rng(seed)
    q = n // 4
    o = rng.uniform(-0.6, 1.6, (n, 3)).astype(f32)
    o[:q] = rng.uniform(0.05, 0.95, (q, 3))  # inside
    d = rng.normal(size=(n, 3)).astype(f32) * rng.uniform(0.1, 10.0, (n, 1)).astype(f32)
    axes = np.eye(3, dtype=f32)[rng.integers(0, 3, q)] * rng.choice([-1.0, 1.0], (q, 1)).astype(f32)
    d[q:2 * q] = axes
    zc = d[2 * q:3 * q].copy()
    zc[np.arange(q), rng.integers(0, 3, q)] = 0.0
    d[2 * q:3 * q] = zc
    # grazing: origin on a face plane (or just off it), direction inside that plane
    g = slice(3 * q, n)
    m = n - 3 * q
    ax = rng.integers(0, 3, m)
    face = rng.choice([0.0, 1.0, 1e-6, 1.0 - 1e-6], m).astype(f32)
    o[g][np.arange(m), ax] = face
    og = o[g].copy()
    og[np.arange(m), ax] = face
    o[g] = og
    dg = d[g].copy()
    dg[np.arange(m), ax] = 0.0
    d[g] = dg
    d[(d == 0).all(1)] = np.array([1.0, 0.0, 0.0], f32)
    return _world(t, o), d


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_arbitrary_rays_match_the_oracle(kernel):
    t = _small(basis=9, seed=7)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    dt = _dev(t)
    n = 200_000 if kernel == R.KERNEL_FAST else 40_000
    o, d = _mixed_rays(t, n, seed=1)
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    ctx.set_kernel(kernel)
    got = R.render_rays(dt, o, d, R.RenderOptions(spp=2), ctx, first_ray=12345).cpu().numpy()
    want = ray_oracle(ht, o, d, 2, first_ray=12345)
    assert_bits_equal(got, want, "render_rays vs the per-ray oracle")
    assert (want[:, 3] > 0).sum() > n // 20


@pytest.mark.gpu
def test_t_max_and_degenerate_rays():
    t = _small(basis=16, seed=11)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    dt = _dev(t)
    rng = np.random.default_rng(4)
    o, d = _mixed_rays(t, 40_000, seed=2)
    world_size = float(1.0 / t.scale[0])
    tm = rng.uniform(0.0, 1.5 * world_size, o.shape[0]).astype(f32)  # (many end inside a leaf)
    tm[::7] = np.inf
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    opt = R.RenderOptions(spp=6)
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx.set_kernel(kernel)
        got = R.render_rays(dt, o, d, opt, ctx, t_max=tm).cpu().numpy()
        assert_bits_equal(got, ray_oracle(ht, o, d, 6, t_max=tm), "t_max vs the oracle's tmax_bg")
        full = R.render_rays(dt, o, d, opt, ctx).cpu().numpy()
        assert_bits_equal(R.render_rays(dt, o, d, opt, ctx, t_max=np.full(o.shape[0], 1e9, f32)).cpu().numpy(), full, "1e9 == NULL")
        assert (got[:, 3] != full[:, 3]).sum() > 100
    # degenerate rays: the backdrop with alpha 0
    inside = _world(t, np.full((1, 3), 0.5, f32))[0]
    bad_o = np.tile(inside, (9, 1))
    bad_d = np.tile(np.array([0.3, -0.2, 1.0], f32), (9, 1))
    bad_t = np.full(9, 5.0, f32)
    bad_d[0] = 0.0
    bad_d[1, 1] = np.nan
    bad_d[2, 0] = np.inf
    bad_o[3, 2] = np.nan
    bad_o[4, 0] = -np.inf
    bad_t[5] = 0.0
    bad_t[6] = -1.0
    bad_t[7] = np.nan
    bad_d[8] = 1e-30  # (its squared length underflows)
    bg = np.random.default_rng(1).uniform(0, 1, (9, 3)).astype(f32)
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx.set_kernel(kernel)
        got = R.render_rays(dt, bad_o, bad_d, opt, ctx, t_max=bad_t, background=bg).cpu().numpy()
        assert_bits_equal(got, np.concatenate([bg, np.zeros((9, 1), f32)], 1), "degenerate rays")


@pytest.mark.gpu
def test_backdrop():
    t = _small(basis=9, seed=7)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    dt = _dev(t)
    o, d = _mixed_rays(t, 30_000, seed=3)
    bg = np.random.default_rng(5).uniform(0, 2, o.shape).astype(f32)
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx.set_kernel(kernel)
        got = R.render_rays(dt, o, d, R.RenderOptions(spp=3), ctx, background=bg).cpu().numpy()
        assert_bits_equal(got, ray_oracle(ht, o, d, 3, background=bg), "per-ray backdrop")
        plain = R.render_rays(dt, o, d, R.RenderOptions(spp=3, background_brightness=0.25), ctx).cpu().numpy()
        same = R.render_rays(dt, o, d, R.RenderOptions(spp=3), ctx, background=np.full(o.shape, 0.25, f32)).cpu().numpy()
        assert_bits_equal(same, plain, "(b, b, b) == NULL")


@pytest.mark.gpu
def test_chunking_and_repeatability():
    import torch
    t = _small(basis=9, seed=7)
    dt = _dev(t)
    o, d = _mixed_rays(t, 50_000, seed=6)
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    opt = R.RenderOptions(spp=6)
    first = 3 << 30  # first_ray * spp > 2^32
    whole = R.render_rays(dt, o, d, opt, ctx, first_ray=first).cpu().numpy()
    assert_bits_equal(R.render_rays(dt, o, d, opt, ctx, first_ray=first).cpu().numpy(), whole, "repeat")
    parts = []
    for a, b in ((0, 1), (1, 300), (300, 20_001), (20_001, 50_000)):
        parts.append(R.render_rays(dt, o[a:b], d[a:b], opt, ctx, first_ray=first + a).cpu().numpy())
    assert_bits_equal(np.concatenate(parts), whole, "chunked calls")
    # n = 0: nothing launched, an empty result
    assert R.render_rays(dt, o[:0], d[:0], opt, ctx).shape == (0, 4)
    # ctx.rng is not modified
    s0 = ctx.rng_get()
    R.render_rays(dt, o[:10], d[:10], opt, ctx)
    torch.cuda.synchronize()
    assert ctx.rng_get() == s0


@pytest.mark.gpu
def test_a_batch_above_the_per_launch_limit_is_split():
    """spp 32: more than 2^32 / 32 rays in one call -- split into launches whose RNG offsets continue exactly"""
    import torch
    t = _small(basis=9, seed=7)
    dt = _dev(t)
    spp = 32
    per_launch = ((0xFFFFFFFF // spp) - 4096) & ~255
    n = per_launch + 8192
    assert n * spp > 1 << 32
    dev = torch.device("cuda", 0)
    # every ray misses (behind the box, pointing away) except a window across the launch boundary
    origins = torch.empty((n, 3), dtype=torch.float32, device=dev)
    origins[:] = torch.as_tensor(_world(t, np.array([[-3.0, 0.5, 0.5]], f32)), device=dev)
    dirs = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    dirs[:, 0] = -1.0
    w0, w1 = per_launch - 1500, per_launch + 1500
    wo, wd = _mixed_rays(t, w1 - w0, seed=8)
    origins[w0:w1] = torch.as_tensor(wo, device=dev)
    dirs[w0:w1] = torch.as_tensor(wd, device=dev)
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    opt = R.RenderOptions(spp=spp)
    out = R.render_rays(dt, origins, dirs, opt, ctx, first_ray=7)
    window = R.render_rays(dt, origins[w0:w1].contiguous(), dirs[w0:w1].contiguous(), opt, ctx, first_ray=7 + w0)
    assert_bits_equal(out[w0:w1].cpu().numpy(), window.cpu().numpy(), "across the launch boundary")
    assert (window[:, 3] > 0).sum().item() > 100
    tail = out[-10:].cpu().numpy()
    assert np.array_equal(tail, np.tile(np.array([1, 1, 1, 0], f32), (10, 1)))  # (the last launch ran)
    del out, origins, dirs
    torch.cuda.empty_cache()


def _launch(tree_h, rays, opt, ctx_h, out):
    return R.lib().rto_launch_rays(tree_h, rays, C.byref(opt.to_c()), ctx_h, out, None)


@pytest.mark.gpu
def test_refusals(tmp_path):
    import torch
    t = _small(basis=9, seed=7)
    dt = _dev(t)
    ctx = R.RenderContext(8, 8)
    o = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    d = torch.ones((4, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((5, 4), dtype=torch.float32, device="cuda")
    opt = R.RenderOptions(spp=1)

    def rays(n=4, first=0, origins=True, dirs=True):
        r = _lib.CRays()
        r.origins = o.data_ptr() if origins else None
        r.dirs = d.data_ptr() if dirs else None
        r.n, r.first_ray = n, first
        return C.byref(r)

    op = C.c_void_p(out.data_ptr())
    assert _launch(dt._h, rays(), opt, ctx._h, op) == 0
    assert _launch(None, rays(), opt, ctx._h, op) == E_INVALID
    assert _launch(dt._h, None, opt, ctx._h, op) == E_INVALID
    assert R.lib().rto_launch_rays(dt._h, rays(), None, ctx._h, op, None) == E_INVALID
    assert _launch(dt._h, rays(), opt, None, op) == E_INVALID
    assert _launch(dt._h, rays(), opt, ctx._h, None) == E_INVALID
    assert _launch(dt._h, rays(n=-1), opt, ctx._h, op) == E_INVALID
    assert _launch(dt._h, rays(first=-1), opt, ctx._h, op) == E_INVALID
    assert _launch(dt._h, rays(origins=False), opt, ctx._h, op) == E_INVALID
    assert _launch(dt._h, rays(dirs=False), opt, ctx._h, op) == E_INVALID
    assert _launch(dt._h, rays(n=0, origins=False, dirs=False), opt, ctx._h, op) == 0
    assert _launch(dt._h, rays(), opt, ctx._h, C.c_void_p(out.data_ptr() + 4)) == E_INVALID
    assert _launch(dt._h, rays(), R.RenderOptions(spp=5), ctx._h, op) == E_SPP
    assert _launch(dt._h, rays(), R.RenderOptions(spp=1, enable_probe=True), ctx._h, op) == E_UNSUPPORTED
    sg = synth.with_lobes(_small(basis=9, seed=7, depth=4), "SG", seed=2)
    bare = R.N3Tree.from_arrays(sg.child, sg.data, sg.scale, sg.offset, sg.data_format)  # (no lobes)
    assert _launch(bare._h, rays(), opt, ctx._h, op) == E_FORMAT
    path = str(tmp_path / "quant.npz")
    _small(basis=9, seed=11).save_quant_npz(path, n_retain=1, quantiser="luminance")
    q = R.N3Tree(path, quant_direct=True)
    assert _launch(q._h, rays(), opt, ctx._h, op) == E_UNSUPPORTED
    with pytest.raises(R.RtoError) as e:
        R.render_rays(q, o, d, opt, ctx)
    assert e.value.code == E_UNSUPPORTED
    torch.cuda.synchronize()
