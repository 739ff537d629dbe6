"""rto_ctx_set_layers / RenderContext.set_layers: frames composited over a depth and a colour layer (the operator's
offscreen = false; volrend.cu:146-153,162-184).

A layered frame is DEFINED by rto_launch_rays: pixel (x, y) is ray y * W + x of the camera's rays with t_max = its depth,
background = its colour's rgb and the frame's RNG base; aux planes 0..3 are those (r, g, b, alpha), planes 4..7 their squares, the
image (r, g, b, 1).  Everything below is bit for bit.  The CPU expectation is test_rays.ray_oracle (layers_ref.expected_rgba)."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import orc
import rt_octree_amd as R
from helpers import assert_bits_equal
from layers_ref import expected_rgba, frame_outputs, make_layers
from rt_octree_amd import _lib, synth
from test_rays import _cam, _dev, _frame_planes, _small, _tree

E_INVALID, E_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 100, 76  # (not multiples of 8)


def _host(t, **kw):
    return orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, **kw)


def _cams(n, w=W, h=H):
    fx = synth.blender_focal(w)
    out = []
    for p in synth.orbit_poses(max(n, 4))[:n]:
        c = R.Camera(w, h, fx, fx)
        c.set_c2w(p)
        out.append(c)
    return out


# ------------------------------------------------------------------ CPU


def test_library_exports_the_layer_functions():
    hdr = open(os.path.join(ROOT, "include", "rto.h")).read()
    for name in ("rto_ctx_set_layers", "rto_ctx_layers"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in hdr
        assert hasattr(R.lib(), name)
    assert hasattr(R.RenderContext, "set_layers")


def test_trivial_layers_give_the_pixel_oracle():
    """depth 1e9 and colour = the background brightness: the layered expectation is orc_render_pixel's frame"""
    t = _small()
    ht = _host(t)
    cam = _cam(40, 30)
    ocam = orc.camera(cam.width, cam.height, cam.fx, cam.fy, cam.transform.reshape(-1))
    aux, rgba, _ = orc.render_frame(ht, ocam, orc.default_options(spp=4, background_brightness=0.75), orc.rng(frame=1), want_stats=False)
    depth = np.full((30, 40), 1e9, f32)
    color = np.full((30, 40, 4), 0.75, f32)
    got = expected_rgba(ht, cam, 4, depth, color, rng_base=orc.rng(frame=1), bg=0.25)  # (bg is unread under a colour layer)
    assert_bits_equal(got, _frame_planes(aux), "layered expectation vs the pixel oracle")
    e_aux, e_img = frame_outputs(got, 30, 40)
    assert_bits_equal(e_aux, aux, "all 8 planes")
    assert_bits_equal(e_img, rgba, "image")


def _bite(off, lay):
    """the fixture assertions on (r, g, b, alpha) [H*W, 4] of the offscreen and the layered render of one pose"""
    inside = off[:, 3] > 0
    assert inside.sum() > 500
    changed = (off.view(np.uint32) != lay.view(np.uint32)).any(1)
    assert (changed & inside).sum() * 10 >= inside.sum(), ((changed & inside).sum(), inside.sum())
    assert ((lay[:, 3] > 0) & (lay[:, 3] < off[:, 3])).sum() > 20


def test_the_fixture_bites_on_the_oracle():
    """the layers of the GPU tests change the frame (CPU oracle): a tenth of the silhouette and more, partly covered pixels"""
    t = _small()
    ht = _host(t)
    cams = _cams(2)
    depth, color = make_layers(t, cams)
    for f in (0, 1):
        off = expected_rgba(ht, cams[f], 2)
        lay = expected_rgba(ht, cams[f], 2, depth[f], color[f])
        _bite(off, lay)
        dead = ~(depth[f].reshape(-1) > 0)  # 0, negative, NaN: the backdrop, alpha 0
        assert dead.sum() > 100 and (dead & (off[:, 3] > 0)).sum() > 5
        assert_bits_equal(lay[dead], np.concatenate([color[f].reshape(-1, 4)[dead, :3], np.zeros((dead.sum(), 1), f32)], 1), "dead depth")


def test_layers_kernels_codegen():
    """every layered kernel exists in the gfx950 code object, holds no private segment where its parent holds none, reaches the
    waves per SIMD it is built for (or its parent's, where that is fewer), and no kernel of the file holds v_pk_fma_f32"""
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to cross-compile the kernels")
    from test_codegen import render_asm, render_resources
    res = render_resources()
    assert "v_pk_fma_f32" not in render_asm()

    def pair(parent_prefix, layered_prefix, target, slack=0):
        """target: the waves per SIMD the kernel is built for (its launch bounds); the layered form may hold a few VGPRs more
        (the pixel's depth, its backdrop) as long as it reaches min(parent, target) - slack"""
        p = [v for n, v in res.items() if n.startswith(parent_prefix)]
        l = [v for n, v in res.items() if n.startswith(layered_prefix)]
        assert len(p) == 1 and len(l) == 1, (parent_prefix, len(p), layered_prefix, len(l))
        a, b = p[0], l[0]
        if a["scratch"] == 0:
            assert b["scratch"] == 0, (layered_prefix, a, b)
        assert b["occupancy"] >= min(a["occupancy"], target) - slack, (layered_prefix, a, b)

    for spp in (1, 2, 3, 4, 6, 8, 16, 32):
        fast_wps = 5 if spp <= 8 else 4  # RTO_FAST_WPS, 4 above SPP 8
        for wide, stack in ((1, 1), (1, 0), (0, 0)):
            pair("_ZN3rto11render_fastILi%dELb0ELb%dELi%dEEE" % (spp, wide, stack),
                 "_ZN3rto18render_fast_layersILi%dELb%dELi%dELi0EEE" % (spp, wide, stack), fast_wps)
            for lobes in (2, 3):
                pair("_ZN3rto17render_fast_lobesILi%dELb0ELb%dELi%dELi%dEEE" % (spp, wide, stack, lobes),
                     "_ZN3rto18render_fast_layersILi%dELb%dELi%dELi%dEEE" % (spp, wide, stack, lobes), fast_wps)
            pair("_ZN3rto14render_persistILi%dELi32ELi8ELb%dELi%dEEE" % (spp, wide, stack),
                 "_ZN3rto21render_persist_layersILi%dELi32ELi8ELb%dELi%dEEE" % (spp, wide, stack), 8)  # RTO_WPS_DEFAULT
        # (no launch-bounds target: three VGPRs more than render_generic may cost one wave, as render_rays_generic)
        pair("_ZN3rto14render_genericILi%dEEE" % spp, "_ZN3rto21render_generic_layersILi%dEEE" % spp, 8, slack=1)
        sp = 2 if spp <= 8 else 1
        for lobes in (0, 2, 3):
            for mode in (0, 28, 49, 76):
                pair("_ZN3rto12shade_kernelILi%dELi%dELi%dELi%dEEE" % (spp, sp, mode, lobes),
                     "_ZN3rto19shade_kernel_layersILi%dELi%dELi%dELi%dEEE" % (spp, sp, mode, lobes), 3 if mode == 76 else 4)  # shade_wps
    # the layered batched kernels exist for the default tuning only
    assert not [n for n in res if n.startswith("_ZN3rto21render_persist_layersILi6ELi24E")]


# ------------------------------------------------------------------ GPU

torch = None


def _torch():
    global torch
    if torch is None:
        import torch as _t
        torch = _t
    return torch


def _dev_layers(depth, color):
    t = _torch()
    d = None if depth is None else t.from_numpy(np.ascontiguousarray(depth, f32)).cuda()
    c = None if color is None else t.from_numpy(np.ascontiguousarray(color, f32)).cuda()
    return d, c


def _rays_of(dt, cam, opt, ctx, depth, color):
    """render_rays on the camera's rays with the layer values (the definition of a layered frame); ctx supplies the RNG base"""
    o, d = R.camera_rays(cam)
    tm = None if depth is None else np.ascontiguousarray(depth, f32).reshape(-1)
    bg = None if color is None else np.ascontiguousarray(np.asarray(color, f32).reshape(-1, 4)[:, :3])
    return R.render_rays(dt, o, d, opt, ctx, t_max=tm, background=bg).cpu().numpy()


def _check_frame(aux, image, rgba, what):
    e_aux, e_img = frame_outputs(rgba, aux.shape[1], aux.shape[2])
    assert_bits_equal(aux[:4], e_aux[:4], what + ": aux planes 0..3")
    assert_bits_equal(aux[4:], aux[:4] * aux[:4], what + ": planes 4..7 are the squares")
    assert_bits_equal(image, e_img, what + ": image (r, g, b, 1)")


def _single(dt, ht, cam, spp, kernel, depth, color, ndc=None, **optkw):
    """one layered single-frame launch checked against render_rays and the CPU oracle (ht = None: an SG / ASG tree, whose lobes the
    C oracle does not evaluate -- render_rays on it is pinned in test_rays.py / test_sg_asg.py); -> its (r, g, b, alpha)"""
    ctx = R.RenderContext(cam.width, cam.height)
    ctx.rng_seed()
    ctx.rng_advance()
    ctx.set_kernel(kernel)
    d, c = _dev_layers(depth[None], color[None])
    ctx.set_layers(d, c)
    opt = R.RenderOptions(spp=spp, denoise=False, **optkw)
    R.launch_renderer(dt, cam, opt, ctx, offscreen=False)
    aux, image = ctx.download_aux(), ctx.download_image()
    rays = _rays_of(dt, cam, opt, ctx, depth, color)
    _check_frame(aux, image, rays, "vs render_rays (spp %d, kernel %d)" % (spp, kernel))
    if ht is not None:
        want = expected_rgba(ht, cam, spp, depth, color, rng_base=orc.rng(frame=1), ndc=ndc, **optkw)
        assert_bits_equal(rays, want, "vs the per-ray oracle (spp %d, kernel %d)" % (spp, kernel))
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("kind,basis", [("SH", 9), ("SH", 16), ("RGBA", -1), ("SG", 16), ("ASG", 16)])
@pytest.mark.parametrize("spp", [1, 6, 32])
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_single_frame_equals_rays_and_oracle(kind, basis, spp, kernel):
    t = _tree(kind, basis)
    ht = None if kind in ("SG", "ASG") else _host(t)
    dt = _dev(t)
    cam = _cams(2)[1]
    depth, color = make_layers(t, _cams(2))
    lay = _single(dt, ht, cam, spp, kernel, depth[1], color[1])
    if spp == 6:  # the fixture bites: against the offscreen render of the same pose
        ctx = R.RenderContext(W, H)
        ctx.rng_seed()
        ctx.rng_advance()
        ctx.set_kernel(kernel)
        R.launch_renderer(dt, cam, R.RenderOptions(spp=spp, denoise=False), ctx)
        _bite(_frame_planes(ctx.download_aux()), lay)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_single_frame_rot_dirs_and_ndc(kernel):
    t = _small(basis=16, seed=11)
    cams = _cams(3)
    depth, color = make_layers(t, cams)
    _single(_dev(t), _host(t), cams[2], 6, kernel, depth[2], color[2], rot_dirs=[0.4, -0.3, 0.9])
    ndc = (float(W), float(H), 80.0)
    nd = _dev(t)
    nd.set_ndc(*ndc)
    _single(nd, _host(t, ndc=ndc), cams[2], 6, kernel, depth[2], color[2], ndc=ndc)


@pytest.mark.gpu
@pytest.mark.parametrize("cull_single", [0, 1])
def test_single_frame_with_tile_culling(cull_single):
    """tuning cull_single: a tile skipped by the marks writes its pixels' backdrop colour, alpha 0 -- same frame either way"""
    t = _small()
    dt = _dev(t)
    cam = _cams(2)[1]
    depth, color = make_layers(t, _cams(2))
    ctx = R.RenderContext(W, H)
    ctx.rng_seed()
    ctx.set_tuning("cull_single", cull_single)
    ctx.set_layers(*_dev_layers(depth[1][None], color[1][None]))
    opt = R.RenderOptions(spp=6, denoise=False)
    R.launch_renderer(dt, cam, opt, ctx)
    _check_frame(ctx.download_aux(), ctx.download_image(), _rays_of(dt, cam, opt, ctx, depth[1], color[1]), "cull_single %d" % cull_single)
    assert ctx.tile_marks() is None  # (a colour layer: the marks' promise does not hold)


def _marks_of(ctx, n):
    """[n][tiles_y][tiles_x] bool: the tile marks the last batched launch left"""
    t = _torch()
    ptr, words, _s0, frames, _bg = ctx.tile_marks()
    raw = t.as_tensor(R.volrend._DevArray(ptr, (frames * words,), ctx), device="cuda:0").view(t.int32).cpu().numpy().view(np.uint32)
    raw = raw.reshape(frames, words)[:n]
    tx, ty = (ctx.width + 7) // 8, (ctx.height + 7) // 8
    bits = ((raw[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(n, -1)[:, :tx * ty].astype(bool)
    keep_all = (raw[:, -1] & 1).astype(bool)
    return (bits | keep_all[:, None]).reshape(n, ty, tx)


def _batch(dt, cams, opt, jumps, depth, color, lean=0, cull=1, frames=None):
    n = len(cams)
    ctx = R.RenderContext(W, H, frames=frames or n)
    ctx.rng_seed()
    ctx.set_tuning("cull", cull)
    ctx.set_lean_outputs(lean)
    ctx.set_layers(*_dev_layers(depth, color))
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=jumps)
    _torch().cuda.synchronize()
    return ctx


def _views(ctx, n):
    t = _torch()
    return tuple(t.as_tensor(v, device="cuda:0")[:n] for v in ctx.batch_views())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,basis,spp", [("SH", 9, 6), ("SH", 16, 1), ("RGBA", -1, 6), ("SG", 16, 6), ("ASG", 9, 6), ("SH", 9, 32)])
def test_batched_launch(kind, basis, spp):
    t = _tree(kind, basis)
    dt = _dev(t)
    n = 5
    cams = _cams(n)
    jumps = [7, 3, 11, 0, 5]
    depth, color = make_layers(t, cams)
    opt = R.RenderOptions(spp=spp, denoise=False)
    ctx = _batch(dt, cams, opt, jumps, depth, color)
    aux, _noisy, image = (v.cpu().numpy() for v in _views(ctx, n))
    one = R.RenderContext(W, H, frames=n)
    one.set_layers(*_dev_layers(depth, color))
    culled_backdrops = 0
    for f in range(n):
        one.select_frame(f)  # (slot f reads plane f)
        one.rng_seed()
        one.rng_advance(jumps[f] << 32)
        R.launch_renderer(dt, cams[f], opt, one)
        assert_bits_equal(aux[f], one.download_aux(), "batch frame %d vs the layered single-frame launch" % f)
        assert_bits_equal(image[f], one.download_image(), "batch frame %d image" % f)
        _check_frame(aux[f], image[f], _rays_of(dt, cams[f], opt, one, depth[f], color[f]), "batch frame %d" % f)
    # the same frames with culling off
    off = _batch(dt, cams, opt, jumps, depth, color, cull=0)
    a2, _n2, i2 = (v.cpu().numpy() for v in _views(off, n))
    assert_bits_equal(a2, aux, "cull off: aux")
    assert_bits_equal(i2, image, "cull off: image")
    # lean level 1: (r, g, b, alpha) in the noisy image
    dn = R.RenderOptions(spp=spp, denoise=True)
    lean = _batch(dt, cams, dn, jumps, depth, color, lean=1)
    noisy = _views(lean, n)[1].cpu().numpy()
    assert_bits_equal(np.ascontiguousarray(noisy.transpose(0, 3, 1, 2)), aux[:, :4], "lean level 1 vs aux planes 0..3")
    # some culled tiles carry a non-constant backdrop (marks of a depth-only launch of the same poses)
    dctx = _batch(dt, cams, opt, jumps, depth, None)
    marks = _marks_of(dctx, n)
    for f in range(n):
        for ty, tx in zip(*np.nonzero(~marks[f])):
            tile = aux[f][:3, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            assert (aux[f][3, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] == 0).all()
            culled_backdrops += int(tile.min() != tile.max())
    assert culled_backdrops > 10


@pytest.mark.gpu
def test_layered_kernels_on_the_one_level_image_and_on_a_deep_tree():
    """the traversal images the default small tree does not take (it walks the two-level image with the register stack): the
    one-level image (WIDE = false) and a tree deep enough to keep its ancestor stack in LDS rows (STACK == 0) -- the layered
    single-frame fast kernel and the layered batch (render_persist_layers, shade_kernel_layers) give the layered generic kernel's
    frames, bit for bit"""
    from helpers import cameras
    from test_render_parity import _chain_tree

    def check(t, dt, cams, tuning=()):
        n, w, h = len(cams), cams[0].width, cams[0].height
        depth, color = make_layers(t, cams)
        opt = R.RenderOptions(spp=6, denoise=False)
        jumps = [4, 1]
        for with_color in (True, False):
            layers = _dev_layers(depth, color if with_color else None)
            bctx = R.RenderContext(w, h, frames=n)
            one = R.RenderContext(w, h, frames=n)
            for ctx in (bctx, one):
                for k, v in tuning:
                    ctx.set_tuning(k, v)
                ctx.set_layers(*layers)
            bctx.rng_seed()
            R.launch_renderer_batch(dt, cams, opt, bctx, rng_jumps=jumps)
            assert (bctx.tile_marks() is not None) == (not with_color)  # (depth only: the marks of the batched kernels)
            for f in range(n):
                outs = []
                for kernel in (R.KERNEL_GENERIC, R.KERNEL_FAST):
                    one.select_frame(f)
                    one.rng_seed()
                    one.rng_advance(jumps[f] << 32)
                    one.set_kernel(kernel)
                    R.launch_renderer(dt, cams[f], opt, one)
                    outs.append((one.download_aux(), one.download_image()))
                bctx.select_frame(f)
                outs.append((bctx.download_aux(), bctx.download_image()))
                for (aux, image), what in zip(outs[1:], ("fast", "batched")):
                    assert_bits_equal(aux, outs[0][0], "%s vs generic, colour %d, frame %d: aux" % (what, with_color, f))
                    assert_bits_equal(image, outs[0][1], "%s vs generic, colour %d, frame %d: image" % (what, with_color, f))
                assert (outs[0][0][3] > 0).sum() >= 50, f

    # (slot-ordered records: a tree whose records follow the two-level image's entries has no one-level fallback; 2^6 entries:
    #  nothing fits, the launches take the WIDE = false instantiations)
    t = _tree("SH", 9)
    check(t, _dev(t, compact_records=True), _cams(2, 60, 44), tuning=(("wide_bits", 6),))
    deep = _chain_tree(13, seed=13)  # four pairs of levels below the grid
    dt = _dev(deep)
    assert (dt.max_depth - 6 + 1) // 2 > 2 and dt.wide_nodes > 0
    check(deep, dt, [cameras(56, 40, synth.look_at_c2w(eye, target=(0.0, -0.1, 0.05)))[1] for eye in ((2.2, 1.7, 1.9), (2.0, 1.9, 1.7))])


@pytest.mark.gpu
def test_plane_selection():
    """slot k reads plane k: slot 2 of a 4-slot context rendered alone"""
    t = _small()
    dt = _dev(t)
    cams = _cams(4)
    depth, color = make_layers(t, cams)
    ctx = R.RenderContext(W, H, frames=4)
    ctx.set_layers(*_dev_layers(depth, color))
    ctx.select_frame(2)
    ctx.rng_seed()
    opt = R.RenderOptions(spp=6, denoise=False)
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx.set_kernel(kernel)
        R.launch_renderer(dt, cams[2], opt, ctx)
        _check_frame(ctx.download_aux(), ctx.download_image(), _rays_of(dt, cams[2], opt, ctx, depth[2], color[2]), "slot 2, kernel %d" % kernel)
    ctx.set_kernel(R.KERNEL_AUTO)
    ctx.set_tuning("frame_via_batch", 1)  # (the single frame as a batch of one into slot 2)
    R.launch_renderer(dt, cams[2], opt, ctx)
    _check_frame(ctx.download_aux(), ctx.download_image(), _rays_of(dt, cams[2], opt, ctx, depth[2], color[2]), "slot 2 via the batched path")
    assert not np.array_equal(depth[2], depth[1])


@pytest.mark.gpu
def test_trivial_layers_reproduce_the_offscreen_launch_and_clearing():
    t = _small()
    dt = _dev(t)
    n = 3
    cams = _cams(n)
    bg = 0.75
    opt = R.RenderOptions(spp=6, denoise=False, background_brightness=bg)
    depth = np.full((n, H, W), 1e9, f32)
    color = np.full((n, H, W, 4), bg, f32)

    def run(ctx, batched, kernel=R.KERNEL_AUTO):
        ctx.rng_seed()
        ctx.set_kernel(kernel)
        if batched:
            R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[4, 1, 2])
            return tuple(v.cpu().numpy() for v in _views(ctx, n))
        ctx.select_frame(1)
        R.launch_renderer(dt, cams[1], opt, ctx)
        return ctx.download_aux(), None, ctx.download_image()

    for batched, kernel in ((True, R.KERNEL_AUTO), (False, R.KERNEL_FAST), (False, R.KERNEL_GENERIC)):
        ctx = R.RenderContext(W, H, frames=n)
        want = run(ctx, batched, kernel)
        ctx.set_layers(*_dev_layers(depth, color))
        got = run(ctx, batched, kernel)
        assert_bits_equal(got[0], want[0], "trivial layers: all 8 aux planes")
        assert_bits_equal(got[2], want[2], "trivial layers: image")
        # real layers, then cleared: the next launch equals a launch on a fresh context
        d2, c2 = make_layers(t, cams)
        ctx.set_layers(*_dev_layers(d2, c2))
        changed = run(ctx, batched, kernel)
        assert not np.array_equal(changed[0], want[0])
        ctx.set_layers(None, None)
        assert ctx.layers() == (None, None) and ctx.offscreen
        again = run(ctx, batched, kernel)
        assert_bits_equal(again[0], want[0], "after clearing: aux")
        assert_bits_equal(again[2], want[2], "after clearing: image")


@pytest.fixture(scope="module")
def net():
    t = _torch()
    from rt_octree_amd import denoiser
    t.manual_seed(3)
    return denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval())


@pytest.mark.gpu
def test_depth_only_lean_levels_and_denoise(net):
    t = synth.make_tree(depth_limit=7, basis_dim=9, shell=2.5)
    dt = _dev(t)
    n = 4
    cams = _cams(n)
    depth, _ = make_layers(t, cams)
    opt = R.RenderOptions(spp=6, denoise=True, background_brightness=0.5)
    jumps = [9, 8, 7, 6]
    images = []
    for lean in (0, 1, 2):
        ctx = _batch(dt, cams, opt, jumps, depth, None, lean=lean)
        assert ctx.tile_marks() is not None and ctx.frames_lean_level(0, n) == lean
        if lean == 0:
            assert not _marks_of(ctx, n).all()  # (some tiles are culled)
        ctx.select_frame(0)
        net.denoise(ctx, n=n, mode=R.FILTER_FAST)
        _torch().cuda.synchronize()
        images.append(_views(ctx, n)[2].cpu().numpy())
        if lean == 0:  # the two-call form without marks
            aux, noisy, image = _views(ctx, n)
            keep = image.clone()
            image.fill_(-7.0)
            net.forward_packed(aux, squares_implied=True)
            net.filter_packed(ctx.noisy_ptr, ctx.image_ptr, shape=(n, H, W))
            _torch().cuda.synchronize()
            assert_bits_equal(image.cpu().numpy(), keep.cpu().numpy(), "depth only: rto_denoise vs the two-call form without marks")
    assert_bits_equal(images[1], images[0], "depth only: lean level 1 vs 0")
    assert_bits_equal(images[2], images[0], "depth only: lean level 2 vs 0")


@pytest.mark.gpu
def test_depth_and_colour_denoise_and_marks(net):
    t = synth.make_tree(depth_limit=7, basis_dim=9, shell=2.5)
    dt = _dev(t)
    n = 4
    cams = _cams(n)
    depth, color = make_layers(t, cams)
    opt = R.RenderOptions(spp=6, denoise=True)
    jumps = [9, 8, 7, 6]
    ctx = _batch(dt, cams, opt, jumps, depth, color)
    assert ctx.tile_marks() is None
    p, w, s0, k, bg = C.c_void_p(None), C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
    assert R.lib().rto_ctx_tile_marks(ctx._h, C.byref(p), C.byref(w), C.byref(s0), C.byref(k), C.byref(bg)) == E_INVALID
    assert b"rto_ctx_tile_marks" in R.lib().rto_last_error()
    aux, noisy, image = _views(ctx, n)
    for mode in (R.FILTER_FAST, R.FILTER_EXACT):
        ctx.select_frame(0)
        image.fill_(-7.0)
        net.denoise(ctx, n=n, mode=mode)
        _torch().cuda.synchronize()
        got = image.cpu().numpy().copy()
        wm, gm = net(aux)  # rto_guidance_net_forward_ex
        image.fill_(-7.0)
        R.filtering(None, wm, gm, noisy, image, mode=mode)  # rto_filtering_batch_mode
        _torch().cuda.synchronize()
        assert_bits_equal(got, image.cpu().numpy(), "depth + colour: rto_denoise vs the plain two-call form, mode %d" % mode)
    # sparse lean outputs need the constant backdrop
    ctx.set_lean_outputs(2)
    with pytest.raises(R.RtoError) as e:
        R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=jumps)
    assert e.value.code == E_UNSUPPORTED and R.lib().rto_last_error()


@pytest.mark.gpu
def test_refusals(tmp_path):
    t = _small()
    dt = _dev(t)
    cam = _cams(1)[0]
    tt = _torch()
    ctx = R.RenderContext(W, H, frames=2)
    L = R.lib()
    px = 2 * H * W
    depth = tt.ones(px, dtype=tt.float32, device="cuda")
    color = tt.ones(px * 4 + 4, dtype=tt.float32, device="cuda")
    set_layers = lambda d, c: L.rto_ctx_set_layers(ctx._h, C.c_void_p(d) if d else None, C.c_void_p(c) if c else None)

    def refused(rc, code):
        assert rc == code and L.rto_last_error(), rc

    assert set_layers(depth.data_ptr(), color.data_ptr()) == 0
    assert ctx.layers() == (depth.data_ptr(), color.data_ptr())
    refused(L.rto_ctx_set_layers(None, None, None), E_INVALID)
    refused(set_layers(depth.data_ptr(), color.data_ptr() + 4), E_INVALID)  # misaligned colour
    ctx.select_frame(0)
    aux, noisy, image = ctx.aux_ptr, ctx.noisy_ptr, ctx.image_ptr
    refused(set_layers(aux + 64, None), E_INVALID)  # overlap: aux / noisy / image, either layer
    refused(set_layers(None, noisy), E_INVALID)
    refused(set_layers(None, image + 16 * (px - 1)), E_INVALID)
    refused(set_layers(noisy + 4 * 4 * px - 4, None), E_INVALID)
    host = np.ones(px * 4, f32)
    refused(set_layers(host.ctypes.data, None), E_INVALID)  # not memory of the context's device
    if tt.cuda.device_count() > 1:
        other = tt.ones(px, dtype=tt.float32, device="cuda:1")
        refused(set_layers(other.data_ptr(), None), E_INVALID)
    assert ctx.layers() == (depth.data_ptr(), color.data_ptr())  # (a refused call changes nothing)
    opt = R.RenderOptions(spp=1, denoise=False)
    co, cc = opt.to_c(), cam.to_c()
    launch = lambda tree, o=co: L.rto_launch_renderer(tree._h, C.byref(cc), C.byref(o), ctx._h, None)
    cams2 = (_lib.CCamera * 2)(cc, cc)
    batch = lambda tree, o=co: L.rto_launch_renderer_batch(tree._h, cams2, None, 2, C.byref(o), ctx._h, None)
    assert launch(dt) == 0 and batch(dt) == 0
    ctx.enable_stats(True)  # layers + work counters
    refused(launch(dt), E_UNSUPPORTED)
    refused(batch(dt), E_UNSUPPORTED)
    ctx.enable_stats(False)
    path = str(tmp_path / "quant.npz")
    _small(basis=9, seed=11).save_quant_npz(path, n_retain=1, quantiser="luminance")
    q = R.N3Tree(path, quant_direct=True)  # layers + a quantised-direct tree
    refused(launch(q), E_UNSUPPORTED)
    refused(batch(q), E_UNSUPPORTED)
    probe = R.RenderOptions(spp=1, enable_probe=True).to_c()
    refused(launch(dt, probe), E_UNSUPPORTED)
    refused(batch(dt, probe), E_UNSUPPORTED)
    # the Python interface: shapes as in _ray_tensor; offscreen=False without layers keeps raising
    with pytest.raises(R.RtoError):
        ctx.set_layers(depth=tt.ones((2, H, W + 1), dtype=tt.float32, device="cuda"))
    with pytest.raises(R.RtoError):
        ctx.set_layers(color=tt.ones((2, H, W, 3), dtype=tt.float32, device="cuda"))
    with pytest.raises(R.RtoError):
        ctx.set_layers(depth=tt.ones((2, H, W), dtype=tt.float64, device="cuda"))
    ctx.set_layers(None, None)
    with pytest.raises(R.RtoError) as e:
        R.launch_renderer(dt, cam, opt, ctx, offscreen=False)
    assert e.value.code == E_UNSUPPORTED
    # rto_launch_rays ignores the layers
    ctx.rng_seed()
    o, d = R.camera_rays(cam)
    plain = R.render_rays(dt, o, d, opt, ctx).cpu().numpy()
    ctx.set_layers(depth.view(2, H, W) * 0.5, None)
    assert_bits_equal(R.render_rays(dt, o, d, opt, ctx).cpu().numpy(), plain, "rto_launch_rays ignores the layers")
    tt.cuda.synchronize()
