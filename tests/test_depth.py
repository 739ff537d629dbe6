"""Depth outputs (include/rto.h "depth outputs"): rto_launch_rays_ex, rto_ctx_enable_depth, volrend.render_rays(depth=, t_near=).

The expectation comes from the unchanged CPU oracle (depth_ref.py): orc_trace_ray's alpha as a function of t_max is a step
function whose steps are the ray's hits; bisection finds each step's boundary b_k and count cnt_k.

Tolerance, derived: b_k is the least float T with fl(T / delta_scale) > t_k, the kernel's d_k = fl(t_k * delta_scale).  The two
differ by the rounding of one division and of one product and by the granularity of T: |d_k - b_k| <= 3 ulp(b_k).  depth is a
weighted sum of at most SPP such positive terms, (float)cnt_k * d_k, added left to right and scaled by fl(1 / SPP): at most
SPP + 1 further roundings, each 2^-24 relative, on top of the 3 ulp (<= 3 * 2^-23 relative) of every term.  So
    |depth - sum_k (cnt_k / SPP) b_k| <= (4 + SPP) * 2^-23 * that sum,      |t_near - b_0| <= 3 ulp(b_0),
and a hit at distance 0 gives exactly 0."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_ref as D
import orc
import rt_octree_amd as R
from helpers import FRAME_ANISO, assert_bits_equal, cameras, reframe, reframe_pose
from rt_octree_amd import _lib, synth
from test_rays import _cam, _dev, _small, _tree, ray_oracle

E_INVALID, E_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 60, 44  # partial 32x8 workgroup tiles and partial 8x8 wave tiles
NEW_SYMBOLS = ("rto_launch_rays_ex", "rto_ctx_enable_depth", "rto_ctx_depth_enabled", "rto_ctx_depth", "rto_ctx_t_near",
               "rto_ctx_download_depth")


# ------------------------------------------------------------------ CPU


def test_library_exports_the_depth_symbols():
    header = open(os.path.join(ROOT, "include", "rto.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert hasattr(R.lib(), name), name
    assert "typedef struct rto_rays_out" in header


def test_rays_ex_refuses_a_call_without_outputs_before_any_device_use():
    """a null `out` and an `out` whose members are all null are RTO_E_INVALID -- decided before the tree, the context or a device
    is looked at: the handles here are never dereferenced (this runs without a GPU)"""
    L = R.lib()
    dummy_tree, dummy_ctx = C.create_string_buffer(64), C.create_string_buffer(64)
    rays = _lib.CRays()
    rays.n = 4
    opt = R.RenderOptions(spp=1).to_c()
    tree_h, ctx_h = C.cast(dummy_tree, C.c_void_p), C.cast(dummy_ctx, C.c_void_p)
    assert L.rto_launch_rays_ex(tree_h, C.byref(rays), C.byref(opt), ctx_h, None, None) == E_INVALID
    none = _lib.CRaysOut()
    assert L.rto_launch_rays_ex(tree_h, C.byref(rays), C.byref(opt), ctx_h, C.byref(none), None) == E_INVALID
    assert b"no output" in L.rto_last_error()
    assert L.rto_ctx_depth_enabled(None) == 0 and L.rto_ctx_depth(None) is None and L.rto_ctx_t_near(None) is None
    assert L.rto_ctx_enable_depth(None, 1) == E_INVALID and L.rto_ctx_download_depth(None, None, None, None) == E_INVALID


def test_the_reconstruction_reproduces_the_oracles_alpha():
    """the steps found by bisection add up to the alpha the oracle returns without a t_max, ray by ray, every step a whole
    number of samples; the rays meet the conditions the GPU tests rely on"""
    spp = 4
    _, ht, o, d = D.scene()
    hits, depth, t_near, calls = D.reference(spp)
    D.check_inputs(hits, spp)
    full = ray_oracle(ht, o, d, spp)[:, 3]
    assert_bits_equal(D.alpha_of(hits, spp).astype(f32), full, "sum of the steps vs the oracle's alpha")
    for h in hits:
        assert sum(c for _, c in h) <= spp and all(b1 < b2 for (b1, _), (b2, _) in zip(h, h[1:]))
    assert np.isinf(t_near[[not h for h in hits]]).all() and (depth[[not h for h in hits]] == 0).all()
    assert calls < 40 * D.N_RAYS


def test_the_reconstruction_reproduces_the_oracles_alpha_ndc():
    t = _small()
    ndc = (40.0, 30.0, 35.0)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)
    o, d = R.camera_rays(_cam(40, 30))
    o, d = np.ascontiguousarray(o[::3]), np.ascontiguousarray(d[::3])
    hits, _ = D.reconstruct(ht, o, d, 2, ndc=ndc)
    # (first_ray + i is the ray's own RNG offset in both)
    full = ray_oracle(ht, o, d, 2, ndc=ndc)[:, 3]
    assert_bits_equal(D.alpha_of(hits, 2).astype(f32), full, "sum of the steps vs the oracle's alpha (NDC)")
    assert sum(1 for h in hits if h) > 20


def test_depth_kernels_codegen():
    """every depth-carrying instantiation (depth_kernels.hip) exists, keeps a private segment no larger than its sibling's
    (render_kernels.hip) and at most one wave per SIMD less -- against the sibling of the same build, not against absolute numbers"""
    import shutil
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to cross-compile the kernels")
    from test_codegen import kernel_resources, render_resources
    res = dict(render_resources())
    new = kernel_resources("depth_kernels.hip")
    assert not set(res) & set(new)
    res.update(new)

    def one(prefix):
        found = [v for n, v in res.items() if n.startswith(prefix)]
        assert len(found) == 1, (prefix, len(found))
        return found[0]

    def check(new, old, what):
        assert new["scratch"] <= old["scratch"], (what, new, old)
        assert new["occupancy"] >= old["occupancy"] - 1, (what, new, old)

    for spp in (1, 2, 3, 4, 6, 8, 16, 32):
        for lobes in (0, 2, 3):
            for wide, stack in ((1, 1), (1, 0), (0, 0)):
                args = "ILi%dELb%dELi%dELi%dEEE" % (spp, wide, stack, lobes)
                check(one("_ZN3rto17render_rays_depth" + args), one("_ZN3rto11render_rays" + args), "rays" + args)
                check(one("_ZN3rto24render_fast_layers_depth" + args), one("_ZN3rto18render_fast_layers" + args), "frame" + args)
        args = "ILi%dEEE" % spp
        check(one("_ZN3rto25render_rays_generic_depth" + args), one("_ZN3rto19render_rays_generic" + args), "generic rays" + args)
        check(one("_ZN3rto27render_generic_layers_depth" + args), one("_ZN3rto21render_generic_layers" + args), "generic frame" + args)


def test_cli_write_depth_needs_an_output_directory(tmp_path):
    import subprocess
    from test_cli import BIN
    p = synth.write_transforms_json(str(tmp_path / "t.json"), synth.orbit_poses(2))
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--write_depth" in r.stdout
    tp = _small(depth=3).save_npz(str(tmp_path / "tree.npz"))
    r = subprocess.run([BIN, tp, p, "--write_depth"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--write_depth needs -o" in r.stderr


# ------------------------------------------------------------------ GPU


def _ctx(kernel=R.KERNEL_AUTO, w=8, h=8, frames=1, depth=False):
    ctx = R.RenderContext(w, h, frames=frames)
    ctx.rng_seed()
    ctx.set_kernel(kernel)
    if depth:
        ctx.enable_depth()
    return ctx


def _rays3(dt, o, d, opt, ctx, **kw):
    rgba, depth, t_near = R.render_rays(dt, o, d, opt, ctx, depth=True, t_near=True, **kw)
    return rgba.cpu().numpy(), depth.cpu().numpy(), t_near.cpu().numpy()


def _check_against(depth, t_near, want_depth, want_near, spp, what):
    """the derived tolerance of the module docstring; figures printed before they are asserted"""
    hit = np.isfinite(want_near)
    assert np.array_equal(np.isfinite(t_near), hit), what
    assert (depth[~hit] == 0).all() and np.isposinf(t_near[~hit]).all(), what
    rel = np.abs(depth[hit].astype(np.float64) - want_depth[hit]) / np.maximum(want_depth[hit], np.finfo(np.float64).tiny)
    rel[want_depth[hit] == 0] = 0.0
    assert (depth[hit][want_depth[hit] == 0] == 0).all(), what  # (every hit at distance 0: exactly 0)
    off = np.abs(t_near[hit].astype(np.float64) - want_near[hit]) / D.ulp(want_near[hit])
    print("%s: depth rel err max %.3g (bound %.3g), t_near max %.2f ulp (bound 3), %d rays with a hit" % (
        what, rel.max(), (4 + spp) * 2.0 ** -23, off.max(), hit.sum()))
    assert (rel <= (4 + spp) * 2.0 ** -23).all(), (what, rel.max())
    assert (off <= 3).all(), (what, off.max())
    assert (t_near[hit][want_near[hit] == 0] == 0).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4, 6])
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_rays_match_the_reconstruction(spp, kernel):
    t, ht, o, d = D.scene()
    hits, want_depth, want_near, _ = D.reference(spp)
    D.check_inputs(hits, spp)
    dt = _dev(t)
    ctx = _ctx(kernel)
    opt = R.RenderOptions(spp=spp)
    rgba, depth, t_near = _rays3(dt, o, d, opt, ctx)
    assert_bits_equal(rgba, R.render_rays(dt, o, d, opt, ctx).cpu().numpy(), "rgba beside the depth outputs vs rto_launch_rays")
    _check_against(depth, t_near, want_depth, want_near, spp, "spp %d kernel %d" % (spp, kernel))


def _fast_vs_generic(dt, o, d, spp, tuning=()):
    out = []
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx = _ctx(kernel)
        for k, v in tuning:
            ctx.set_tuning(k, v)
        out.append(_rays3(dt, o, d, R.RenderOptions(spp=spp), ctx))
    for a, b, what in zip(out[0], out[1], ("rgba", "depth", "t_near")):
        assert_bits_equal(a, b, "fast vs generic: " + what)
    return out[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,basis", [("RGBA", -1), ("SH", 9), ("SH", 16), ("SG", 16), ("ASG", 9)])
@pytest.mark.parametrize("spp", [1, 6, 32])
def test_fast_and_generic_kernels_agree_bit_for_bit(kind, basis, spp):
    _, _, o, d = D.scene()
    _, depth, t_near = _fast_vs_generic(_dev(_tree(kind, basis)), o, d, spp)
    assert np.isfinite(t_near).sum() >= 100 and (depth[np.isfinite(t_near)] >= 0).all() and (t_near == 0).any()


@pytest.mark.gpu
def test_fast_and_generic_kernels_agree_on_the_one_level_image_and_on_a_deep_tree():
    _, _, o, d = D.scene()
    # (slot-ordered records: a tree whose records follow the two-level image's entries has no one-level fallback; 2^6 entries:
    #  nothing fits, the launch takes the WIDE = false instantiation)
    _, _, t_near = _fast_vs_generic(_dev(_tree("SH", 9), compact_records=True), o, d, 6, tuning=(("wide_bits", 6),))
    assert np.isfinite(t_near).sum() >= 100
    from test_render_parity import _chain_tree
    deep = _chain_tree(13, seed=13)  # four pairs of levels below the grid: the ancestor stack lives in LDS rows (STACK == 0)
    dt = _dev(deep)
    assert (dt.max_depth - 6 + 1) // 2 > 2 and dt.wide_nodes > 0
    _, cam = cameras(56, 40, synth.look_at_c2w((2.2, 1.7, 1.9), target=(0.0, -0.1, 0.05)))
    co, cd = R.camera_rays(cam)
    _, _, t_near = _fast_vs_generic(dt, co, cd, 6)
    assert np.isfinite(t_near).sum() >= 100


def _frame_vs_rays(t, dt, cam, spp, kernel, depth_layer=None, color=None, tuning=()):
    """a frame of a context with depth outputs == rto_launch_rays_ex on the camera's rays, all outputs bit for bit"""
    ctx = _ctx(kernel, cam.width, cam.height, depth=True)
    ctx.rng_advance()
    for k, v in tuning:
        ctx.set_tuning(k, v)
    if depth_layer is not None or color is not None:
        ctx.set_layers(depth_layer, color)
    opt = R.RenderOptions(spp=spp, denoise=False)
    R.launch_renderer(dt, cam, opt, ctx)
    aux = ctx.download_aux()
    fdepth, fnear = ctx.download_depth()
    o, d = R.camera_rays(cam)
    rctx = _ctx(kernel)
    rctx.rng_advance()
    rgba, depth, t_near = _rays3(dt, o, d, opt, rctx, t_max=None if depth_layer is None else depth_layer.reshape(-1),
                                 background=None if color is None else np.ascontiguousarray(color.reshape(-1, 4)[:, :3]))
    assert_bits_equal(np.ascontiguousarray(aux[:4].reshape(4, -1).T), rgba, "frame vs rays: rgba")
    assert_bits_equal(fdepth.reshape(-1), depth, "frame vs rays: depth")
    assert_bits_equal(fnear.reshape(-1), t_near, "frame vs rays: t_near")
    import torch
    assert_bits_equal(torch.as_tensor(ctx.depth_view(), device="cuda").cpu().numpy(), fdepth, "depth_view")
    assert_bits_equal(torch.as_tensor(ctx.t_near_view(), device="cuda").cpu().numpy(), fnear, "t_near_view")
    return fdepth, fnear


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
def test_a_frame_equals_the_rays_of_its_camera(kernel):
    from layers_ref import make_layers
    t = _small()
    dt = _dev(t)
    cam = _cam(W, H)
    plain_d, plain_n = _frame_vs_rays(t, dt, cam, 6, kernel)  # offscreen
    assert np.isfinite(plain_n).sum() > 200
    layer_depth, layer_color = make_layers(t, [cam])
    cut_d, cut_n = _frame_vs_rays(t, dt, cam, 6, kernel, depth_layer=layer_depth[0], color=layer_color[0])
    assert np.isfinite(cut_n).sum() > 100 and (cut_n != plain_n).sum() > 50  # (the layer cuts the object in half)
    if kernel == R.KERNEL_FAST:
        cull_d, cull_n = _frame_vs_rays(t, dt, cam, 6, kernel, tuning=(("cull_single", 1),))
        assert_bits_equal(cull_d, plain_d, "cull_single: depth")
        assert_bits_equal(cull_n, plain_n, "cull_single: t_near")
    ndc = _dev(t)
    ndc.set_ndc(float(W), float(H), 40.0)
    _, ndc_n = _frame_vs_rays(t, ndc, cam, 4, kernel)
    assert np.isfinite(ndc_n).sum() > 20
    t2 = reframe(t, *FRAME_ANISO)
    _, cam2 = cameras(W, H, reframe_pose(synth.orbit_poses(4)[1], t, t2))
    _, aniso_n = _frame_vs_rays(t2, _dev(t2), cam2, 6, kernel)
    assert np.isfinite(aniso_n).sum() > 200


def _poses(n):
    cams = []
    for i in range(n):
        cams.append(_cam(W, H, pose=i))
    return cams


def _slot_outputs(ctx, slot):
    ctx.select_frame(slot)
    return (ctx.download_aux(), ctx.download_image()) + ctx.download_depth()


@pytest.mark.gpu
def test_a_batch_on_a_depth_context_is_n_single_launches():
    t = _small()
    dt = _dev(t)
    cams, jumps = _poses(3), [4, 1, 7]
    opt = R.RenderOptions(spp=6, denoise=False)
    bctx = _ctx(w=W, h=H, frames=3, depth=True)
    R.launch_renderer_batch(dt, cams, opt, bctx, rng_jumps=jumps)
    assert bctx.tile_marks() is None  # (rto_ctx_tile_marks: RTO_E_INVALID, as after any single-frame launch)
    for f in range(3):
        one = _ctx(w=W, h=H, depth=True)
        for _ in range(jumps[f]):
            one.rng_advance()
        R.launch_renderer(dt, cams[f], opt, one)
        for a, b, what in zip(_slot_outputs(bctx, f), _slot_outputs(one, 0), ("aux", "image", "depth", "t_near")):
            assert_bits_equal(a, b, "batch frame %d vs a single launch: %s" % (f, what))
        assert np.isfinite(_slot_outputs(bctx, f)[3]).sum() > 200
    bctx.set_lean_outputs(1)
    with pytest.raises(R.RtoError) as e:
        R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=True), bctx, rng_jumps=jumps)
    assert e.value.code == E_UNSUPPORTED


@pytest.mark.gpu
def test_t_max_cuts_degenerate_rays_and_a_start_inside_density():
    """derived as the module docstring's bound: a hit exists only with t_k < fl(T / delta_scale), so d_k = fl(t_k delta_scale)
    lies below T up to the roundings of that division and that product -- t_near < T + 3 ulp(T); and depth, a sum of
    cnt_k / SPP shares of such d_k, stays below alpha * T by the same (4 + SPP) 2^-23 plus the two roundings of alpha itself"""
    spp = 4
    t, ht, o, d = D.scene()
    hits, _, want_near, _ = D.reference(spp)
    dt = _dev(t)
    tm = np.random.default_rng(4).uniform(0.0, 1.5 / float(t.scale[0]), o.shape[0]).astype(f32)
    tm[::7] = np.inf
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx = _ctx(kernel)
        opt = R.RenderOptions(spp=spp)
        rgba, depth, t_near = _rays3(dt, o, d, opt, ctx, t_max=tm)
        assert_bits_equal(rgba, R.render_rays(dt, o, d, opt, ctx, t_max=tm).cpu().numpy(), "rgba with t_max")
        hit = np.isfinite(t_near)
        assert hit.sum() > 50 and (hit != np.isfinite(want_near)).sum() > 10  # (some rays lose every hit to their t_max)
        lim = tm.astype(np.float64)
        assert (t_near[hit] < lim[hit] + 3 * D.ulp(np.minimum(lim[hit], 3e38))).all()
        assert (depth[hit] <= rgba[hit, 3].astype(np.float64) * lim[hit] * (1 + (6 + spp) * 2.0 ** -23)).all()
        assert (depth[~hit] == 0).all() and (rgba[~hit, 3] == 0).all()
        # a hit that survives its t_max is the hit the uncut ray has first
        keep = hit & (want_near < lim * (1 - 2.0 ** -20))
        assert keep.sum() > 50 and (np.abs(t_near[keep] - want_near[keep]) <= 3 * D.ulp(want_near[keep])).all()
        # rays that start inside a dense leaf and cross a threshold in their first step (from the reconstruction)
        zero = np.array([bool(h) and h[0][0] == 0.0 for h in hits])
        full = _rays3(dt, o, d, opt, ctx)[2]
        assert zero.any() and (full[zero] == 0).all()
    # degenerate rays: (0, +inf) and their backdrop
    inside = ((np.full((1, 3), 0.5, f32) - t.offset[None, :]) / t.scale[None, :]).astype(f32)[0]
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
    bad_d[8] = 1e-30
    bg = np.random.default_rng(1).uniform(0, 1, (9, 3)).astype(f32)
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        rgba, depth, t_near = _rays3(dt, bad_o, bad_d, R.RenderOptions(spp=6), _ctx(kernel), t_max=bad_t, background=bg)
        assert_bits_equal(rgba, np.concatenate([bg, np.zeros((9, 1), f32)], 1), "degenerate rays")
        assert (depth == 0).all() and np.isposinf(t_near).all()
    # a ray that misses the box
    away = np.array([[0.0, 0.0, -1.0]], f32)
    far_o = ((np.array([[0.5, 0.5, -3.0]], f32) - t.offset[None, :]) / t.scale[None, :]).astype(f32)
    _, depth, t_near = _rays3(dt, far_o, away, R.RenderOptions(spp=6), _ctx())
    assert depth[0] == 0 and np.isposinf(t_near[0])


@pytest.mark.gpu
def test_split_calls_and_repeats_give_the_same_bytes():
    t, _, o, d = D.scene()
    dt = _dev(t)
    opt = R.RenderOptions(spp=6)
    first = 3 << 30
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx = _ctx(kernel)
        whole = _rays3(dt, o, d, opt, ctx, first_ray=first)
        for a, b in zip(_rays3(dt, o, d, opt, ctx, first_ray=first), whole):
            assert_bits_equal(a, b, "repeat")
        parts = [_rays3(dt, o[a:b], d[a:b], opt, ctx, first_ray=first + a) for a, b in ((0, 1), (1, 300), (300, 1000))]
        for k, what in enumerate(("rgba", "depth", "t_near")):
            assert_bits_equal(np.concatenate([p[k] for p in parts]), whole[k], "split calls: " + what)
        # each output by itself is the same output
        only_d = R.render_rays(dt, o, d, opt, ctx, first_ray=first, depth=True)
        only_n = R.render_rays(dt, o, d, opt, ctx, first_ray=first, t_near=True)
        assert len(only_d) == 2 and len(only_n) == 2
        assert_bits_equal(only_d[1].cpu().numpy(), whole[1], "depth alone")
        assert_bits_equal(only_n[1].cpu().numpy(), whole[2], "t_near alone")
        assert_bits_equal(_raw_ex(dt, o, d, opt, ctx, first, rgba=False)[1], whole[1], "no rgba asked for")
        no_rgba = R.render_rays(dt, o, d, opt, ctx, first_ray=first, depth=True, t_near=True, rgba=False)
        assert len(no_rgba) == 2
        assert_bits_equal(no_rgba[0].cpu().numpy(), whole[1], "rgba=False: depth")
        assert_bits_equal(no_rgba[1].cpu().numpy(), whole[2], "rgba=False: t_near")
        with pytest.raises(R.RtoError):
            R.render_rays(dt, o, d, opt, ctx, rgba=False)
    assert len(R.render_rays(dt, o[:0], d[:0], opt, ctx, depth=True, t_near=True)) == 3


def _raw_ex(dt, o, d, opt, ctx, first_ray=0, rgba=True, depth=True, t_near=True):
    """rto_launch_rays_ex through ctypes with the outputs asked for -> (rgba, depth, t_near) numpy arrays or None"""
    import torch
    n = o.shape[0]
    dev = torch.device("cuda", 0)
    to, td = torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev)
    bufs = [torch.full((n, 4), -7.0, device=dev) if rgba else None, torch.full((n,), -7.0, device=dev) if depth else None,
            torch.full((n,), -7.0, device=dev) if t_near else None]
    r = _lib.CRays()
    r.origins, r.dirs, r.n, r.first_ray = to.data_ptr(), td.data_ptr(), n, first_ray
    ro = _lib.CRaysOut()
    ro.rgba, ro.depth, ro.t_near = (b.data_ptr() if b is not None else None for b in bufs)
    co = opt.to_c()
    _lib.check(R.lib().rto_launch_rays_ex(dt._h, C.byref(r), C.byref(co), ctx._h, C.byref(ro), None))
    torch.cuda.synchronize()
    return [b.cpu().numpy() if b is not None else None for b in bufs]


@pytest.mark.gpu
def test_with_depth_off_nothing_changes():
    from layers_ref import make_layers
    t, _, o, d = D.scene()
    dt = _dev(t)
    opt = R.RenderOptions(spp=6, denoise=False)
    cams = _poses(3)
    # rays: only rgba asked for is rto_launch_rays
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        ctx = _ctx(kernel)
        assert_bits_equal(_raw_ex(dt, o, d, opt, ctx, depth=False, t_near=False)[0], R.render_rays(dt, o, d, opt, ctx).cpu().numpy(),
                          "rto_launch_rays_ex(rgba) vs rto_launch_rays")
    # frames: a context whose depth outputs were enabled and disabled again, and one that is enabled, against one that never was
    layer_depth, layer_color = make_layers(t, cams)
    for layered in (False, True):
        outs = []
        for mode in ("never", "off again", "on"):
            ctx = _ctx(w=W, h=H, frames=3)
            if mode != "never":
                ctx.enable_depth()
                assert ctx.depth_enabled() and ctx.depth_view() is not None
            if mode == "off again":
                ctx.enable_depth(False)
            if mode != "on":
                assert not ctx.depth_enabled() and ctx.depth_view() is None and ctx.t_near_view() is None
                with pytest.raises(R.RtoError):
                    ctx.download_depth()
            if layered:
                ctx.set_layers(layer_depth, layer_color)
            R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[4, 1, 7])
            if mode != "on":
                assert (ctx.tile_marks() is not None) == (not layered)  # (the batched kernels ran)
            frames = []
            for f in range(3):
                ctx.select_frame(f)
                frames.append((ctx.download_aux(), ctx.download_image()))
            ctx.select_frame(1)
            ctx.set_kernel(R.KERNEL_FAST)
            R.launch_renderer(dt, cams[2], opt, ctx)
            frames.append((ctx.download_aux(), ctx.download_image()))
            outs.append(frames)
        for other, what in ((outs[1], "depth disabled again"), (outs[2], "depth enabled")):
            for f, (a, b) in enumerate(zip(outs[0], other)):
                assert_bits_equal(a[0], b[0], "%s, layered %d, frame %d: aux" % (what, layered, f))
                assert_bits_equal(a[1], b[1], "%s, layered %d, frame %d: image" % (what, layered, f))


@pytest.mark.gpu
def test_refusals(tmp_path):
    import torch
    t = _small()
    dt = _dev(t)
    cam = _cam(W, H)
    ctx = _ctx(w=W, h=H, frames=2, depth=True)
    opt = R.RenderOptions(spp=1, denoise=False)

    def refused(fn):
        with pytest.raises(R.RtoError) as e:
            fn()
        assert e.value.code == E_UNSUPPORTED, e.value

    R.launch_renderer(dt, cam, opt, ctx)
    probe = R.RenderOptions(spp=1, denoise=False, enable_probe=True)
    refused(lambda: R.launch_renderer(dt, cam, probe, ctx))
    refused(lambda: R.launch_renderer_batch(dt, [cam, cam], probe, ctx))
    ctx.enable_stats(True)
    refused(lambda: R.launch_renderer(dt, cam, opt, ctx))
    refused(lambda: R.launch_renderer_batch(dt, [cam, cam], opt, ctx))
    ctx.enable_stats(False)
    path = str(tmp_path / "quant.npz")
    _small(basis=9, seed=11).save_quant_npz(path, n_retain=1, quantiser="luminance")
    q = R.N3Tree(path, quant_direct=True)
    refused(lambda: R.launch_renderer(q, cam, opt, ctx))
    refused(lambda: R.launch_renderer_batch(q, [cam, cam], opt, ctx))
    for level in (1, 2):
        ctx.set_lean_outputs(level)
        refused(lambda: R.launch_renderer_batch(dt, [cam, cam], R.RenderOptions(spp=1, denoise=True), ctx))
    ctx.set_lean_outputs(0)
    R.launch_renderer_batch(dt, [cam, cam], opt, ctx)  # (and nothing above left the context unusable)
    ctx.enable_depth(False)
    R.launch_renderer(dt, cam, probe, ctx)  # (with depth off the probe is drawn as before)
    # rto_launch_rays_ex: the argument checks of rto_launch_rays, and its own
    L = R.lib()
    o = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    d = torch.ones((4, 3), dtype=torch.float32, device="cuda")
    buf = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    rays = _lib.CRays()
    rays.origins, rays.dirs, rays.n = o.data_ptr(), d.data_ptr(), 4
    co = opt.to_c()

    def ex(rgba=None, depth=None, t_near=None, tree=dt._h, r=rays, c=ctx._h, options=co):
        ro = _lib.CRaysOut()
        ro.rgba, ro.depth, ro.t_near = rgba, depth, t_near
        return L.rto_launch_rays_ex(tree, C.byref(r) if r is not None else None, C.byref(options) if options is not None else None, c,
                                    C.byref(ro), None)

    p = buf.data_ptr()
    assert ex(rgba=p, depth=p + 256, t_near=p + 512) == 0
    assert ex(depth=p) == 0 and ex(t_near=p) == 0
    assert ex() == E_INVALID
    assert L.rto_launch_rays_ex(dt._h, C.byref(rays), C.byref(co), ctx._h, None, None) == E_INVALID
    assert ex(depth=p, tree=None) == E_INVALID and ex(depth=p, r=None) == E_INVALID and ex(depth=p, c=None) == E_INVALID
    assert ex(depth=p, options=None) == E_INVALID
    assert ex(rgba=p + 4, depth=p) == E_INVALID and ex(depth=p + 2) == E_INVALID and ex(t_near=p + 1) == E_INVALID
    neg = _lib.CRays()
    neg.origins, neg.dirs, neg.n = o.data_ptr(), d.data_ptr(), -1
    assert ex(depth=p, r=neg) == E_INVALID
    assert ex(depth=p, options=R.RenderOptions(spp=5).to_c()) == -2
    assert ex(depth=p, options=probe.to_c()) == E_UNSUPPORTED
    assert ex(depth=p, tree=q._h) == E_UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cli_write_depth(tmp_path):
    """--write_depth: depth_<name>.bin beside each pose's image, float32 [2][H][W] = depth, t_near of that frame -- the planes
    rto_launch_renderer writes for the pose with the CLI's RNG (advanced warmup + i times), one launch per frame whatever --batch"""
    import subprocess
    from test_cli import BIN
    tree = _small()
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(3)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    op = synth.write_opt_json(str(tmp_path / "opt.json"), denoise=False, spp=6)
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, tp, pp, "--options", op, "-w", str(W), "-h", str(H), "-o", out, "--warmup", "2", "--batch", "3",
                        "--write_depth"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    dt = _dev(tree)
    fx = synth.blender_focal(W)
    for i in range(3):
        assert os.path.exists(os.path.join(out, "r_%d.png" % i))
        got = np.fromfile(os.path.join(out, "depth_r_%d.bin" % i), f32)
        assert got.size == 2 * H * W
        cam = R.Camera(W, H, fx, fx)
        cam.set_c2w(poses[i])
        ctx = _ctx(w=W, h=H, depth=True)
        for _ in range(2 + i):
            ctx.rng_advance()
        R.launch_renderer(dt, cam, R.RenderOptions(spp=6, denoise=False), ctx)
        depth, t_near = ctx.download_depth()
        assert_bits_equal(got.reshape(2, H, W)[0], depth, "depth_r_%d.bin: depth" % i)
        assert_bits_equal(got.reshape(2, H, W)[1], t_near, "depth_r_%d.bin: t_near" % i)
        assert np.isfinite(t_near).sum() > 200
