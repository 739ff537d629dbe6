"""rto_draw_grid_layers / volrend.draw_grid_layers / RenderContext.show_grid / volrend_headless --grid: the octree grid
(RenderOptions::show_grid) ray-traced into a depth and a colour layer.

grid_ref.grid_depth restates the kernel in numpy float32; the GPU tests are bit for bit against it.  The CPU tests check the model
against a float64 geometry of the truncated cells' edges (grid_ref.wire_segments) on the twelve cases Shapes A-C x poses 0, 5 x
line_px 1, 2.5.  Measured with this model (worst of the twelve): largest rho_min of a line pixel 1.002; largest distance of a hit
point from a wire 1.152 r; no pixel with rho_min < 0.5 (nor < 0.8) and a chord > 8 r missed -- without the chord condition 47 and
161 silhouette rays of Shape C pose 5 are; front-most: 242 of 18676 = 1.30 % of the sure pixels lie more than 4 r behind the
nearest sure wire (Shape C, pose 5, line_px 2.5), the other cases 0 to 0.35 %."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grid_ref as G
import layer_ref
import rt_octree_amd as R
from helpers import assert_bits_equal, check_33_cameras_in_one_call, gpu_torch as _torch, rcam as _rcam
from rt_octree_amd import _lib, synth

E_INVALID, E_UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rt-octree_amd", "bin", "volrend_headless")
f32 = np.float32


# ------------------------------------------------------------------ CPU
def test_grid_symbols_are_exported_and_the_defaults_are_right():
    hdr = open(os.path.join(ROOT, "include", "rto.h")).read()
    assert "#define RTO_GRID_MERGE 1" in hdr and "typedef struct rto_grid_params" in hdr
    assert "void rto_grid_params_default(" in hdr and "int rto_draw_grid_layers(" in hdr
    L = R.lib()
    for name in ("rto_grid_params_default", "rto_draw_grid_layers"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.rto_draw_grid_layers.restype is C.c_int and len(L.rto_draw_grid_layers.argtypes) == 7
    p = _lib.CGridParams()
    o = R.RenderOptions().to_c()
    L.rto_grid_params_default(C.byref(p), C.byref(o))
    assert (p.max_depth, p.line_px, list(p.color), p.background, p.flags) == (4, 1.0, [0.0, 0.0, 0.0], 1.0, 0)
    o = R.RenderOptions(grid_max_depth=2, background_brightness=0.25).to_c()
    L.rto_grid_params_default(C.byref(p), C.byref(o))
    assert (p.max_depth, p.line_px, p.background, p.flags) == (2, 1.0, 0.25, 0)
    L.rto_grid_params_default(C.byref(p), None)  # the default options
    assert (p.max_depth, p.background) == (4, 1.0)
    g = R.GridParams(R.RenderOptions(grid_max_depth=3), line_px=2.5)
    assert (g.max_depth, g.line_px, g.background, g.color) == (3, 2.5, 1.0, [0.0, 0.0, 0.0])
    assert R.GRID_MERGE == 1 and g.to_c(merge=True).flags == 1
    assert hasattr(R.RenderContext, "show_grid") and callable(R.draw_grid_layers)


def _raw(tree_h, cams, n, p, depth, color):
    arr = (_lib.CCamera * max(1, len(cams)))(*[c.to_c() for c in cams]) if cams is not None else None
    return R.lib().rto_draw_grid_layers(tree_h, arr, n, C.byref(p) if p is not None else None, depth, color, None)


def _invalid_calls(tree_h, cam, depth, color):
    """every RTO_E_INVALID of include/rto.h as (what, thunk -> rc); depth / color: valid device pointers or fake ones"""
    def params(**kw):
        return R.GridParams(**kw).to_c()

    return layer_ref.invalid_layer_calls(_raw, params, tree_h, cam, depth, color) + [
        ("line_px < 0", lambda: _raw(tree_h, [cam], 1, params(line_px=-1.0), depth, color)),
        ("line_px inf", lambda: _raw(tree_h, [cam], 1, params(line_px=float("inf")), depth, color)),
        ("max_depth < 0", lambda: _raw(tree_h, [cam], 1, params(max_depth=-1), depth, color)),
        ("colour nan", lambda: _raw(tree_h, [cam], 1, params(color=[0.0, float("nan"), 0.0]), depth, color)),
        ("colour inf", lambda: _raw(tree_h, [cam], 1, params(color=[float("inf"), 0.0, 0.0]), depth, color)),
    ]


def test_grid_argument_checks_run_before_any_device_use():
    fake = C.create_string_buffer(256)  # never dereferenced: every check below returns first
    h = C.cast(fake, C.c_void_p)
    cam = R.Camera(32, 24, 40.0, 40.0)
    for what, call in _invalid_calls(h, cam, h, h):
        assert call() == E_INVALID, what
        assert R.lib().rto_last_error().decode().startswith("rto_draw_grid_layers:"), what


@pytest.mark.parametrize("name,pose,line_px", G.CASES)
def test_model_draws_the_wires_only_the_wires_and_the_front_ones(name, pose, line_px):
    tree, D, W, H = G.shape(name)
    cam = G.case_cam(name, pose)
    depth = G.case_depth(name, pose, line_px)
    S, n_cells = G.wire_segments(tree, D)
    assert n_cells >= 64 and (name == "A") == (n_cells == 64)  # A: every cell at the cap; B, C: mixed levels
    rho, t_front = G.rho_min(S, cam, line_px)
    line = np.isfinite(depth)
    hit = G.hit_distance(S, cam, depth, line_px)
    sure = (rho < 0.5) & (G.chord_over_r(tree, cam, line_px) > 8.0)
    r_front = 0.5 * line_px * t_front / cam.fx
    with np.errstate(invalid="ignore"):
        late = sure & line & ((depth.astype(np.float64) - t_front) > 4.0 * r_front)
    print("%s pose %d line_px %.1f: %d line pixels, max rho_min on a line pixel %.3f, max hit distance %.3f r, %d sure pixels, "
          "%d missed, %d late (%.2f %%)" % (name, pose, line_px, line.sum(), rho[line].max(), hit.max(), sure.sum(),
                                           (sure & ~line).sum(), late.sum(), 100.0 * late.sum() / sure.sum()))
    assert line.sum() > 4000 and sure.sum() > 2000
    assert not (rho[line] > 1.5).any(), "a line pixel further than 1.5 half widths from every wire"
    assert hit.max() <= 1.5, "a hit point further than 1.5 r from every wire"
    assert not (sure & ~line).any(), "a pixel within half a half width of a wire is no line pixel"
    assert late.sum() <= 0.03 * sure.sum(), "more than 3 % of the sure pixels show a wire behind the front one"


# ------------------------------------------------------------------ GPU
def _upload(tree, walk="wide", **kw):
    """the walks a tree can be loaded with (as tests/test_query.py selects them): the two-level image, or with RTO_NO_WIDE=1 the
    one-level image"""
    if walk == "nodew":
        os.environ["RTO_NO_WIDE"] = "1"
    try:
        dt = R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra, **kw)
    finally:
        os.environ.pop("RTO_NO_WIDE", None)
    assert (dt.wide_nodes > 0) == (walk == "wide")
    return dt


def _world(tree, xyz):
    return (np.asarray(xyz, np.float64) - tree.offset.astype(np.float64)) / tree.scale.astype(np.float64)


def _special_cams(tree, W, H):
    """(a camera inside the box, a camera whose every ray misses the box)"""
    inside = _rcam(W, H, synth.look_at_c2w(_world(tree, (0.4, 0.45, 0.55)), _world(tree, (0.95, 0.8, 0.1))))
    pos = np.asarray(synth.orbit_poses(16)[3], np.float64)[:3, 3]
    away = _rcam(W, H, synth.look_at_c2w(pos, 2.0 * pos))
    return inside, away


def _draw(dt, cams, params, **kw):
    d, c = R.draw_grid_layers(dt, cams, params, **kw)
    _torch().cuda.synchronize()
    return (None if d is None else d.cpu().numpy()), (None if c is None else c.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["wide", "nodew"])
@pytest.mark.parametrize("line_px", [1.0, 2.5])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_layers_equal_the_model_bit_for_bit(name, line_px, walk):
    """one call of four cameras: orbit poses 0 and 5, one inside the box, one that misses it"""
    tree, D, W, H = G.shape(name)
    dt = _upload(tree, walk)
    inside, away = _special_cams(tree, W, H)
    cams = [_rcam(W, H, synth.orbit_poses(16)[0]), _rcam(W, H, synth.orbit_poses(16)[5]), inside, away]
    params = R.GridParams(max_depth=D, line_px=line_px, color=[0.9, 0.2, 0.1], background=0.75)
    want_d = np.stack([G.case_depth(name, 0, line_px), G.case_depth(name, 5, line_px), G.grid_depth(tree, inside, D, line_px),
                       G.grid_depth(tree, away, D, line_px)])
    assert np.isfinite(want_d[2]).sum() > 1000 and np.isinf(want_d[3]).all() and (want_d[3] > 0).all()
    line = np.isfinite(want_d)
    want_c = np.empty(want_d.shape + (4,), f32)
    want_c[..., :3] = np.where(line[..., None], np.array([0.9, 0.2, 0.1], f32), f32(0.75))
    want_c[..., 3] = 1.0
    got_d, got_c = _draw(dt, cams, params)
    assert_bits_equal(got_d, want_d, "depth")
    assert_bits_equal(got_c, want_c, "colour")


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["wide", "nodew"])
def test_partial_tiles_every_cut_off_and_a_reframed_tree(walk):
    """67 x 45: partial 8 x 8 tiles and a partial last workgroup; max_depth 0 (the root's children), 3 and 30 (clamped to 22: every
    leaf of the tree is a cell) on Shape C's anisotropic tree"""
    tree, _, _, _ = G.shape("C")
    dt = _upload(tree, walk)
    W, H = 67, 45
    cams = [_rcam(W, H, synth.orbit_poses(16)[p]) for p in (0, 5, 11)]
    for D, lp in ((0, 2.0), (3, 1.0), (30, 1.5)):
        want_d, want_c = G.grid_layers(tree, cams, D, lp, color=(0.0, 0.0, 0.0), background=1.0)
        assert np.isfinite(want_d).sum() > 500
        got_d, got_c = _draw(dt, cams, R.GridParams(max_depth=D, line_px=lp))
        assert_bits_equal(got_d, want_d, "depth, max_depth %d" % D)
        assert_bits_equal(got_c, want_c, "colour, max_depth %d" % D)


@pytest.mark.gpu
def test_one_call_equals_three_and_a_null_output_leaves_the_other_unchanged():
    torch = _torch()
    tree, D, _, _ = G.shape("B")
    dt = _upload(tree)
    W, H = 67, 45
    cams = [_rcam(W, H, synth.orbit_poses(16)[p]) for p in (0, 5, 9)]
    params = R.GridParams(max_depth=D, line_px=1.5, color=[0.1, 0.2, 0.3], background=0.5)
    d3, c3 = R.draw_grid_layers(dt, cams, params)
    for f in range(3):
        d1, c1 = R.draw_grid_layers(dt, [cams[f]], params)
        assert torch.equal(d1[0].view(torch.int32), d3[f].view(torch.int32)) and torch.equal(c1[0].view(torch.int32), c3[f].view(torch.int32)), f
    d_only, none = R.draw_grid_layers(dt, cams, params, color=False)
    assert none is None and torch.equal(d_only.view(torch.int32), d3.view(torch.int32))
    none, c_only = R.draw_grid_layers(dt, cams, params, depth=False)
    assert none is None and torch.equal(c_only.view(torch.int32), c3.view(torch.int32))
    # more cameras than travel in one launch's arguments (32): frame f of 70 is camera f % 3
    many = [cams[f % 3] for f in range(70)]
    d70, c70 = R.draw_grid_layers(dt, many, params)
    for f in (0, 31, 32, 33, 63, 64, 69):
        assert torch.equal(d70[f].view(torch.int32), d3[f % 3].view(torch.int32)) and torch.equal(c70[f].view(torch.int32), c3[f % 3].view(torch.int32)), f
    # n == 0 launches nothing
    d0, c0 = R.draw_grid_layers(dt, [], params)
    assert tuple(d0.shape) == (0, 0, 0)
    p = params.to_c()
    buf = torch.full((16,), 7.0, device="cuda")
    assert _raw(dt._h, [cams[0]], 0, p, C.c_void_p(buf.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (buf == 7.0).all()


@pytest.mark.gpu
def test_33_cameras_in_one_call_equal_33_calls_and_the_model_across_the_chunk_boundary():
    """one more camera than travels in one launch's arguments: frames 0, 31 (the last of the first launch) and 32 (the first of
    the second) against the model, every frame against a call of its own; 67 x 45: partial tiles"""
    tree, D, _, _ = G.shape("B")
    dt = _upload(tree)
    cams = [_rcam(67, 45, p) for p in synth.orbit_poses(33)]
    params = R.GridParams(max_depth=D, line_px=1.5, color=[0.1, 0.2, 0.3], background=0.5)

    def model(f):
        wd, wc = G.grid_layers(tree, [cams[f]], D, 1.5, color=(0.1, 0.2, 0.3), background=0.5)
        assert np.isfinite(wd).sum() > 500
        return wd[0], wc[0]

    check_33_cameras_in_one_call(lambda c, **kw: R.draw_grid_layers(dt, c, params, **kw), cams, model)


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["wide", "nodew"])
def test_merge_is_the_depth_test_against_what_the_buffers_hold(walk):
    from layers_ref import make_layers
    torch = _torch()
    tree, D, _, _ = G.shape("B")
    dt = _upload(tree, walk)
    W, H = 100, 76
    cams = [_rcam(W, H, synth.orbit_poses(16)[p]) for p in (0, 5)]
    old_d, old_c = make_layers(tree, cams)  # a tilted plane through the volume, +inf rows, 0 / negative / NaN pixels
    with np.errstate(invalid="ignore"):
        assert np.isinf(old_d).any() and (old_d == 0).any() and (old_d < 0).any() and np.isnan(old_d).any()
    params = R.GridParams(max_depth=D, line_px=2.0, color=[0.0, 1.0, 0.0], background=0.3)
    new_d, new_c = G.grid_layers(tree, cams, D, 2.0, color=(0.0, 1.0, 0.0), background=0.3)
    want_d, want_c = G.merge_layers(new_d, new_c, old_d, old_c)
    with np.errstate(invalid="ignore"):
        taken = np.isfinite(new_d) & (old_d > new_d)
        dead = ~(old_d > 0)
    assert taken.sum() > 500 and (np.isfinite(new_d) & ~taken & ~dead).sum() > 500 and (np.isfinite(new_d) & dead).sum() > 5
    d, c = torch.from_numpy(old_d).cuda(), torch.from_numpy(old_c).cuda()
    R.draw_grid_layers(dt, cams, params, depth=d, color=c, merge=True)
    torch.cuda.synchronize()
    assert_bits_equal(d.cpu().numpy(), want_d, "merged depth (untouched pixels keep their bytes)")
    assert_bits_equal(c.cpu().numpy(), want_c, "merged colour")
    # depth alone
    d = torch.from_numpy(old_d).cuda()
    R.draw_grid_layers(dt, cams, params, depth=d, color=False, merge=True)
    torch.cuda.synchronize()
    assert_bits_equal(d.cpu().numpy(), want_d, "merged depth without a colour buffer")


def _e2e_scene():
    from test_rays import _small
    tree = _small()  # SH9, depth 6
    W, H = 64, 48
    cams = [_rcam(W, H, synth.orbit_poses(4)[p]) for p in (1, 2)]
    return tree, W, H, cams


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
@pytest.mark.parametrize("spp", [1, 6])
def test_render_over_the_drawn_layers_single_frame(spp, kernel):
    import orc
    from layers_ref import expected_rgba
    from test_rays import _frame_planes
    tree, W, H, cams = _e2e_scene()
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    dt = _upload(tree)
    opt = R.RenderOptions(spp=spp, denoise=False, show_grid=True, grid_max_depth=2, background_brightness=0.8)
    ctx = R.RenderContext(W, H)
    ctx.rng_seed()
    ctx.rng_advance()
    ctx.set_kernel(kernel)
    d, c = ctx.show_grid(dt, cams[0], opt)
    assert ctx.layers() == (d.data_ptr(), c.data_ptr()) and not ctx.offscreen
    R.launch_renderer(dt, cams[0], opt, ctx, offscreen=False)
    aux = ctx.download_aux()
    want_d, want_c = G.grid_layers(tree, cams[:1], 2, 1.0, background=0.8)
    assert_bits_equal(d.cpu().numpy(), want_d, "the layers show_grid drew: depth")
    assert_bits_equal(c.cpu().numpy(), want_c, "the layers show_grid drew: colour")
    want = expected_rgba(ht, cams[0], spp, want_d[0], want_c[0], rng_base=orc.rng(frame=1), bg=0.8)
    assert_bits_equal(_frame_planes(aux), want, "frame over the grid vs the per-ray oracle")
    assert (want[np.isfinite(want_d[0]).reshape(-1), 3] < 1).any()  # the grid shows through the volume somewhere


@pytest.mark.gpu
def test_render_over_the_drawn_layers_batched():
    import orc
    from layers_ref import expected_rgba
    from test_rays import _frame_planes
    torch = _torch()
    tree, W, H, cams = _e2e_scene()
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    dt = _upload(tree)
    opt = R.RenderOptions(spp=6, denoise=False, show_grid=True, grid_max_depth=2)
    ctx = R.RenderContext(W, H, frames=2)
    ctx.rng_seed()
    ctx.show_grid(dt, cams, opt)
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[3, 1])
    torch.cuda.synchronize()
    aux = torch.as_tensor(ctx.batch_views()[0], device="cuda:0").cpu().numpy()
    want_d, want_c = G.grid_layers(tree, cams, 2, 1.0)
    for f, jump in enumerate((3, 1)):
        want = expected_rgba(ht, cams[f], 6, want_d[f], want_c[f], rng_base=orc.rng(frame=jump))
        assert_bits_equal(_frame_planes(aux[f]), want, "batched frame %d over the grid vs the per-ray oracle" % f)


@pytest.mark.gpu
def test_cli_grid_writes_what_the_python_route_renders(tmp_path):
    """volrend_headless --grid 2 -o: the PNGs of the per-frame loop and of the batched loop decode to the RGBA8 of
    RenderContext.show_grid + launch_renderer with the CLI's per-pose RNG"""
    from PIL import Image
    tree = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(2)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    op = synth.write_opt_json(str(tmp_path / "opt.json"), denoise=False, spp=6)
    W, H = 96, 64
    dt = _upload(tree)
    opt = R.RenderOptions.from_json(op)
    opt.show_grid, opt.grid_max_depth = True, 2
    want = []
    for i in range(2):
        ctx = R.RenderContext(W, H)
        ctx.rng_seed()
        for _ in range(i):
            ctx.rng_advance()
        cam = _rcam(W, H, poses[i])
        ctx.show_grid(dt, cam, opt)
        R.launch_renderer(dt, cam, opt, ctx)
        want.append(ctx.download_rgba8())
    plain = R.RenderContext(W, H)
    plain.rng_seed()
    R.launch_renderer(dt, _rcam(W, H, poses[0]), opt, plain)
    assert (plain.download_rgba8() != want[0]).any(2).sum() > 200  # the grid is in the picture
    for batch in ("1", "2"):
        out = str(tmp_path / ("out" + batch))
        r = subprocess.run([BIN, tp, pp, "--options", op, "-w", str(W), "-h", str(H), "-o", out, "--warmup", "0", "--batch", batch,
                            "--grid", "2"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        for i in range(2):
            got = np.array(Image.open(os.path.join(out, "r_%d.png" % i)))
            assert got.shape == (H, W, 4) and np.array_equal(got, want[i]), (batch, i)


@pytest.mark.gpu
def test_refusals_leave_the_buffers_untouched(tmp_path):
    torch = _torch()
    from test_query import _n4_tree
    tree, D, _, _ = G.shape("B")
    dt = _upload(tree)
    cam = _rcam(40, 30, synth.orbit_poses(16)[0])
    depth = torch.full((2, 30, 40), 3.25, device="cuda")
    color = torch.full((2, 30, 40, 4), -7.5, device="cuda")
    dp, cp = C.c_void_p(depth.data_ptr()), C.c_void_p(color.data_ptr())
    for what, call in _invalid_calls(dt._h, cam, dp, cp):
        assert call() == E_INVALID, what
    ok = R.GridParams(max_depth=D).to_c()
    # RTO_E_UNSUPPORTED: an NDC tree, N != 2  (a tree with neither a traversal image nor child[] resident cannot be uploaded)
    ndc = _upload(tree)
    ndc.set_ndc(40.0, 30.0, 35.0)
    assert _raw(ndc._h, [cam], 1, ok, dp, cp) == E_UNSUPPORTED and "NDC" in R.lib().rto_last_error().decode()
    n4 = _n4_tree()
    d4 = R.N3Tree.from_arrays(n4.child, n4.data, n4.scale, n4.offset, n4.data_format)
    assert _raw(d4._h, [cam], 1, ok, dp, cp) == E_UNSUPPORTED and "N != 2" in R.lib().rto_last_error().decode()
    with pytest.raises(R.RtoError) as e:
        R.draw_grid_layers(ndc, [cam], R.GridParams(max_depth=D))
    assert e.value.code == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (depth == 3.25).all() and (color == -7.5).all(), "a refused call wrote to its buffers"
    # max_depth above 22 is clamped, not refused; a quantised tree loaded with RTO_TREE_QUANT_DIRECT draws like the expanded one
    assert _raw(dt._h, [cam], 1, R.GridParams(max_depth=1000).to_c(), dp, cp) == 0
    path = str(tmp_path / "quant.npz")
    tree.save_quant_npz(path, n_retain=1, quantiser="luminance")
    qd, ex = R.N3Tree(path, quant_direct=True), R.N3Tree(path)
    a, b = R.draw_grid_layers(qd, [cam], R.GridParams(max_depth=D)), R.draw_grid_layers(ex, [cam], R.GridParams(max_depth=D))
    want_d, want_c = G.grid_layers(tree, [cam], D, 1.0)
    for got in (a, b):
        assert_bits_equal(got[0].cpu().numpy(), want_d, "quantised tree: depth")
        assert_bits_equal(got[1].cpu().numpy(), want_c, "quantised tree: colour")
