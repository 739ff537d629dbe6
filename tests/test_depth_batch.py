"""Depth outputs from the batched kernels: rto_ctx_enable_depth(ctx, RTO_DEPTH_BATCHED) (include/rto.h "depth outputs").

The expectation throughout is mode 1 -- rto_ctx_enable_depth(ctx, 1), a batch rendered frame by frame through the single-frame depth
kernels -- on the same inputs: tests/test_depth.py pins that route to the CPU oracle's reconstruction, and mode 2 promises its bytes.
Every comparison is bit for bit on aux, image, depth and t_near.  One test (the anchor) goes to the reconstruction directly."""
import ctypes as C
import inspect
import os
import shutil

import numpy as np
import pytest

import depth_ref as D
import orc
import rt_octree_amd as R
from helpers import FRAME_ANISO, assert_bits_equal, cameras, reframe, reframe_pose
from rt_octree_amd import _lib, synth
from test_depth import E_UNSUPPORTED, H, W, _check_against, _poses, _slot_outputs
from test_rays import _cam, _dev, _small, _tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
JUMPS = [4, 1, 7]
WHAT = ("aux", "image", "depth", "t_near")


# ------------------------------------------------------------------ CPU


def test_depth_batch_codegen():
    """every <SPP, WIDE, STACK> form of render_persist_depth exists exactly once in depth_kernels.hip, keeps a private segment no larger
    than its sibling render_persist_layers (render_kernels.hip) and at most one wave per SIMD less -- against the sibling of the same
    build, no absolute number"""
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc is needed to cross-compile the kernels")
    from test_codegen import kernel_resources, render_resources
    old = render_resources()
    new = kernel_resources("depth_kernels.hip")
    assert not [n for n in old if "render_persist_depth" in n]
    forms = 0
    for spp in (1, 2, 3, 4, 6, 8, 16, 32):
        for wide, stack in ((1, 1), (1, 0), (0, 0)):
            args = "ILi%dELi32ELi8ELb%dELi%dEEE" % (spp, wide, stack)
            mine = [v for n, v in new.items() if n.startswith("_ZN3rto20render_persist_depth" + args)]
            sib = [v for n, v in old.items() if n.startswith("_ZN3rto21render_persist_layers" + args)]
            assert len(mine) == 1 and len(sib) == 1, (args, len(mine), len(sib))
            print("render_persist_depth%s: %s  sibling: %s" % (args, mine[0], sib[0]))
            assert mine[0]["scratch"] <= sib[0]["scratch"], (args, mine[0], sib[0])
            assert mine[0]["occupancy"] >= sib[0]["occupancy"] - 1, (args, mine[0], sib[0])
            forms += 1
    assert forms == 24 and len([n for n in new if "render_persist_depth" in n]) == 24  # (the default tuning only)


def test_exports_and_the_batched_switch():
    header = open(os.path.join(ROOT, "include", "rto.h")).read()
    assert "#define RTO_DEPTH_BATCHED 2" in header
    L = R.lib()  # (raises when a declared symbol is missing)
    for name in _lib.SYMBOLS:
        assert hasattr(L, name), name
    assert "batched" in inspect.signature(R.RenderContext.enable_depth).parameters
    assert hasattr(R.RenderContext, "depth_mode") and R.DEPTH_BATCHED == 2
    assert L.rto_ctx_depth_enabled(None) == 0 and L.rto_ctx_enable_depth(None, 2) == -1


# ------------------------------------------------------------------ GPU


def _ctx(mode, w=W, h=H, frames=3, tuning=(), layers=None, lean=0):
    """a context with depth outputs in `mode` (0: none)"""
    ctx = R.RenderContext(w, h, frames=frames)
    ctx.rng_seed()
    if mode:
        ctx.enable_depth(batched=mode == 2)
        assert ctx.depth_mode() == mode and ctx.depth_enabled()
    for k, v in tuning:
        ctx.set_tuning(k, v)
    if layers is not None:
        ctx.set_layers(*layers)
    if lean:
        ctx.set_lean_outputs(lean)
    return ctx


def _render(dt, cams, spp, mode, jumps=JUMPS, denoise=False, **kw):
    """the batch in `mode` -> (context, [(aux, image, depth, t_near) per frame])"""
    ctx = _ctx(mode, cams[0].width, cams[0].height, frames=kw.pop("frames", len(cams)), **kw)
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=spp, denoise=denoise), ctx, rng_jumps=jumps[:len(cams)])
    return ctx, [_slot_outputs(ctx, f) for f in range(len(cams))]


def _same(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        for x, y, name in zip(a, b, WHAT):
            assert_bits_equal(x, y, "%s, frame %d: %s" % (what, f, name))


def _two_modes(dt, cams, spp, marks=True, min_hit=200, **kw):
    """mode 2 == mode 1 on the same inputs; -> (mode-2 context, mode-1 outputs)"""
    _, want = _render(dt, cams, spp, 1, **kw)
    for f, o in enumerate(want):  # (not a vacuous pass: decided on the mode-1 frames)
        print("frame %d: %d pixels with a finite t_near (asked: > %d)" % (f, int(np.isfinite(o[3]).sum()), min_hit))
        assert np.isfinite(o[3]).sum() > min_hit, (f, int(np.isfinite(o[3]).sum()))
    ctx, got = _render(dt, cams, spp, 2, **kw)
    _same(got, want, "mode 2 vs mode 1 (spp %d)" % spp)
    assert (ctx.tile_marks() is not None) == marks  # (the persistent kernels ran)
    return ctx, want


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 6, 32])
def test_a_mode_2_batch_equals_the_mode_1_batch(spp):
    dt = _dev(_small())
    _, want = _two_modes(dt, _poses(3), spp)
    if spp == 6:
        for f, o in enumerate(want):  # (pixels whose sum has more than one term)
            assert (o[0][3] >= f32(2.0 / 6.0)).sum() >= 50, f


@pytest.mark.gpu
def test_culling_changes_no_byte():
    t = _small()
    dt = _dev(t)
    cams = _poses(3)
    # the pose: at least a quarter of the 8x8 tiles hold no pixel with alpha, at least a quarter hold one (the CPU oracle)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    for cam, jump in zip(cams, JUMPS):
        ocam = orc.camera(W, H, cam.fx, cam.fy, cam.transform.reshape(-1))
        alpha = orc.render_frame(ht, ocam, orc.default_options(spp=6), orc.rng(frame=jump))[0][3]
        tiles = [(alpha[y:y + 8, x:x + 8] == 0).all() for y in range(0, H, 8) for x in range(0, W, 8)]
        assert 4 * sum(tiles) >= len(tiles) and 4 * (len(tiles) - sum(tiles)) >= len(tiles), (sum(tiles), len(tiles))
    outs = {}
    for cull in (0, 1):
        ctx, outs[cull] = _render(dt, cams, 6, 2, tuning=(("cull", cull),))
        live, every = ctx.queue_stats()
        assert (0 < live < every) if cull else (live == every), (cull, live, every)
    _same(outs[1], outs[0], "cull 1 vs cull 0")
    _same(outs[1], _render(dt, cams, 6, 1)[1], "cull 1 vs mode 1")


@pytest.mark.gpu
def test_the_three_image_forms_and_other_tree_formats():
    cams = _poses(3)
    _two_modes(_dev(_tree("SH", 9), compact_records=True), cams, 6, tuning=(("wide_bits", 6),))  # one-level image
    from test_render_parity import _chain_tree
    deep = _dev(_chain_tree(13, seed=13))  # four pairs of levels below the grid: the ancestor stack in LDS rows
    assert (deep.max_depth - 6 + 1) // 2 > 2 and deep.wide_nodes > 0
    dcams = [cameras(56, 40, synth.look_at_c2w(eye, target=(0.0, -0.1, 0.05)))[1]
             for eye in ((2.2, 1.7, 1.9), (2.0, 1.9, 1.7), (2.4, 1.5, 2.0))]
    # (min_hit: another tree and a smaller frame than the issue's 200 is stated for; 100 is the guard tests/test_depth.py sets for
    #  this tree and this camera)
    _two_modes(deep, dcams, 6, min_hit=100)
    _two_modes(_dev(_tree("SG", 16)), cams, 6)
    _two_modes(_dev(_tree("RGBA", -1)), cams, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["depth", "color", "both"])
def test_layers(which):
    from layers_ref import make_layers
    t = _small()
    dt = _dev(t)
    cams = _poses(3)
    layer_depth, layer_color = make_layers(t, cams)
    layers = (layer_depth if which != "color" else None, layer_color if which != "depth" else None)
    # (min_hit: the depth layer cuts the object in half and rows 20..25 of it lie in front of the whole volume, so fewer pixels
    #  keep a hit than offscreen; 100 is what tests/test_depth.py asks of a frame over these layers)
    _, want = _two_modes(dt, cams, 6, marks=which == "depth", min_hit=100, layers=layers)
    if which != "color":  # (the layer cuts the object in half)
        _, plain = _render(dt, cams, 6, 1)
        for f in range(3):
            assert (want[f][3] != plain[f][3]).sum() > 50, f


@pytest.mark.gpu
def test_ndc_tree_and_reframed_tree():
    t = _small()
    ndc = _dev(t)
    ndc.set_ndc(float(W), float(H), 40.0)
    # (min_hit: the NDC warp moves the volume in the frame; 20 is the guard tests/test_depth.py sets for this NDC frame)
    ctx, _ = _two_modes(ndc, _poses(3), 4, min_hit=20)
    live, every = ctx.queue_stats()
    assert live == every  # (no culling over the NDC warp)
    t2 = reframe(t, *FRAME_ANISO)
    cams2 = [cameras(W, H, reframe_pose(synth.orbit_poses(4)[i], t, t2))[1] for i in range(3)]
    _two_modes(_dev(t2), cams2, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
def test_lean_outputs(level):
    import torch
    from rt_octree_amd import denoiser
    dt = _dev(_small())
    cams = _poses(3)
    torch.manual_seed(3)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval())
    _, full = _render(dt, cams, 6, 2, denoise=True)

    def noisy_and_denoised(ctx):
        assert ctx.frames_lean_level(0, 3) == level and ctx.tile_marks() is not None
        noisy = torch.as_tensor(ctx.batch_views()[1], device="cuda:0").clone().cpu().numpy()
        ctx.select_frame(0)
        net.denoise(ctx, n=3, mode=R.FILTER_FAST)
        torch.cuda.synchronize()
        return noisy, torch.as_tensor(ctx.batch_views()[2], device="cuda:0").clone().cpu().numpy()

    outs = {}
    for mode in (0, 2):
        ctx = _ctx(mode, lean=level)
        if level == 2:  # (nothing is stored for culled tiles: the same bytes underneath in both contexts)
            for v in ctx.batch_views()[1:]:
                torch.as_tensor(v, device="cuda:0").fill_(-7.0)
        R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=True), ctx, rng_jumps=JUMPS)
        outs[mode] = noisy_and_denoised(ctx)
        if mode == 2:
            for f in range(3):
                ctx.select_frame(f)
                depth, t_near = ctx.download_depth()
                assert_bits_equal(depth, full[f][2], "lean %d, frame %d: depth vs the full-output launch" % (level, f))
                assert_bits_equal(t_near, full[f][3], "lean %d, frame %d: t_near vs the full-output launch" % (level, f))
    assert_bits_equal(outs[2][0], outs[0][0], "lean %d: the noisy image vs a context without depth" % level)
    assert_bits_equal(outs[2][1], outs[0][1], "lean %d: rto_denoise(FACTORISED) vs a context without depth" % level)


@pytest.mark.gpu
def test_the_fill():
    import torch
    t = _small()
    dt = _dev(t)
    cams = _poses(3)
    opt = R.RenderOptions(spp=6, denoise=False)
    ctx = _ctx(2)
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)
    before = [_slot_outputs(ctx, f) for f in range(3)]
    assert all(np.isfinite(o[3]).sum() > 200 for o in before)
    # cameras that look away from the volume: every plane of the launch's slots reads (0, +inf) ...
    away = []
    for i in range(2):
        c2w = np.array(synth.orbit_poses(4)[i], np.float64)
        c2w[:3, 0] *= -1.0  # (turned about its up axis: the volume is behind it)
        c2w[:3, 2] *= -1.0
        cam = R.Camera(W, H, cams[0].fx, cams[0].fy)
        cam.set_c2w(c2w)
        away.append(cam)
    R.launch_renderer_batch(dt, away, opt, ctx, rng_jumps=JUMPS[:2])
    for f in range(2):
        _, _, depth, t_near = _slot_outputs(ctx, f)
        assert (depth.view(np.uint32) == 0).all() and np.isposinf(t_near).all(), f
    # ... and the slot outside the launch keeps its contents
    after = _slot_outputs(ctx, 2)
    assert_bits_equal(after[2], before[2][2], "slot 2 of a 2-frame launch: depth")
    assert_bits_equal(after[3], before[2][3], "slot 2 of a 2-frame launch: t_near")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("hook", [1, 2])
def test_fallbacks(hook):
    dt = _dev(_small())
    cams = _poses(3)
    _, want = _render(dt, cams, 6, 1)
    ctx, got = _render(dt, cams, 6, 2, tuning=(("batch_fallback", hook),))
    _same(got, want, "batch_fallback %d in mode 2 vs mode 1" % hook)
    assert ctx.tile_marks() is None
    for level in (1, 2):
        ctx.set_lean_outputs(level)
        with pytest.raises(R.RtoError) as e:
            R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=True), ctx, rng_jumps=JUMPS)
        assert e.value.code == E_UNSUPPORTED, e.value
    ctx.set_lean_outputs(0)
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=False), ctx, rng_jumps=JUMPS)
    _same([_slot_outputs(ctx, f) for f in range(3)], want, "after the refusals")
    ctx.set_tuning("batch_fallback", 0)
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=False), ctx, rng_jumps=JUMPS)
    assert ctx.tile_marks() is not None
    _same([_slot_outputs(ctx, f) for f in range(3)], want, "the hook off again")


@pytest.mark.gpu
def test_mode_switching_and_refusals(tmp_path):
    dt = _dev(_small())
    cams = _poses(3)
    opt = R.RenderOptions(spp=6, denoise=False)
    L = R.lib()
    ctx = _ctx(2)
    ptr = L.rto_ctx_depth(ctx._h)
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)
    first = [_slot_outputs(ctx, f) for f in range(3)]
    assert ctx.tile_marks() is not None
    ctx.select_frame(0)
    ctx.enable_depth()  # 2 -> 1
    assert ctx.depth_mode() == 1 and L.rto_ctx_depth(ctx._h) == ptr
    assert_bits_equal(ctx.download_depth()[0], first[0][2], "the planes survive a mode switch")
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)
    assert ctx.tile_marks() is None
    _same([_slot_outputs(ctx, f) for f in range(3)], first, "mode 1 after mode 2 on one context")
    ctx.select_frame(0)
    ctx.enable_depth(batched=True)  # 1 -> 2
    assert ctx.depth_mode() == 2 and L.rto_ctx_depth(ctx._h) == ptr
    for _ in range(2):  # (and a repeat gives the same bytes)
        R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)
        assert ctx.tile_marks() is not None
        _same([_slot_outputs(ctx, f) for f in range(3)], first, "mode 2 again")
    # any other non-zero value is mode 1
    _lib.check(L.rto_ctx_enable_depth(ctx._h, 5))
    assert ctx.depth_mode() == 1 and L.rto_ctx_depth_enabled(ctx._h) == 1
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)
    assert ctx.tile_marks() is None
    five = R.RenderContext(W, H)
    _lib.check(L.rto_ctx_enable_depth(five._h, 5))
    assert five.depth_mode() == 1
    # what depth outputs refuse, they refuse in mode 2
    ctx.enable_depth(batched=True)

    def refused(fn):
        with pytest.raises(R.RtoError) as e:
            fn()
        assert e.value.code == E_UNSUPPORTED, e.value

    refused(lambda: R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=False, enable_probe=True), ctx, rng_jumps=JUMPS))
    ctx.enable_stats(True)
    refused(lambda: R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS))
    ctx.enable_stats(False)
    path = str(tmp_path / "quant.npz")
    _small(basis=9, seed=11).save_quant_npz(path, n_retain=1, quantiser="luminance")
    q = R.N3Tree(path, quant_direct=True)
    refused(lambda: R.launch_renderer_batch(q, cams, opt, ctx, rng_jumps=JUMPS))
    refused(lambda: R.launch_renderer(q, cams[0], opt, ctx))
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=JUMPS)  # (and nothing above left the context unusable)
    _same([_slot_outputs(ctx, f) for f in range(3)], first, "after the refusals")
    ctx.enable_depth(False)
    assert ctx.depth_mode() == 0 and not ctx.depth_enabled() and L.rto_ctx_depth(ctx._h) is None


@pytest.mark.gpu
def test_frame_0_against_the_reconstruction():
    """the one anchor outside the library: rows 16..25 of frame 0 of a mode-2 batch against depth_ref's reconstruction from the CPU
    oracle, with test_depth's derived bound ((4 + SPP) 2^-23 relative for depth, 3 ulp for t_near).  SPP 4 and 4 RNG jumps: the frame's
    RNG is then the oracle's default advanced by a whole number of rays, 4 * 2^32 / 4 = 2^32 of them."""
    spp = 4
    t = _small()
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    cams = _poses(3)
    _, got = _render(_dev(t), cams, spp, 2)
    o, d = R.camera_rays(cams[0])
    lo, hi = 16 * W, 26 * W
    hits, _ = D.reconstruct(ht, np.ascontiguousarray(o[lo:hi]), np.ascontiguousarray(d[lo:hi]), spp, first_ray=(1 << 32) + lo)
    want_depth, want_near = D.expectation(hits, spp)
    assert sum(1 for h in hits if h) > 100 and sum(1 for h in hits if len(h) >= 2) > 25
    _check_against(got[0][2].reshape(-1)[lo:hi], got[0][3].reshape(-1)[lo:hi], want_depth, want_near, spp, "frame 0 of a mode-2 batch")


@pytest.mark.gpu
def test_cli_write_depth_renders_batches(tmp_path):
    """--write_depth no longer forces one launch per frame: the binary reports the 3 poses per launch it was asked for, and the
    planes it writes are mode 1's"""
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
    assert "INFO: 3 poses per launch" in r.stdout, r.stdout
    fx = synth.blender_focal(W)
    cams = []
    for i in range(3):
        cam = R.Camera(W, H, fx, fx)
        cam.set_c2w(poses[i])
        cams.append(cam)
    _, want = _render(_dev(tree), cams, 6, 1, jumps=[2, 3, 4])
    for i in range(3):
        got = np.fromfile(os.path.join(out, "depth_r_%d.bin" % i), f32).reshape(2, H, W)
        assert_bits_equal(got[0], want[i][2], "depth_r_%d.bin: depth" % i)
        assert_bits_equal(got[1], want[i][3], "depth_r_%d.bin: t_near" % i)
        assert np.isfinite(got[1]).sum() > 200


def _n4_tree():
    """a small N = 4 tree (no traversal image: the persistent kernels cannot take it): the root, two of its 64 cells refined, one of
    those refined once more; half the leaves dense"""
    rng = np.random.default_rng(2)
    child = np.zeros((4, 4, 4, 4), np.int32)
    child[0, 1, 2, 3] = 1
    child[0, 3, 0, 1] = 2
    child[2, 0, 3, 2] = 1
    data = rng.normal(0, 1, (4, 4, 4, 4, 28)).astype(np.float16)
    data[..., -1] = np.abs(data[..., -1]) * (rng.uniform(0, 1, (4, 4, 4, 4)) < 0.5)
    return synth.SynthTree(child, data, np.array((0.4, 0.3, 0.5), f32), np.array((0.5, 0.45, 0.55), f32), "SH9", 3, {})


@pytest.mark.gpu
def test_cli_write_depth_on_a_tree_the_persistent_kernels_cannot_take(tmp_path):
    """the CLI's default configuration -- denoise on, the fused network, a batch: lean outputs -- with --write_depth on an N = 4
    tree: the batch goes frame by frame, which stores full outputs only; the CLI must fall back to those and still write every
    PNG and every depth file, the planes being mode 1's"""
    import subprocess
    import torch
    from rt_octree_amd import denoiser
    from test_cli import BIN
    w, h = 64, 48
    tree = _n4_tree()
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(3)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    torch.manual_seed(0)
    ts = denoiser.compact_and_compile(denoiser.GuidanceNet(8, 32, 5, 2, 4), device="cuda:0", example_hw=(h, w))
    tsp = str(tmp_path / "ts_latest.ts")
    ts.save(tsp)
    op = synth.write_opt_json(str(tmp_path / "opt.json"))  # spp 6, denoise true
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, tp, pp, "--options", op, "--ts_module", tsp, "-w", str(w), "-h", str(h), "-o", out, "--warmup", "2",
                        "--batch", "3", "--write_depth"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "GuidanceNet runs as the fused HIP kernel" in r.stdout and "INFO: 3 poses per launch" in r.stdout
    dt = _dev(tree)
    assert dt.N == 4
    fx = synth.blender_focal(w)
    cams = []
    for i in range(3):
        cam = R.Camera(w, h, fx, fx)
        cam.set_c2w(poses[i])
        cams.append(cam)
    _, want = _render(dt, cams, 6, 1, jumps=[2, 3, 4], denoise=True)
    for i in range(3):
        assert os.path.getsize(os.path.join(out, "r_%d.png" % i)) > 0
        got = np.fromfile(os.path.join(out, "depth_r_%d.bin" % i), f32).reshape(2, h, w)
        assert_bits_equal(got[0], want[i][2], "N = 4, depth_r_%d.bin: depth" % i)
        assert_bits_equal(got[1], want[i][3], "N = 4, depth_r_%d.bin: t_near" % i)
        assert np.isfinite(got[1]).sum() > 1000  # (the CPU oracle finds 2600-2800 pixels with alpha in each of these frames)
