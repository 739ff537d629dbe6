"""The operator's probe (enable_probe, volrend.cu:100-134, 215-231, 244-251): a launch with the probe on equals the same launch
without it outside the lumisphere's disc, and tests/probe_ref.py's float32 restatement inside it, bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import probe_ref
import rt_octree_amd as R
from rt_octree_amd import synth

E_INVALID, E_UNSUPPORTED = -1, -3
f32 = np.float32
SIZES = ((64, 48), (50, 37))
DISPS = (1, 7, 16, 100)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ no device needed: the restatement against hand-computed pixels
class _Host:
    """what probe_ref reads of an orc.HostTree, for a one-node tree"""

    def __init__(self, data_row, data_format):
        import orc
        child = np.zeros((1, 2, 2, 2), np.int32)
        data = np.tile(np.asarray(data_row, np.float16), (1, 2, 2, 2, 1))
        self.ht = orc.HostTree(child, data, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), data_format)


IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
# disp 4 in a 16 x 12 frame: x >= 7, y < 9; xx = x - 7, yy = y - 5; cen0 = 1 - xx / 2, cen1 = yy / 2 - 1.  c <= 1 holds for
# (cen0, cen1) in {0, +-.5, +-1}^2 with cen0^2 + cen1^2 <= 1: the centre, 4 + 4 at distance .5 / sqrt(.5), 4 at distance 1
DISC_4 = {(9, 7)} | {(9 + dx, 7 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)} | {(7, 7), (11, 7), (9, 5), (9, 9)}


def test_probe_ref_membership_of_a_size_4_probe():
    mask, cen0, cen1, c = probe_ref.disc(16, 12, 4)
    assert {(int(x), int(y)) for y, x in zip(*np.nonzero(mask))} == {p for p in DISC_4 if p[1] < 9} == DISC_4 - {(9, 9)}
    # (9, 9) has c = 1 but fails y < disp + 5: the disc's lowest pixel is cut by the reference's own condition
    assert cen0[7, 9] == 0 and cen1[7, 9] == 0 and c[7, 7] == 1 and c[6, 8] == f32(0.5)
    # clipped by the image: a probe larger than the frame
    big, _, _, _ = probe_ref.disc(64, 48, 100)
    assert big.shape == (48, 64) and big[47, 0] and big[30, 20] and not big[0, 0] and not big[0, 63]
    assert not probe_ref.disc(16, 12, 100)[0].any() and not probe_ref.disc(64, 48, 1)[0].any()  # (no pixel has c <= 1 there)


def test_probe_ref_colours_of_a_size_4_probe():
    # RGBA: the first three coefficients as they are
    rgba = _Host([0.25, 0.5, 0.75, 3.0], "RGBA").ht
    mask, rgb = probe_ref.colours(rgba, (0.3, 0.3, 0.3), IDENTITY, 16, 12, 4)
    assert mask.sum() == 12 and np.array_equal(rgb, np.tile(np.array([0.25, 0.5, 0.75], f32), (12, 1)))
    # SH4, the centre pixel: dir = M (0, 0, -1).  Channel 0 all zero -> tmp = 0 -> 1 / (1 + 1) = 0.5; channel 1 DC = 1000 ->
    # tmp = 282.09 -> expf(-tmp) = 0 -> 1; channel 2 DC = -1000 -> expf(282.09) = inf -> 0
    row = np.zeros(13, np.float16)
    row[4], row[8], row[12] = 1000.0, -1000.0, 2.0
    sh4 = _Host(row, "SH4").ht
    mask, rgb = probe_ref.colours(sh4, (0.3, 0.3, 0.3), IDENTITY, 16, 12, 4)
    centre = int(np.flatnonzero((np.argwhere(mask) == (7, 9)).all(1))[0])
    assert np.array_equal(rgb[centre], np.array([0.5, 1.0, 0.0], f32))
    aux, img = probe_ref.outputs(rgb[centre:centre + 1])
    assert np.array_equal(aux[0], np.array([0.5, 1, 0, 1, 0.25, 1, 0, 1], f32)) and np.array_equal(img[0], np.array([0.5, 1, 0, 1], f32))
    # with basis_minmax = {1, 3} the DC terms drop out: every channel 0.5
    _, rgb = probe_ref.colours(sh4, (0.3, 0.3, 0.3), IDENTITY, 16, 12, 4, basis_minmax=(1, 3))
    assert np.array_equal(rgb[centre], np.array([0.5, 0.5, 0.5], f32))


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _tree(name):
    from helpers import rgba_tree
    sh9 = synth.make_tree(depth_limit=5, basis_dim=9, seed=7)
    if name in ("sh9", "sh9_minmax"):
        return sh9
    if name == "rgba":
        return rgba_tree(sh9)
    if name == "sg9":
        return synth.with_lobes(sh9, "SG", seed=2)
    return synth.make_tree(depth_limit=4 if name == "sh25" else 5, basis_dim=int(name[2:]), seed=7)


def _pair(tree):
    import orc
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    dt = R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra)
    return ht, dt


def _probe_points(tree):
    """inside a dense leaf, inside an empty one, outside the box (clamped)"""
    dd = tree.data.shape[-1]
    sig = tree.data.reshape(-1, dd)[:, -1].astype(f32)
    leaf = tree.child.reshape(-1) == 0
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.4, 1.4, (4000, 3)).astype(f32)
    import orc
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    dense = empty = None
    for p in pts:
        xyz = (ht.offset + ht.scale * p).astype(f32)
        buf, cs, lv = (C.c_float * 3)(*[float(v) for v in xyz]), C.c_float(), C.c_int()
        slot = orc.lib().orc_query(C.byref(ht.c), buf, C.byref(cs), C.byref(lv))
        assert leaf[slot]
        if sig[slot] > 0 and dense is None:
            dense = p
        if sig[slot] == 0 and empty is None:
            empty = p
        if dense is not None and empty is not None:
            break
    assert dense is not None and empty is not None
    return [tuple(float(v) for v in dense), tuple(float(v) for v in empty), (9.0, -7.5, 0.2)]


def _camera(W, H, k=1):
    from helpers import cameras
    return cameras(W, H, synth.orbit_poses(5)[k])[1]


def _render(dt, cam, ctx, kernel, **optkw):
    ctx.rng_seed()
    ctx.set_kernel(kernel)
    opt = R.RenderOptions(**optkw)
    R.launch_renderer(dt, cam, opt, ctx)
    return ctx.download_aux(), ctx.download_image(noisy=bool(optkw.get("denoise")))


def _check_frame(aux, img, aux0, img0, mask, rgb, what):
    out = ~mask
    assert np.array_equal(_bits(aux)[:, out], _bits(aux0)[:, out]), what + ": a pixel outside the disc changed (aux)"
    assert np.array_equal(_bits(img)[out], _bits(img0)[out]), what + ": a pixel outside the disc changed (image)"
    eaux, eimg = probe_ref.outputs(rgb)
    assert np.array_equal(_bits(aux[:, mask].T), _bits(eaux)), what + ": disc pixels differ from probe_ref (aux)"
    assert np.array_equal(_bits(img[mask]), _bits(eimg)), what + ": disc pixels differ from probe_ref (image)"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sh9", "sh16", "sh25", "rgba", "sg9", "sh9_minmax"])
def test_single_frame_probe(name):
    tree = _tree(name)
    ht, dt = _pair(tree)
    minmax = (1, 3) if name == "sh9_minmax" else (0, 24)
    points = _probe_points(tree)
    for (W, H) in SIZES:
        cam = _camera(W, H)
        ctx = R.RenderContext(W, H)
        base = {}
        refs = {(d, p): probe_ref.colours(ht, p, cam.transform.reshape(-1), W, H, d, minmax, tree.extra) for d in DISPS for p in points}
        assert refs[(100, points[0])][0].sum() > refs[(16, points[0])][0].sum() > refs[(7, points[0])][0].sum() > 0
        for spp in (1, 6):
            for denoise in (False, True):
                for kernel in (R.KERNEL_GENERIC, R.KERNEL_FAST):
                    kw = dict(spp=spp, denoise=denoise, basis_minmax=list(minmax))
                    base = _render(dt, cam, ctx, kernel, **kw)
                    for (d, p), (mask, rgb) in refs.items():
                        aux, img = _render(dt, cam, ctx, kernel, enable_probe=True, probe=list(p), probe_disp_size=d, **kw)
                        _check_frame(aux, img, base[0], base[1], mask, rgb,
                                     "%s %dx%d disp %d point %r spp %d denoise %d kernel %d" % (name, W, H, d, p, spp, denoise, kernel))


@pytest.mark.gpu
def test_batched_probe_marks_denoise_and_lean_levels():
    import torch
    from rt_octree_amd import denoiser
    tree = _tree("sh9")
    ht, dt = _pair(tree)
    W, H = SIZES[1]
    cams = [_camera(W, H, k) for k in (0, 2, 3)]
    p = _probe_points(tree)[0]
    torch.manual_seed(0)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).half().float())
    for d in (7, 100):
        refs = [probe_ref.colours(ht, p, c.transform.reshape(-1), W, H, d) for c in cams]
        plain = R.RenderOptions(spp=6, denoise=True)
        probe = R.RenderOptions(spp=6, denoise=True, enable_probe=True, probe=list(p), probe_disp_size=d)
        for lean in (0, 1):
            ctx0, ctx1 = R.RenderContext(W, H, frames=3), R.RenderContext(W, H, frames=3)
            for c in (ctx0, ctx1):
                c.set_lean_outputs(lean)
            R.launch_renderer_batch(dt, cams, plain, ctx0, rng_jumps=[4, 1, 7])
            R.launch_renderer_batch(dt, cams, probe, ctx1, rng_jumps=[4, 1, 7])
            for f in range(3):
                ctx0.select_frame(f)
                ctx1.select_frame(f)
                mask, rgb = refs[f]
                img0, img1 = ctx0.download_image(noisy=True), ctx1.download_image(noisy=True)
                assert np.array_equal(_bits(img1)[~mask], _bits(img0)[~mask]), (d, lean, f)
                assert np.array_equal(_bits(img1[mask]), _bits(probe_ref.outputs(rgb)[1])), (d, lean, f)
                if not lean:
                    _check_frame(ctx1.download_aux(), img1, ctx0.download_aux(), img0, mask, rgb, "batch frame %d disp %d" % (f, d))
            ctx1.select_frame(0)
            # (c) no tile marks after a probe launch; rto_denoise runs its plain kernels and equals the two-call plain route
            assert ctx1.tile_marks() is None and ctx0.tile_marks() is not None
            z = [C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_float()]
            assert R.lib().rto_ctx_tile_marks(ctx1._h, *[C.byref(v) for v in z]) == E_INVALID
            if lean:
                continue
            for mode in (R.FILTER_EXACT, R.FILTER_FAST):
                net.denoise(ctx1, 3, mode)
                torch.cuda.synchronize()
                for f in range(3):
                    ctx1.select_frame(f)
                    one_call = ctx1.download_image()
                    aux_t = torch.as_tensor(ctx1.aux_view(), device="cuda:0")
                    if mode == R.FILTER_EXACT:
                        w, g = net(aux_t, squares_implied=True)
                        R.filtering(None, w[0].contiguous(), g[0].contiguous(), ctx1.noisy_ptr, ctx1.image_ptr)
                    else:
                        net.forward_packed(aux_t, squares_implied=True)
                        net.filter_packed(ctx1.noisy_ptr, ctx1.image_ptr)
                    torch.cuda.synchronize()
                    assert np.array_equal(_bits(ctx1.download_image()), _bits(one_call)), (d, mode, f)
                ctx1.select_frame(0)
        ctx2 = R.RenderContext(W, H, frames=3)
        ctx2.set_lean_outputs(2)
        with pytest.raises(R.RtoError) as e:
            R.launch_renderer_batch(dt, cams, probe, ctx2)
        assert e.value.code == E_UNSUPPORTED
        R.launch_renderer_batch(dt, cams, plain, ctx2)  # (without the probe the sparse level renders)


@pytest.mark.gpu
def test_probe_refusals(tmp_path):
    import torch
    tree = _tree("sh9")
    _, dt = _pair(tree)
    W, H = SIZES[0]
    cam = _camera(W, H)
    ctx = R.RenderContext(W, H)
    on = dict(spp=1, denoise=False, enable_probe=True)

    def code(fn):
        with pytest.raises(R.RtoError) as e:
            fn()
        return e.value.code

    assert code(lambda: R.launch_renderer(dt, cam, R.RenderOptions(probe_disp_size=0, **on), ctx)) == E_INVALID
    assert code(lambda: R.launch_renderer_batch(dt, [cam], R.RenderOptions(probe_disp_size=-3, **on), ctx)) == E_INVALID
    ctx.enable_stats(True)
    assert code(lambda: R.launch_renderer(dt, cam, R.RenderOptions(**on), ctx)) == E_UNSUPPORTED
    ctx.enable_stats(False)
    depth = torch.full((1, H, W), 2.0, dtype=torch.float32, device="cuda")
    ctx.set_layers(depth=depth)
    assert code(lambda: R.launch_renderer(dt, cam, R.RenderOptions(**on), ctx, offscreen=False)) == E_UNSUPPORTED
    assert "layers" in R.lib().rto_last_error().decode()
    ctx.set_layers()
    path = str(tmp_path / "quant.npz")
    tree.save_quant_npz(path, n_retain=1, quantiser="luminance")
    q = R.N3Tree(path, quant_direct=True)
    assert code(lambda: R.launch_renderer(q, cam, R.RenderOptions(**on), ctx)) == E_UNSUPPORTED
    assert code(lambda: R.launch_renderer_batch(q, [cam], R.RenderOptions(**on), ctx)) == E_UNSUPPORTED
    o = torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    assert code(lambda: R.render_rays(dt, o, o + 1, R.RenderOptions(**on), ctx)) == E_UNSUPPORTED
    cr = R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, compact_records=True)
    assert code(lambda: R.launch_renderer(cr, cam, R.RenderOptions(**on), ctx)) == E_UNSUPPORTED
    assert "RTO_TREE_KEEP_REFERENCE" in R.lib().rto_last_error().decode()
    # cull_single is ignored with the probe on: no marks are left
    ctx.set_tuning("cull_single", 1)
    R.launch_renderer(dt, cam, R.RenderOptions(**on), ctx)
    assert ctx.tile_marks() is None
    R.launch_renderer(dt, cam, R.RenderOptions(spp=1, denoise=False), ctx)
    assert ctx.tile_marks() is not None


@pytest.mark.gpu
def test_cli_probe_flag_and_opt_json_agree(tmp_path):
    import torch
    from rt_octree_amd import denoiser
    BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rt-octree_amd", "bin", "volrend_headless")
    tree = _tree("sh9")
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), synth.orbit_poses(2))
    torch.manual_seed(0)
    ts = denoiser.compact_and_compile(denoiser.GuidanceNet(8, 32, 5, 2, 4), device="cuda:0", example_hw=(48, 64))
    tsp = str(tmp_path / "ts_latest.ts")
    ts.save(tsp)
    p = _probe_points(tree)[0]
    op = synth.write_opt_json(str(tmp_path / "opt.json"), spp=1, enable_probe=True, probe=list(p))
    plain = synth.write_opt_json(str(tmp_path / "plain.json"), spp=1)
    common = [tp, pp, "--ts_module", tsp, "-w", "64", "-h", "48", "--warmup", "1"]

    def run(extra, out):
        r = subprocess.run([BIN] + common + extra + ["-o", str(tmp_path / out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return [open(str(tmp_path / out / ("r_%d.png" % i)), "rb").read() for i in range(2)]

    a = run(["--probe", "%r,%r,%r" % p], "flag")
    b = run(["--options", op], "json")
    c = run(["--options", plain], "plain")
    assert a == b and a != c
    r = subprocess.run([BIN] + common + ["--probe", "0.5,0.5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--probe must be of format" in r.stderr
