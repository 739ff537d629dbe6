"""Trees in world frames other than synth.make_tree's cube centred on the origin: invradius3 with three different values
and a free offset (helpers.FRAMES), as the PlenOctrees of scenes that are not cubic carry them.  The tree-space content
is the same; what changes is every place that maps the world into the tree axis by axis -- the ray set-up
(cen = offset + scale * cen), delta_scale and the depth limit that goes through it, the culling cells' world-space
bounding spheres and the tile marks made from them, the loader's invradius3 / invradius branch.

Every traversal kernel against the CPU oracle bit for bit (SG / ASG: against the restatement of tests/test_sg_asg.py, the
oracle marches but does not shade them), culled against unculled, marked against unmarked denoise, arbitrary rays with
depth limits and backdrops, quantised trees, and the seeded scenes of test_fuzz_parity in random frames."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import orc
import rt_octree_amd as R
from helpers import (ANISO_FRAMES, FRAMES, aim_point, assert_bits_equal, oracle_threads, reframe, reframe_point, reframe_pose,
                     rgba_tree)
from rt_octree_amd import synth

f32 = np.float32


def _tree(fmt, depth=6, seed=7):
    kind = "".join(c for c in fmt if c.isalpha())
    basis = 9 if kind == "RGBA" else int(fmt[len(kind):])
    t = synth.make_tree(depth_limit=depth, basis_dim=basis, seed=seed)
    if kind == "RGBA":
        t = rgba_tree(t)
    elif kind in ("SG", "ASG"):
        t = synth.with_lobes(t, kind, seed=3)
    return t


def _dev(t, **kw):
    return R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format, extra_data=t.extra, **kw)


def _host(t):
    return orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)


def _map(poses, t0, t):
    """poses of t0's world in t's, each aimed at the image of the point it looked at"""
    return [reframe_pose(p, t0, t, target=aim_point(p)) for p in poses]


def _cams(W, H, fx, poses, fy=None):
    out = []
    for p in poses:
        c = R.Camera(W, H, fx, fx if fy is None else fy)
        c.set_c2w(p)
        out.append(c)
    return out


def _oracle(ht, cam, spp, jump, **optkw):
    ocam = orc.camera(cam.width, cam.height, cam.fx, cam.fy, np.asarray(cam.transform, f32).reshape(-1))
    aux, rgba, _ = orc.render_frame(ht, ocam, orc.default_options(spp=spp, **optkw), orc.rng(frame=jump), threads=oracle_threads(),
                                    want_stats=False)
    return aux, rgba


def _distinct(t):
    assert len(set(float(s) for s in t.scale)) == 3 and np.sum(t.offset != f32(0.5)) >= 2  # (what this file is about)


# ------------------------------------------------------------------ CPU: the frames, the loader


def test_reframing_keeps_the_tree_space_content():
    t0 = synth.make_tree(depth_limit=4, basis_dim=9, seed=2)
    lobed = synth.with_lobes(t0, "SG", seed=1)
    for name, (scale, offset) in FRAMES.items():
        t = reframe(lobed, scale, offset)
        assert t.child is lobed.child and t.data is lobed.data and t.extra is lobed.extra and t.data_format == "SG9"
        assert np.array_equal(t.scale, np.asarray(scale, f32)) and np.array_equal(t.offset, np.asarray(offset, f32))
        # a point of the old world and its image are the same tree-space point; the scene centre is looked at
        p = np.array([0.3, -1.0, 0.7])
        q = reframe_point(p, t0, t)
        assert np.allclose(t0.offset + t0.scale * p, t.offset.astype(np.float64) + t.scale.astype(np.float64) * q, atol=1e-12)
        pose = reframe_pose(synth.orbit_poses(3)[1], t0, t)
        centre = reframe_point((0, 0, 0), t0, t)
        to_centre = centre - pose[:3, 3]
        assert np.allclose(np.cross(-pose[:3, 2], to_centre / np.linalg.norm(to_centre)), 0, atol=1e-9), name
        assert np.allclose(pose[:3, :3].T @ pose[:3, :3], np.eye(3), atol=1e-12)
    for name in ANISO_FRAMES:
        _distinct(reframe(t0, *FRAMES[name]))
    assert np.argmax(FRAMES["aniso"][0]) != np.argmax(FRAMES["aniso_perm"][0])  # another axis is the short one


def _probe(path):
    buf = C.create_string_buffer(4096)
    rc = R.lib().rto_tree_probe_npz(os.fsencode(str(path)), buf, 4096)
    assert rc == 0, R.lib().rto_last_error()
    return json.loads(buf.value.decode())


def test_loader_reads_invradius3_in_order_and_the_scalar_invradius(tmp_path):
    t = reframe(synth.make_tree(depth_limit=3, basis_dim=4, seed=2), *FRAMES["aniso"])
    info = _probe(t.save_npz(str(tmp_path / "three.npz")))
    assert [f32(v) for v in info["scale"]] == [f32(0.5), f32(0.25), f32(0.3)]
    assert [f32(v) for v in info["offset"]] == [f32(0.55), f32(0.4), f32(0.5)]
    ht = _host(t)
    assert list(ht.c.scale) == [f32(v) for v in info["scale"]] and list(ht.c.offset) == [f32(v) for v in info["offset"]]
    # float64 arrays and a row vector are read value by value
    kw = dict(data_dim=np.int64(t.data_dim), data_format=np.array(t.data_format), offset=t.offset.astype(np.float64)[None, :],
              child=t.child, data=t.data)
    np.savez(str(tmp_path / "f64.npz"), invradius3=np.array([0.5, 0.25, 0.3]), **kw)
    info64 = _probe(tmp_path / "f64.npz")
    assert [f32(v) for v in info64["scale"]] == [f32(0.5), f32(0.25), f32(0.3)] and info64["offset"] == info["offset"]
    # the legacy key: one value for the three axes
    np.savez(str(tmp_path / "scalar.npz"), invradius=f32(0.37), **kw)
    one = _probe(tmp_path / "scalar.npz")
    assert [f32(v) for v in one["scale"]] == [f32(0.37)] * 3 and one["offset"] == info["offset"]
    # invradius3 wins where a file carries both
    np.savez(str(tmp_path / "both.npz"), invradius=f32(0.37), invradius3=t.scale, **kw)
    assert _probe(tmp_path / "both.npz")["scale"] == info["scale"]


# ------------------------------------------------------------------ GPU: all kernels, all bases


# cameras of the isotropic world: outside, far, inside the box, looking past the model
VIEW_POSES = [synth.orbit_poses(5)[1], synth.look_at_c2w((9.0, 0.5, 1.0)), synth.look_at_c2w((0.2, 0.1, 0.3)),
              synth.look_at_c2w((3.0, 0.5, 1.0), target=(0.5, 2.5, 0.3))]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 6, 32])
@pytest.mark.parametrize("fmt", ["RGBA", "SH9", "SH16", "SG16", "ASG9"])
@pytest.mark.parametrize("frame", ANISO_FRAMES)
def test_every_kernel_equals_the_oracle(frame, fmt, spp):
    t0 = _tree(fmt)
    t = reframe(t0, *FRAMES[frame])
    _distinct(t)
    dt = _dev(t)
    W, H = 72, 56
    fx = synth.blender_focal(W)
    cams = _cams(W, H, fx, _map(VIEW_POSES, t0, t))
    jumps = [40 + i for i in range(len(cams))]
    lobed = t.extra is not None
    want = []
    for cam, j in zip(cams, jumps):
        if not lobed:
            want.append(_oracle(_host(t), cam, spp, j, background_brightness=0.25))
        elif spp == 1:  # the oracle's hit leaf + the restated SG / ASG shading
            from test_sg_asg import _expected_frame
            aux, image, _ = _expected_frame(t, W, H, fx, cam.transform.reshape(-1), rng_frame=j, bg=0.25)
            want.append((aux, image))
        else:  # opacity does not depend on the colours: the oracle's, of an RGBA tree over the same child[] and sigma
            from test_sg_asg import _slot_tree
            want.append(_oracle(_slot_tree(t), cam, spp, j, background_brightness=0.25))
    assert sum(int((w[0][3] > 0).sum()) for w in want) > 1000  # (the views hold the object)
    opt = R.RenderOptions(spp=spp, denoise=False, background_brightness=0.25)
    got = {}
    ctx = R.RenderContext(W, H, frames=len(cams))
    ctx.rng_seed()
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=jumps)
    for i in range(len(cams)):
        ctx.select_frame(i)
        got["batched", i] = (ctx.download_aux(), ctx.download_image())
    one = R.RenderContext(W, H)
    for kernel, name in ((R.KERNEL_FAST, "fast"), (R.KERNEL_GENERIC, "generic")):
        one.set_kernel(kernel)
        for i, cam in enumerate(cams):
            one.rng_seed()
            one.rng_advance(jumps[i] << 32)
            R.launch_renderer(dt, cam, opt, one)
            got[name, i] = (one.download_aux(), one.download_image())
    for (name, i), (aux, image) in got.items():
        what = "%s %s spp %d %s pose %d" % (frame, fmt, spp, name, i)
        if not lobed or spp == 1:
            assert_bits_equal(aux, want[i][0], what + " aux")
            assert_bits_equal(image, want[i][1], what + " image")
        else:
            assert_bits_equal(aux[3], want[i][0][3], what + " alpha")
            assert_bits_equal(aux[7], want[i][0][7], what + " alpha^2")
            assert_bits_equal(aux, got["generic", i][0], what + " aux vs generic")
            assert_bits_equal(image, got["generic", i][1], what + " image vs generic")
    dt.free()


# ------------------------------------------------------------------ GPU: culling


def _short_axis_poses(t):
    """Two cameras that look across the SHORT world axis of t (the largest scale), the model reaching the frame's edge along
    it: one centred, so close that the model's extent along the axis overflows the image, and one aimed at the model's end.
    A bounding sphere too small along the short axis would cull tiles at the model's rim there."""
    sc, off = t.scale.astype(np.float64), t.offset.astype(np.float64)
    a = int(np.argmax(sc))
    b = (a + 1) % 3
    centre = (0.5 - off) / sc
    half = 0.37 / sc  # (the model spans about [0.13, 0.87] of the tree: |world| < 1.1 of make_tree's radius 1.5)
    eye = centre.copy()
    eye[b] -= 1.2 * half[a] + half[b]  # the model's depth + a distance from which 2 * half[a] is wider than the image
    up = np.eye(3)[(a + 2) % 3]
    end = centre.copy()
    end[a] += half[a]
    return [synth.look_at_c2w(eye, centre, up=up), synth.look_at_c2w(eye, end, up=up)]


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(FRAMES))
def test_culled_frames_equal_marched_ones_and_the_oracle(frame):
    from test_culling import _poses, _render
    t0 = synth.make_tree(depth_limit=7, basis_dim=9, seed=21, shell=2.0)
    t = reframe(t0, *FRAMES[frame])
    ht, dt = _host(t), _dev(t)
    plain = _dev(t, no_culling=True)
    W, H = 200, 136
    poses = _map(_poses(), t0, t) + _short_axis_poses(t)
    cams = []
    for i, p in enumerate(poses):
        c = R.Camera(W, H, 260.0, 300.0 if i % 2 else 260.0)  # non-square pixels on every second pose
        c.set_c2w(p)
        cams.append(c)
    cams[3].transform[:3] *= f32(1.7)  # the scaled (non-orthonormal) camera matrix
    n = len(cams)
    ctx = R.RenderContext(W, H, frames=n)
    jumps = list(range(100, 100 + n))
    on, (live_on, all_on) = _render(dt, cams, 6, True, ctx, jumps)
    off, (live_off, all_off) = _render(plain, cams, 6, True, ctx, jumps)
    assert all_on == all_off == n * 25 * 17 and live_off == all_off
    assert 0 < live_on < all_on  # (the test really culls)
    for f in range(n):
        assert_bits_equal(on[f][0], off[f][0], "%s aux frame %d, culled vs no_culling" % (frame, f))
        assert_bits_equal(on[f][1], off[f][1], "%s image frame %d, culled vs no_culling" % (frame, f))
    for f in (0, 3, 12, 13, 16, n - 2, n - 1):  # orbit, the scaled matrix, inside, grazing, the edge of the frame, the short axis
        aux_o, rgba_o = _oracle(ht, cams[f], 6, jumps[f])
        assert_bits_equal(on[f][0], aux_o, "%s aux frame %d vs oracle" % (frame, f))
        assert_bits_equal(on[f][1], rgba_o, "%s image frame %d vs oracle" % (frame, f))
    # the short-axis views hold the model up to the frame's edge and cull some tiles, not all
    solo = R.RenderContext(W, H, frames=1)
    for f in (n - 2, n - 1):
        _, (live, total) = _render(dt, [cams[f]], 6, True, solo, [5])
        assert 0 < live and (live < total or f == n - 2), (frame, f, live, total)  # (the centred close-up may fill every tile)
        alpha = on[f][0][3]
        assert (alpha[:, :4] > 0).any() or (alpha[:, -4:] > 0).any() or (alpha[:4] > 0).any() or (alpha[-4:] > 0).any()
    # the single-frame kernel's own culling (tuning key cull_single)
    for f in (0, 13, n - 1):
        for key in (1, 0):
            solo.set_tuning("cull_single", key)
            solo.set_kernel(R.KERNEL_FAST)
            solo.rng_seed()
            solo.rng_advance(jumps[f] << 32)
            R.launch_renderer(dt, cams[f], R.RenderOptions(spp=6, denoise=False), solo)
            assert_bits_equal(solo.download_aux(), on[f][0], "%s frame %d single-frame kernel, cull_single %d" % (frame, f, key))
    dt.free()
    plain.free()


# ------------------------------------------------------------------ GPU: denoise routes


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [0, 1, 2])
def test_denoise_with_tile_marks_equals_denoise_without(lean):
    """net.denoise after a culled batch (tile marks: culled tiles are neither read nor filtered) == after the same batch with
    the culling off (every tile marked), both filter modes, full / lean / sparse outputs"""
    import torch
    from rt_octree_amd import denoiser
    t0 = synth.make_tree(depth_limit=6, basis_dim=9, seed=7, shell=2.0)
    t = reframe(t0, *FRAMES["aniso"])
    dt = _dev(t)
    torch.manual_seed(3)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval())
    W, H, n = 168, 120, 4
    poses = _map([synth.orbit_poses(5)[1], synth.orbit_poses(5)[3], synth.look_at_c2w((9.0, 0.5, 1.0)),
                  synth.look_at_c2w((2.5, 2.5, 0.2), target=(0.0, 3.0, 0.0))], t0, t)
    cams = _cams(W, H, synth.blender_focal(W), poses)
    opt = R.RenderOptions(spp=6, denoise=True, background_brightness=0.7)
    for mode in (R.FILTER_FAST, R.FILTER_EXACT):
        if lean == 2 and mode == R.FILTER_EXACT:  # sparse frames take the factorised route only: refused, not mis-filtered
            ctx = R.RenderContext(W, H, frames=n)
            ctx.set_lean_outputs(lean)
            ctx.rng_seed()
            R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[7, 8, 9, 10])
            ctx.select_frame(0)
            with pytest.raises(R.RtoError):
                net.denoise(ctx, n, mode)
            ctx.free()
            continue
        images = []
        for cull in (1, 0):
            ctx = R.RenderContext(W, H, frames=n)
            ctx.set_lean_outputs(lean)
            ctx.set_tuning("cull", cull)
            ctx.rng_seed()
            R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[7, 8, 9, 10])
            live, total = ctx.queue_stats()
            assert (0 < live < total) if cull else live == total
            ctx.select_frame(0)
            net.denoise(ctx, n, mode)
            torch.cuda.synchronize()
            images.append(torch.as_tensor(ctx.batch_views()[2], device="cuda:0")[:n].cpu().numpy().copy())
            ctx.free()
        assert_bits_equal(images[0], images[1], "lean %d mode %d: marked vs unmarked denoise" % (lean, mode))
        assert np.isfinite(images[0]).all() and images[0][..., :3].std() > 0.01
    dt.free()


# ------------------------------------------------------------------ GPU: rays


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [R.KERNEL_FAST, R.KERNEL_GENERIC])
@pytest.mark.parametrize("frame", ANISO_FRAMES)
def test_rays_with_depth_limits_and_backdrops_equal_the_oracle(frame, kernel):
    from test_rays import _camera_equivalence, _mixed_rays, ray_oracle
    t0 = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    t = reframe(t0, *FRAMES[frame])
    ht, dt = _host(t), _dev(t)
    n = 60_000
    o, d = _mixed_rays(t, n, seed=5)
    rng = np.random.default_rng(6)
    diagonal = float(np.sqrt(np.sum((1.0 / t.scale.astype(np.float64)) ** 2)))  # of the tree's box in world units, per axis
    tm = rng.uniform(0.0, 2.0 * diagonal, n).astype(f32)
    tm[::9] = np.inf
    back = rng.uniform(0, 1.5, (n, 3)).astype(f32)
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed()
    ctx.set_kernel(kernel)
    opt = R.RenderOptions(spp=6)
    got = R.render_rays(dt, o, d, opt, ctx, t_max=tm, background=back, first_ray=777).cpu().numpy()
    assert_bits_equal(got, ray_oracle(ht, o, d, 6, t_max=tm, background=back, first_ray=777), "%s rays, kernel %d" % (frame, kernel))
    full = R.render_rays(dt, o, d, opt, ctx, background=back, first_ray=777).cpu().numpy()
    assert (got[:, 3] != full[:, 3]).sum() > 100 and ((got[:, 3] == full[:, 3]) & (full[:, 3] > 0)).sum() > 100  # (cuts in front of and behind what a ray hits)
    assert (full[:, 3] > 0).sum() > n // 20
    # a camera's rays == the camera's frame
    cam = _cams(72, 40, synth.blender_focal(72), _map([synth.orbit_poses(4)[1]], t0, t))[0]
    for spp in (1, 32):
        hit = _camera_equivalence(dt, cam, spp, kernel)
        assert (hit[:, 3] > 0).sum() > 200
    dt.free()


# ------------------------------------------------------------------ GPU: quantised trees


@pytest.mark.gpu
@pytest.mark.parametrize("basis,n_retain", [(9, 1), (16, 2)])
def test_quantised_tree_direct_and_expanded(tmp_path, basis, n_retain):
    t0 = synth.make_tree(depth_limit=6, basis_dim=basis, seed=11)
    t = reframe(t0, *FRAMES["aniso"])
    path = str(tmp_path / "tree.npz")
    decoded = t.save_quant_npz(path, n_retain=n_retain)
    direct, dense = R.N3Tree(path, quant_direct=True), R.N3Tree(path)
    assert np.array_equal(direct.scale, t.scale) and np.array_equal(dense.offset, t.offset)
    ht = orc.HostTree(t.child, decoded, t.scale, t.offset, t.data_format)
    W, H = 96, 64
    cams = _cams(W, H, synth.blender_focal(W), _map(VIEW_POSES[:3], t0, t))
    opt = R.RenderOptions(spp=6, denoise=False)
    a, b = R.RenderContext(W, H, frames=3), R.RenderContext(W, H, frames=3)
    R.launch_renderer_batch(direct, cams, opt, a, rng_jumps=[100, 101, 102])
    R.launch_renderer_batch(dense, cams, opt, b, rng_jumps=[100, 101, 102])
    for f in range(3):
        aux_o, rgba_o = _oracle(ht, cams[f], 6, 100 + f)
        for ctx, name in ((a, "direct"), (b, "expanded")):
            ctx.select_frame(f)
            assert_bits_equal(ctx.download_aux(), aux_o, "%s aux f%d vs oracle" % (name, f))
            assert_bits_equal(ctx.download_image(), rgba_o, "%s image f%d vs oracle" % (name, f))
    direct.free()
    dense.free()


# ------------------------------------------------------------------ GPU: fuzz


def _random_frame(rs):
    """per-axis scale log-uniform in [0.05, 4], offset uniform in [0.2, 0.8]"""
    return np.exp(rs.uniform(np.log(0.05), np.log(4.0), 3)), rs.uniform(0.2, 0.8, 3)


def _seeds():
    """32 scenes by default; RTO_FUZZ_SEEDS="first:last" widens the sweep for a soak run (tools/fuzz_soak.sh)"""
    spec = os.environ.get("RTO_FUZZ_SEEDS", "")
    if ":" in spec:
        a, b = spec.split(":")
        return range(int(a), int(b))
    return range(32)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds())
def test_random_reframed_scene_all_kernels_bit_exact(seed):
    from test_fuzz_parity import _scene
    t0, W, H, fx, poses, optkw, frame0 = _scene(seed)
    t = reframe(t0, *_random_frame(np.random.RandomState(7000 + seed)))
    ht, dt = _host(t), _dev(t)
    spp = optkw.pop("spp")
    cams = _cams(W, H, fx, _map(poses, t0, t))
    want = [_oracle(ht, cam, spp, frame0 + i, **optkw) for i, cam in enumerate(cams)]
    opt = R.RenderOptions(spp=spp, denoise=False, **optkw)
    ctx = R.RenderContext(W, H, frames=len(cams))
    R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=[frame0 + i for i in range(len(cams))])
    for i in range(len(cams)):
        ctx.select_frame(i)
        assert_bits_equal(ctx.download_aux(), want[i][0], "seed %d batched aux %d" % (seed, i))
        assert_bits_equal(ctx.download_image(), want[i][1], "seed %d batched image %d" % (seed, i))
    one = R.RenderContext(W, H)
    for kernel in (R.KERNEL_FAST, R.KERNEL_GENERIC):
        one.set_kernel(kernel)
        one.rng_seed()
        one.rng_advance(frame0 << 32)
        R.launch_renderer(dt, cams[0], opt, one)
        assert_bits_equal(one.download_aux(), want[0][0], "seed %d kernel %d aux" % (seed, kernel))
        assert_bits_equal(one.download_image(), want[0][1], "seed %d kernel %d image" % (seed, kernel))
    dt.free()
