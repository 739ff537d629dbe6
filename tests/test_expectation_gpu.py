"""GPU twin of tests/test_expectation.py: the mean of 4096 spp rendered by the HIP kernels (batched
persistent kernel and the single-frame kernel, independently seeded launches) against the independent float64
rendering-equation model of tests/expected_render.py -- evidence that does not pass through oracle/."""
import numpy as np
import pytest

import expected_render as E
import rt_octree_amd as R
from rt_octree_amd import synth
from test_expectation import _check_against_model, _thin

pytestmark = pytest.mark.gpu


def test_hip_mean_matches_rendering_equation():
    t = _thin(synth.make_tree(depth_limit=6, basis_dim=9, seed=3, shell=1.5), 0.08)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    W = H = 64
    fx = 0.9 * synth.blender_focal(W)
    pose = synth.orbit_poses(7)[3]
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(pose)
    rot = [0.1, 0.3, -0.2]
    opt = R.RenderOptions(spp=32, denoise=False, background_brightness=0.5, rot_dirs=rot)
    # independently seeded launches (see _mean_of_frames: the reference's 2^32-strided frame streams are
    # correlated in the tails); two frames per launch of the batched kernel
    ctx = R.RenderContext(W, H, frames=2)
    acc = np.zeros((4, H, W))
    n_frames = 0
    for launch in range(64):
        ctx.rng_seed(977 + 7919 * launch)
        R.launch_renderer_batch(dt, [cam] * 2, opt, ctx, rng_jumps=[0, 1 + launch])
        for k in range(2):
            ctx.select_frame(k)
            acc += ctx.download_aux()[:4]
            n_frames += 1
    scene = E.Scene(t.child, t.data, t.scale, t.offset, t.data_format)
    mean, var = E.expected_frame(scene, pose, W, H, fx, fx, bg=0.5, rot_dirs=rot)
    _check_against_model(acc / n_frames, mean, var, n_frames * 32, "hip batched")
    # the single-frame kernel on other RNG streams
    one = R.RenderContext(W, H)
    acc[:] = 0
    for k in range(64):
        one.rng_seed(31337 + 104729 * k)
        R.launch_renderer(dt, cam, opt, one)
        acc += one.download_aux()[:4]
    _check_against_model(acc / 64, mean, var, 64 * 32, "hip single-frame")


# ------------------------------------------------------------------ the bases, frames and ray batches added since
def _lobed(kind):
    from test_expectation import _lobed_thin
    return _lobed_thin(kind)


def _reframed(name, density=0.08):
    from helpers import FRAMES, reframe
    return reframe(_thin(synth.make_tree(depth_limit=6, basis_dim=9, seed=3, shell=1.5), density), *FRAMES[name])


def _orbit_pose(t):
    """synth.orbit_poses(7)[3], mapped into t's world where that is not make_tree's"""
    from helpers import reframe_pose
    return reframe_pose(synth.orbit_poses(7)[3], synth.make_tree(depth_limit=1, basis_dim=1), t)


THIN = 0.03  # at 0.08 these views hold ~90 pixels of alpha > 0.9995, whose rare misses are Poisson, not Gaussian: one of them
# (expected alpha 0.999973, 2 misses in 4096 samples) failed the 5 sigma bound in the oracle's frames of the same seeds too


def _rgba():
    from helpers import rgba_tree
    return _thin(rgba_tree(synth.make_tree(depth_limit=6, basis_dim=9, seed=3, shell=1.5)), THIN)


# name -> (tree, background, NDC?, culling must skip tiles?).  Every SH / RGBA input passed the same check with the CPU oracle's
# frames first, under the very seeds used below (the kernels equal the oracle bit for bit) and under others: a miss here is the
# kernels', not a tail pixel of the input.  (The oracle does not shade SG / ASG; their tree and view passed on the CPU at 24 x 20.)
CASES = {
    "SH16": (lambda: _thin(synth.make_tree(depth_limit=6, basis_dim=16, seed=3, shell=1.5), THIN), 0.5, False, False),
    "SH25": (lambda: _thin(synth.make_tree(depth_limit=6, basis_dim=25, seed=3, shell=1.5), THIN), 0.5, False, False),
    "RGBA": (_rgba, 0.5, False, False),
    "SG9": (lambda: _lobed("SG"), 1.0, False, False),
    "ASG9": (lambda: _lobed("ASG"), 1.0, False, False),
    "aniso": (lambda: _reframed("aniso", THIN), 0.5, False, True),
    "aniso_perm": (lambda: _reframed("aniso_perm", THIN), 0.5, False, True),
    "ndc": (lambda: _thin(synth.make_tree(depth_limit=6, basis_dim=9, seed=3, shell=1.5), THIN), 0.5, True, False),
}
W = H = 64
FX = 0.9 * synth.blender_focal(W)


def case_inputs(name):
    """-> tree, pose, background, ndc"""
    from test_expectation import NDC_POSE
    make, bg, ndc, _ = CASES[name]
    t = make()
    return t, (NDC_POSE if ndc else _orbit_pose(t)), bg, ((float(W), float(H), FX) if ndc else None)


@pytest.mark.parametrize("name", list(CASES))
def test_hip_mean_matches_the_model(name):
    t, pose, bg, ndc = case_inputs(name)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format, extra_data=t.extra)
    if ndc:
        dt.set_ndc(*ndc)
    cam = R.Camera(W, H, FX, FX)
    cam.set_c2w(pose)
    opt = R.RenderOptions(spp=32, denoise=False, background_brightness=bg)
    mean, var = E.expected_frame(E.Scene.of(t), pose, W, H, FX, FX, bg=bg, ndc=ndc)  # (one model for both kernels)
    assert (mean[3] > 0.05).sum() > 400
    ctx = R.RenderContext(W, H, frames=2)
    acc = np.zeros((4, H, W))
    for launch in range(64):
        ctx.rng_seed(977 + 7919 * launch)
        R.launch_renderer_batch(dt, [cam] * 2, opt, ctx, rng_jumps=[0, 1 + launch])
        if CASES[name][3]:  # a wrong cull turns expected density into background: the culling must be at work here
            live, total = ctx.queue_stats()
            assert 0 < live < total, (live, total)
        for k in range(2):
            ctx.select_frame(k)
            acc += ctx.download_aux()[:4]
    _check_against_model(acc / 128, mean, var, 128 * 32, "%s, hip batched" % name)
    one = R.RenderContext(W, H)
    acc[:] = 0
    for k in range(128):
        one.rng_seed(31337 + 104729 * k)
        R.launch_renderer(dt, cam, opt, one)
        acc += one.download_aux()[:4]
    _check_against_model(acc / 128, mean, var, 128 * 32, "%s, hip single-frame" % name)
    dt.free()


def ray_inputs(which):
    """-> tree, origins, dirs, t_max, backdrop of the two ray batches: "camera": the pixels of a camera on an anisotropic tree,
    each ray cut in the middle of its widest empty gap; "free": origins inside and outside the box, aimed at the model's
    neighbourhood, directions scaled by 0.01 ... 100, a third of them cut the same way"""
    t = _reframed("aniso", THIN)
    scene = E.Scene.of(t)
    rng = np.random.default_rng(17)
    if which == "camera":
        cam = R.Camera(48, 40, 0.9 * synth.blender_focal(48))
        cam.set_c2w(_orbit_pose(t))
        o, d = R.camera_rays(cam)
        cut = np.ones(o.shape[0], bool)
    else:
        n = 1800
        ot = rng.uniform(-0.3, 1.3, (n, 3))
        ot[: n // 3] = rng.uniform(0.1, 0.9, (n // 3, 3))  # inside the box
        aim = rng.uniform(0.3, 0.7, (n, 3))
        to_world = lambda p: (p - t.offset.astype(np.float64)) / t.scale.astype(np.float64)
        o = to_world(ot).astype(np.float32)
        d = to_world(aim) - to_world(ot)
        d = (d / np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
        cut = np.arange(n) % 3 == 0
    tm = np.full(o.shape[0], np.inf, np.float32)
    for i in np.flatnonzero(cut):
        tm[i] = E.t_max_in_widest_gap(scene, o[i], d[i], min_gap=0.02) or np.inf
    back = rng.uniform(0, 1, o.shape).astype(np.float32)
    return t, o, d, tm, back


@pytest.mark.parametrize("which", ["camera", "free"])
def test_hip_rays_match_the_model(which):
    t, o, d, tm, back = ray_inputs(which)
    assert np.isfinite(tm).sum() > 150
    mean, var = E.expected_rays(E.Scene.of(t), o, d, t_max=tm, background=back)
    full, _ = E.expected_rays(E.Scene.of(t), o, d, background=back)
    assert (np.abs(full[:, 3] - mean[:, 3]) > 0.02).sum() > 100  # (the cuts remove something)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    ctx = R.RenderContext(8, 8)
    opt = R.RenderOptions(spp=32)
    for kernel, name in ((R.KERNEL_FAST, "fast"), (R.KERNEL_GENERIC, "generic")):
        ctx.set_kernel(kernel)
        acc = np.zeros((o.shape[0], 4))
        for k in range(128):
            ctx.rng_seed(4242 + 15485863 * k + kernel)  # independently seeded launches
            acc += R.render_rays(dt, o, d, opt, ctx, t_max=tm, background=back).cpu().numpy()
        _check_against_model(acc / 128, mean, var, 128 * 32, "rays (%s), %s kernel" % (which, name))
    dt.free()
