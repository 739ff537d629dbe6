"""Shared helpers for the parity tests: build the same scene for the oracle and for librto."""
import numpy as np

import orc
import rt_octree_amd as R
from rt_octree_amd import synth


def rgba_tree(tree_sh, seed=3):
    """An RGBA-format (data_dim 4, basis_dim -1) tree on the topology of `tree_sh`
    (rt_core.cuh:318-322 branch)."""
    rng = np.random.default_rng(seed)
    sig = tree_sh.data[..., -1:].astype(np.float32)
    rgb = rng.uniform(0, 1, tree_sh.data.shape[:-1] + (3,)).astype(np.float32) * (sig > 0)
    data = np.concatenate([rgb, sig], -1).astype(np.float16)
    return synth.SynthTree(tree_sh.child, data, tree_sh.scale, tree_sh.offset, "RGBA", tree_sh.depth_limit, {})


# World frames (invradius3, offset) other than synth.make_tree's cube centred on the origin.  The tree-space content does not
# move under a re-framing, so the object stays inside [0, 1)^3; the world it is seen from is stretched and shifted.
FRAME_ANISO = ((0.5, 0.25, 0.3), (0.55, 0.4, 0.5))        # strongly anisotropic, off centre; x is the short world axis
FRAME_ANISO_PERM = ((0.3, 0.5, 0.25), (0.5, 0.55, 0.4))   # the same values on other axes: y is the short one
FRAME_OFF_CENTRE = ((1.0 / 3.0,) * 3, (0.3, 0.65, 0.5))   # isotropic, off centre
FRAME_LARGE = ((0.01, 0.012, 0.008), (0.45, 0.5, 0.6))    # a world some hundred units across
FRAME_SMALL = ((8.0, 6.0, 10.0), (0.5, 0.55, 0.4))        # a world an eighth of a unit across
FRAMES = {"aniso": FRAME_ANISO, "aniso_perm": FRAME_ANISO_PERM, "off_centre": FRAME_OFF_CENTRE, "large": FRAME_LARGE,
          "small": FRAME_SMALL}
ANISO_FRAMES = ("aniso", "aniso_perm")


def reframe(tree, scale3, offset3):
    """The same SynthTree (topology, data, lobes) in another world frame: tree = offset3 + scale3 * world."""
    scale3 = np.broadcast_to(np.asarray(scale3, np.float32), (3,)).copy()
    offset3 = np.broadcast_to(np.asarray(offset3, np.float32), (3,)).copy()
    return synth.SynthTree(tree.child, tree.data, scale3, offset3, tree.data_format, tree.depth_limit, tree.stats, tree.extra)


def reframe_point(p, tree_from, tree_to):
    """world' = (offset_from + scale_from * world - offset_to) / scale_to: the same tree-space point in the other world"""
    p = np.asarray(p, np.float64)
    q = tree_from.offset.astype(np.float64) + tree_from.scale.astype(np.float64) * p
    return (q - tree_to.offset.astype(np.float64)) / tree_to.scale.astype(np.float64)


def reframe_pose(c2w, tree_from, tree_to, target=None):
    """A camera placed for tree_from's world, in tree_to's: the position is mapped with reframe_point, the orientation rebuilt
    with synth.look_at_c2w towards the mapped `target` (a point of tree_from's world; default: the scene centre, tree-space
    (0.5, 0.5, 0.5)).  An affine map does not keep a rotation a rotation, hence the rebuilding."""
    c2w = np.asarray(c2w, np.float64)
    if target is None:
        target = (0.5 - tree_from.offset.astype(np.float64)) / tree_from.scale.astype(np.float64)
    return synth.look_at_c2w(reframe_point(c2w[:3, 3], tree_from, tree_to), reframe_point(target, tree_from, tree_to))


def aim_point(c2w, distance=None):
    """the point `distance` (default: the camera's distance from the origin, at least 1) along the view axis of a look_at_c2w pose"""
    c2w = np.asarray(c2w, np.float64)
    pos = c2w[:3, 3]
    return pos - c2w[:3, 2] * (max(np.linalg.norm(pos), 1.0) if distance is None else distance)


def make_pair(tree, device=0):
    """-> (orc.HostTree, R.N3Tree) over the same arrays"""
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    dt = R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, device=device)
    return ht, dt


def rcam(W, H, pose, fx=None):
    """the package's Camera for a pose (fx: synth.blender_focal(W) unless given)"""
    fx = synth.blender_focal(W) if fx is None else fx
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(pose)
    return cam


def cameras(W, H, pose, fx=None):
    cam = rcam(W, H, pose, fx)
    ocam = orc.camera(W, H, cam.fx, cam.fx, cam.transform.reshape(-1))
    return ocam, cam


def rcam_of(model_cam):
    """the package's Camera for a camera of the numpy models (layer_ref.Cam): the same 12 floats"""
    cam = R.Camera(model_cam.width, model_cam.height, model_cam.fx, model_cam.fy)
    cam.transform = [float(v) for v in model_cam.transform]
    return cam


def gpu_torch():
    import torch
    return torch


def check_33_cameras_in_one_call(draw, cams, model):
    """33 cameras, one more than a launch takes: draw(cams, **kw) -> (depth, color) against 33 calls and model(f) -> (depth, color)"""
    torch = gpu_torch()
    d33, c33 = draw(cams)
    for f in range(33):
        d1, c1 = draw([cams[f]])
        assert torch.equal(d1[0].view(torch.int32), d33[f].view(torch.int32)) and torch.equal(c1[0].view(torch.int32), c33[f].view(torch.int32)), f
    for f in (0, 31, 32):
        wd, wc = model(f)
        assert_bits_equal(d33[f].cpu().numpy(), wd, "frame %d depth" % f)
        assert_bits_equal(c33[f].cpu().numpy(), wc, "frame %d colour" % f)
    d_only, none = draw(cams, color=False)
    assert none is None and torch.equal(d_only.view(torch.int32), d33.view(torch.int32))
    none, c_only = draw(cams, depth=False)
    assert none is None and torch.equal(c_only.view(torch.int32), c33.view(torch.int32))


def oracle_frame(ht, ocam, spp, frame=0, **optkw):
    opt = orc.default_options(spp=spp, **optkw)
    return orc.render_frame(ht, ocam, opt, orc.rng(frame=frame))


def hip_frame(dt, cam, spp, frame=0, kernel=R.KERNEL_AUTO, ctx=None, denoise=False, **optkw):
    ctx = ctx or R.RenderContext(cam.width, cam.height)
    ctx.rng_seed()
    for _ in range(frame):
        ctx.rng_advance()
    ctx.set_kernel(kernel)
    opt = R.RenderOptions(spp=spp, denoise=denoise, **optkw)
    R.launch_renderer(dt, cam, opt, ctx)
    return ctx.download_aux(), ctx.download_image(noisy=denoise), ctx


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    av, bv = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(av.reshape(-1) != bv.reshape(-1))
    assert bad.size == 0, "%s: %d of %d words differ; first at %d: %r vs %r" % (
        what, bad.size, av.size, bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


def oracle_threads():
    """threads for whole-frame oracle renders: the cores this process may really use (affinity mask capped by the cgroup's CPU
    quota -- the GPU boxes show 256 CPUs behind a quota of 16, and 256 throttled OpenMP threads crawl)"""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                n = min(n, max(1, int(float(q) / float(per))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def oracle_whole_frame(ht, cam, fx, spp, jump, fy=None):
    """orc.render_frame for one librto camera at RNG jump `jump` -> (aux [8,H,W], rgba [H,W,4])"""
    ocam = orc.camera(cam.width, cam.height, fx, fx if fy is None else fy, cam.transform.reshape(-1))
    aux, rgba, _ = orc.render_frame(ht, ocam, orc.default_options(spp=spp), orc.rng(frame=jump), threads=oracle_threads(), want_stats=False)
    return aux, rgba
