"""What the three launch entries refuse, and what a refused launch leaves behind.

rto_launch_renderer, rto_launch_renderer_batch and rto_launch_rays share their argument checks (rto_render_abi.cpp:
check_tree_options, check_camera).  The table pins the code of every applicable entry x fault pair; the last test pins that a
batched launch refused for its arguments leaves the context as it was (the tile marks of the launch before it stay readable)."""
import ctypes as C

import numpy as np
import pytest

import rt_octree_amd as R
from rt_octree_amd import synth
from rt_octree_amd._lib import CCamera, CRays

pytestmark = pytest.mark.gpu

E_INVALID, E_SPP, E_UNSUPPORTED, E_FORMAT = -1, -2, -3, -6
W = H = 16
ENTRIES = ("frame", "batch", "rays")


@pytest.fixture(scope="module")
def world():
    import torch
    t = synth.make_tree(depth_limit=3, basis_dim=9, seed=7)
    sg = synth.with_lobes(synth.make_tree(depth_limit=3, basis_dim=4, seed=5), "SG", seed=9)
    w = {
        "plain": R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format),
        "compact": R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format, compact_records=True),
        "bare_sg": R.N3Tree.from_arrays(sg.child, sg.data, sg.scale, sg.offset, sg.data_format),  # (no extra_data: no lobes)
        "ctx": R.RenderContext(W, H, frames=2),
    }
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(synth.orbit_poses(4)[1])
    w["cam"] = cam
    dev = torch.device("cuda", 0)
    o, d = R.camera_rays(cam)
    w["origins"], w["dirs"] = torch.from_numpy(o[:8].copy()).to(dev), torch.from_numpy(d[:8].copy()).to(dev)
    w["out"] = torch.empty((8, 4), dtype=torch.float32, device=dev)
    yield w
    for k in ("plain", "compact", "bare_sg", "ctx"):
        w[k].free()


def _ccam(cam, width=None, height=None, fx=None):
    c = cam.to_c()
    if width is not None:
        c.width, c.height = width, height
    if fx is not None:
        c.fx = fx
    return c


def _launch(entry, w, tree_h, cc, opt):
    """the raw return code of one entry point (tree_h may be None: a null tree)"""
    L, co, ctx = R.lib(), opt.to_c(), w["ctx"]._h
    if entry == "frame":
        return L.rto_launch_renderer(tree_h, C.byref(cc), C.byref(co), ctx, None)
    if entry == "batch":
        arr = (CCamera * 2)(cc, cc)
        return L.rto_launch_renderer_batch(tree_h, arr, None, 2, C.byref(co), ctx, None)
    r = CRays()
    r.origins, r.dirs, r.t_max, r.background = w["origins"].data_ptr(), w["dirs"].data_ptr(), None, None
    r.n, r.first_ray = 8, 0
    return L.rto_launch_rays(tree_h, C.byref(r), C.byref(co), ctx, C.c_void_p(w["out"].data_ptr()), None)


# fault -> (tree, camera changes, option changes, code, entries it applies to, what the message says)
FAULTS = {
    "spp5": ("plain", {}, {"spp": 5}, E_SPP, ENTRIES, "spp =="),
    "compact_records_negative_threshold": ("compact", {}, {"sigma_thresh": -1.0}, E_UNSUPPORTED, ENTRIES, "sigma_thresh"),
    "sg_without_lobes": ("bare_sg", {}, {}, E_FORMAT, ENTRIES, "lobes"),
    "camera_8x8": ("plain", {"width": 8, "height": 8}, {}, E_INVALID, ("frame", "batch"), "camera size"),
    "fx_zero": ("plain", {"fx": 0.0}, {}, E_INVALID, ("frame", "batch"), "focal"),
    "null_tree": (None, {}, {}, E_INVALID, ENTRIES, "null argument"),
}


@pytest.mark.parametrize("entry,fault", [(e, f) for f, v in FAULTS.items() for e in v[4]])
def test_refusal(world, entry, fault):
    tree, camkw, optkw, code, _, says = FAULTS[fault]
    opt = R.RenderOptions(**{"spp": 1, **optkw})
    rc = _launch(entry, world, world[tree]._h if tree else None, _ccam(world["cam"], **camkw), opt)
    msg = R.lib().rto_last_error().decode()
    print(entry, fault, rc, msg)
    assert rc == code
    assert says in msg  # (the thread-local string could be a stale one: pin this fault's own wording)


def test_every_entry_renders_the_fixture(world):
    """the table's refusals are about the fault: the same calls without one succeed"""
    for entry in ENTRIES:
        assert _launch(entry, world, world["plain"]._h, _ccam(world["cam"]), R.RenderOptions(spp=1)) == 0, entry
        assert _launch(entry, world, world["compact"]._h, _ccam(world["cam"]), R.RenderOptions(spp=1)) == 0, entry


def test_a_refused_batch_leaves_the_context_as_it_was(world):
    ctx, cam = world["ctx"], world["cam"]
    R.launch_renderer_batch(world["plain"], [cam, cam], R.RenderOptions(spp=1), ctx)
    before = ctx.tile_marks()
    assert before is not None and before[3] == 2
    rc = _launch("batch", world, world["plain"]._h, _ccam(cam, width=8, height=8), R.RenderOptions(spp=1))
    assert rc == E_INVALID
    assert ctx.tile_marks() == before
    import torch
    torch.cuda.synchronize()
