"""Tile marks from the bounds of a culling cell's dense leaves (host/tree_layout.cpp culling_cells, mark_cell in render_kernels.hip):
a node of the culling level is projected as the axis-aligned bounds of the dense leaves below it, not as its whole cube, and the
absolute pad of the projected rectangle is 0.5 pixels.  Tuning key "cull_cubes" marks from the whole cubes, same pad.

  fewer tiles       dense leaves that fill one corner octant of one level-7 cell: the tiles only the rest of the cube projects
                    into stay unmarked, the tiles the octant projects into are marked; the single-frame kernel marks the same
  a subset          for every pose of every case here the marks from the bounds lie within the marks from the cubes
  coarse leaf       a dense leaf coarser than the culling level is its own cell: the same marks either way
  same pixels       culling on == culling off, bit for bit: anisotropic and off-centre world frames under a sheared camera, a
                    camera inside a cell's bounds (every tile kept), every cell behind the camera (no tile kept)
  the pad           16 seeded random poses: no tile that holds a pixel with alpha > 0 in the culling-off render is unmarked
  the host          culling_cells under ASan + UBSan, a stand-alone program on the CPU (tools/sanitize/run_culling.sh)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rt_octree_amd as R
from helpers import FRAMES, aim_point, assert_bits_equal, reframe, reframe_pose
from rt_octree_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCC_LEVEL, MARGIN = 7, 1e-4  # rto_tree_bits.h kOccLevel; host/tree_layout.cpp culling_cells
W = H = 128
TX = TY = 16
PAD = 0.5  # render_kernels.hip kMarkPad
# what the marked rectangle may exceed the float64 projection of the padded box by: PAD plus the relative pad, a ball of radius
# e = 1e-5 (|p|_1 |M^-1|_F + r) round each corner, on the image f e / D (1 + |x|) pixels -- with the cameras below (|p|_1 < 1,
# |M^-1|_F < 2.5, D > 0.08, f = 200, |x| < 0.5) under 0.1 pixel; float32 rounding is another 1e-4
SLACK = PAD + 0.1


def dev(t):
    return R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)


def camera(pose, fx, fy=None):
    c = R.Camera(W, H, float(np.float32(fx)), float(np.float32(fx if fy is None else fy)))
    c.set_c2w(pose)
    return c


def sheared(cam):
    """the same camera with a matrix that is no rotation (mark_cell inverts it by Cramer's rule; the rays use it as it is)"""
    cam.transform[0] += np.float32(0.3) * cam.transform[1]
    cam.transform[2] -= np.float32(0.2) * cam.transform[0]
    return cam


def tile_marks(ctx, n):
    import torch
    from rt_octree_amd.volrend import _DevArray
    ptr, words, _s0, frames, _bg = ctx.tile_marks()
    assert frames == n
    torch.cuda.synchronize()
    m = torch.as_tensor(_DevArray(ptr, (n * words,), ctx), device="cuda:0").cpu().numpy().view(np.uint32).reshape(n, words)
    bits = np.unpackbits(m.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :TX * TY].astype(bool)
    return (bits | (m[:, -1:] != 0)).reshape(n, TY, TX)  # (the last word: keep every tile of the frame)


def render(dt, cams, ctx, cull, cubes=False):
    """-> (aux, noisy) of the batch, its tile marks (None with the culling off)"""
    import torch
    n = len(cams)
    ctx.set_tuning("cull", int(cull))
    ctx.set_tuning("cull_cubes", int(cubes))
    ctx.rng_seed()
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=4, denoise=False), ctx, rng_jumps=[50 + f for f in range(n)])
    torch.cuda.synchronize()
    aux, noisy, _ = (torch.as_tensor(v, device="cuda:0")[:n].cpu().numpy() for v in ctx.batch_views())
    marks = tile_marks(ctx, n) if cull else None
    ctx.set_tuning("cull_cubes", 0)
    ctx.set_tuning("cull", 1)
    return (aux, noisy), marks


def hit_tiles(aux):
    """[n, TY, TX]: the tiles that hold a pixel with alpha > 0 (aux plane 3: the accumulated opacity)"""
    return (aux[:, 3] > 0).reshape(len(aux), TY, 8, TX, 8).any(axis=(2, 4))


def check(dt, cams, ctx, what):
    """The three renders of a case: bounds, cubes, culling off.  Pixels equal bit for bit, every tile with a hit pixel marked, the
    marks from the bounds a subset of the marks from the cubes.  -> (marks from the bounds, from the cubes, tiles with a hit)"""
    off, _ = render(dt, cams, ctx, False)
    tight, m_tight = render(dt, cams, ctx, True)
    cubes, m_cubes = render(dt, cams, ctx, True, cubes=True)
    for k, name in enumerate(("aux", "noisy")):
        assert_bits_equal(tight[k], off[k], "%s: %s, bounds against culling off" % (what, name))
        assert_bits_equal(cubes[k], off[k], "%s: %s, cubes against culling off" % (what, name))
    hit = hit_tiles(off[0])
    assert not np.any(hit & ~m_tight), "%s: a tile with a hit pixel is not marked" % what
    assert not np.any(m_tight & ~m_cubes), "%s: the bounds mark a tile the cubes do not" % what
    print("%s: tiles marked from the bounds %s, from the cubes %s, with a hit pixel %s"
          % (what, m_tight.sum(axis=(1, 2)).tolist(), m_cubes.sum(axis=(1, 2)).tolist(), hit.sum(axis=(1, 2)).tolist()))
    return m_tight, m_cubes, hit


@pytest.fixture(scope="module")
def ctx4():
    return R.RenderContext(W, H, frames=4)


@pytest.fixture(scope="module")
def scene():
    return synth.make_tree(depth_limit=8, basis_dim=9, seed=21, shell=2.0)


# ------------------------------------------------------------------ one corner octant of one level-7 cell
Q7 = (37, 90, 61)  # the level-7 cell, integer coordinates


def chain_tree(q, level, fill, basis=9):
    """a chain of nodes down to the node of cell q of `level`, all eight slots of that node dense (fill = True: the cell is full of
    leaves of level + 1) or followed by one more node in its low corner octant whose eight slots are dense (leaves of level + 2)"""
    nodes = level + (1 if fill else 2)
    child = np.zeros((nodes, 2, 2, 2), np.int32)
    data = np.zeros((nodes, 2, 2, 2, 3 * basis + 1), np.float16)
    for n in range(level):
        child[(n,) + tuple((int(v) >> (level - 1 - n)) & 1 for v in q)] = 1
    if not fill:
        child[level, 0, 0, 0] = 1
    data[nodes - 1, ..., :-1] = np.random.default_rng(5).normal(0.0, 0.6, (2, 2, 2, 3 * basis))
    data[nodes - 1, ..., -1] = 3000.0
    return synth.SynthTree(child, data, (1.0 / 3.0,) * 3, (0.5,) * 3, "SH%d" % basis, nodes, {})


def world_box(tree, lo, hi):
    """tree-space box [lo, hi] -> world (centre, half-widths with culling_cells' margin)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    scale, offset = tree.scale.astype(np.float64), tree.offset.astype(np.float64)
    return (0.5 * (lo + hi) - offset) / scale, (0.5 * (hi - lo) + MARGIN) / np.abs(scale)


def projected_tiles(centre, hw, cam, pad):
    """[TY, TX]: the tiles of the bounding rectangle of the box's 8 projected corners (float64; all in front of the camera), widened
    by `pad` pixels (negative: narrowed)"""
    m = np.asarray(cam.transform, np.float64)
    Mi = np.linalg.inv(m[:3].T)
    px, py = [], []
    for s in range(8):
        sign = np.array([1.0 if s & 4 else -1.0, 1.0 if s & 2 else -1.0, 1.0 if s & 1 else -1.0])
        a, b, c = Mi @ (centre + sign * hw - m[3])
        assert -c > 0.0
        px.append(0.5 * W + cam.fx * a / -c)
        py.append(0.5 * H - cam.fy * b / -c)
    out = np.zeros((TY, TX), bool)
    x0, x1 = int(np.floor((min(px) - pad) / 8.0)), int(np.floor((max(px) + pad) / 8.0))
    y0, y1 = int(np.floor((min(py) - pad) / 8.0)), int(np.floor((max(py) + pad) / 8.0))
    if x1 >= x0 and y1 >= y0:
        out[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
    return out


def octant_case():
    tree = chain_tree(Q7, OCC_LEVEL, fill=False)
    size = 2.0 ** -OCC_LEVEL
    lo = np.array(Q7) * size
    cube = world_box(tree, lo, lo + size)
    octant = world_box(tree, lo, lo + 0.5 * size)
    # from 0.12 world units the cube (3 / 128 = 0.023 units) is ~40 pixels at fx = 200: 5 tiles or more, the octant half that
    cams = [camera(synth.look_at_c2w(cube[0] + 0.12 * np.array(d) / np.linalg.norm(d), cube[0]), 200.0)
            for d in ((1.0, 0.2, 0.3), (-0.3, 1.0, 0.4), (0.2, -0.4, 1.0), (-1.0, -0.8, -0.5))]
    return tree, cube, octant, cams


@pytest.mark.gpu
def test_bounds_of_a_corner_octant_mark_fewer_tiles_than_the_cube(ctx4):
    tree, cube, octant, cams = octant_case()
    dt = dev(tree)
    m_tight, m_cubes, hit = check(dt, cams, ctx4, "corner octant")
    assert hit.any(axis=(1, 2)).all()
    one = R.RenderContext(W, H)
    one.rng_seed()
    one.set_tuning("cull_single", 1)
    one.set_kernel(R.KERNEL_FAST)
    for f, cam in enumerate(cams):
        inside = projected_tiles(octant[0], octant[1] - MARGIN / abs(float(tree.scale[0])), cam, 0.0)  # the leaves themselves
        outer = projected_tiles(octant[0], octant[1], cam, SLACK)
        whole = projected_tiles(cube[0], cube[1], cam, -SLACK)  # tiles well inside the cube's rectangle: the cube rule marks them
        assert whole.any(axis=0).sum() >= 3 and whole.any(axis=1).sum() >= 3  # the cube spans 3 tiles or more each way
        assert not np.any(inside & ~m_tight[f]), "pose %d: a tile the dense octant projects into is not marked" % f
        assert not np.any(m_tight[f] & ~outer), "pose %d: tiles marked beyond the octant's padded rectangle" % f
        empty = whole & ~outer  # what only the empty part of the cube projects into
        assert empty.any() and not np.any(m_tight[f] & empty) and m_cubes[f][empty].all(), "pose %d" % f
        assert m_tight[f].sum() < m_cubes[f].sum()
        # the single-frame kernel (mark_tiles_one_kernel) marks what the batch marks
        for cubes, want in ((0, m_tight[f]), (1, m_cubes[f])):
            one.set_tuning("cull_cubes", cubes)
            R.launch_renderer(dt, cam, R.RenderOptions(spp=4, denoise=False), one)
            assert np.array_equal(tile_marks(one, 1)[0], want), "pose %d, cull_cubes %d: single-frame marks" % (f, cubes)
    dt.free()


@pytest.mark.gpu
def test_a_full_cell_and_a_coarse_leaf_mark_the_same_tiles_either_way(ctx4):
    """a level-7 cell whose eight octants are all dense has its cube for bounds; a dense leaf coarser than the culling level is
    emitted as its own cube"""
    full = chain_tree(Q7, OCC_LEVEL, fill=True)
    coarse = chain_tree((2, 1, 3), 2, fill=True)  # eight dense leaves of level 3
    _, cube, _, cams = octant_case()
    for what, tree, cs in (("full cell", full, cams),
                           ("coarse leaf", coarse, [camera(p, 90.0, 120.0) for p in synth.orbit_poses(4)])):
        dt = dev(tree)
        m_tight, m_cubes, hit = check(dt, cs, ctx4, what)
        assert np.array_equal(m_tight, m_cubes), what
        assert hit.any() and not m_tight.all(axis=(1, 2)).any()
        dt.free()


# ------------------------------------------------------------------ scenes
@pytest.mark.gpu
@pytest.mark.parametrize("frame", ["cube", "aniso", "off_centre"])
def test_scene_frames_equal_marched_ones_and_bounds_mark_a_subset(ctx4, scene, frame):
    """(cube: synth.make_tree's own world; the others: tests/test_reframed_trees.py's, under a camera matrix that is no rotation)"""
    t = scene if frame == "cube" else reframe(scene, *FRAMES[frame])
    poses = [reframe_pose(p, scene, t, target=aim_point(p)) for p in synth.orbit_poses(4)]
    cams = [camera(p, 150.0, 130.0) for p in poses]
    if frame != "cube":
        cams = [sheared(c) for c in cams]
    dt = dev(t)
    m_tight, m_cubes, hit = check(dt, cams, ctx4, frame)
    n = m_tight.sum(axis=(1, 2))
    assert (n > 0).all() and (n < TX * TY).all()  # an object in empty space
    dt.free()


@pytest.mark.gpu
def test_near_and_behind_the_camera(ctx4, scene):
    tree, cube, octant, _ = octant_case()
    look = lambda pos, target: camera(synth.look_at_c2w(pos, target), 120.0)
    # 0: inside the octant's bounds -- corners on both sides of the camera plane (nearer than 100 e), the sphere rule at d < 2 r:
    #    every tile is kept
    # 1: in the empty part of the cube, at its far corner, looking at the octant: the cube keeps every tile, the bounds need not
    # 2: the cell behind the camera: no tile; 3: an ordinary pose
    cams = [look(octant[0], octant[0] + np.array([1.0, 0.3, 0.2])), look(cube[0] + 0.95 * cube[1], octant[0]),
            look(octant[0] + np.array([0.5, 0.0, 0.0]), octant[0] + np.array([2.0, 0.1, 0.0])),
            look(octant[0] + np.array([0.1, 0.0, 0.3]), octant[0])]
    dt = dev(tree)
    m_tight, m_cubes, _ = check(dt, cams, ctx4, "octant, near and behind")
    assert m_tight[0].all() and m_cubes[0].all() and m_cubes[1].all()
    assert not m_tight[2].any() and not m_cubes[2].any()
    assert 0 < m_tight[3].sum() < TX * TY
    dt.free()
    # the scene: a camera inside its bounding box, in the shell; one that looks away from all of it
    cams = [look((0.2, 0.1, 0.3), (0.0, 0.0, 0.0)), look((3.0, 0.0, 1.0), (9.0, 0.0, 1.0))]
    dt = dev(scene)
    m_tight, m_cubes, _ = check(dt, cams, ctx4, "scene, near and behind")
    assert m_tight[0].all() and not m_tight[1].any() and not m_cubes[1].any()
    dt.free()


@pytest.mark.gpu
def test_half_pixel_pad_misses_no_tile_over_random_poses(scene):
    """a condition, not a measurement: zero tiles with a hit pixel unmarked (the render with the culling on is compared too)"""
    rng = np.random.default_rng(20250117)
    cams = []
    for i in range(16):
        d = rng.normal(size=3)
        pos = d / np.linalg.norm(d) * rng.uniform(1.6, 5.0)
        target = rng.normal(size=3) * 0.5
        if abs(np.dot((target - pos) / np.linalg.norm(target - pos), (0, 0, 1))) > 0.99:
            target = target + np.array([0.5, 0.0, 0.0])  # (look_at_c2w's up vector)
        fx, fy = rng.uniform(90.0, 400.0, 2)
        cams.append(camera(synth.look_at_c2w(pos, target), fx, fy))
    ctx = R.RenderContext(W, H, frames=16)
    dt = dev(scene)
    m_tight, _, hit = check(dt, cams, ctx, "random poses")
    assert int((hit & ~m_tight).sum()) == 0
    assert hit.sum() > 200 and (m_tight.sum(axis=(1, 2)) < TX * TY).any()  # the sweep saw the object, and frames with culled tiles
    dt.free()


# ------------------------------------------------------------------ CPU
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_culling_cells_are_clean_under_asan_ubsan():
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "run_culling.sh"), "200"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "clean under ASan + UBSan" in out and "bounds tighter than the cube" in out, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
