"""Tile marks from projected boxes (mark_cell in render_kernels.hip): a culling cell marks the tiles of the bounding rectangle of
its 8 projected corners, clamped by the rectangle of the bounding-sphere rule it replaces.

  never too tight   frames with the culling on and off are bit-identical, full outputs and lean, batches of 1 and 5: trees of ONE
                    dense leaf placed so that its projection straddles a tile corner, a tile edge, the image border, or covers
                    less than a pixel; and a scene under cameras that stress the projection (fx != fy, negative focal lengths,
                    scaled and sheared camera matrices, an anisotropic off-centre world frame, cameras near, grazing and inside
                    the volume, cells partly and wholly behind the camera, NaN poses)
  a lower bound     every tile that holds a pixel with alpha > 0 in the culling-off render is marked
  never looser      over a few hundred random (cell, camera) pairs every tile the GPU marks is one the sphere rule marks; that rule
                    is restated here in float64 from its formula: a ball of radius r = 1.001 |hw| 1.0001 |M^-1|_F round the cell
                    centre at camera coordinates (a, b, -d): nothing if d <= -r, every tile unless d > 2 r, else the tiles of
                    centre pixel +- (f r / (d - r) (1 + |a| / d) + 1.5) along x, the same with b along y
(The marks exist only as the kernel's output, so there is no CPU variant.)"""
import numpy as np
import pytest

import rt_octree_amd as R
from helpers import FRAMES, aim_point, assert_bits_equal, reframe, reframe_pose
from rt_octree_amd import synth
from rt_octree_amd.volrend import _DevArray

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OCC_LEVEL, MARGIN = 7, 1e-4  # rto_tree_bits.h kOccLevel; host/tree_layout.cpp culling_cells
W, H = 72, 56
TX, TY = 9, 7


def leaf_tree(q, level, frame=((1.0 / 3.0,) * 3, (0.5,) * 3), sigma=3000.0, basis=9):
    """a tree whose only leaf of positive density is the cell q (integer coordinates) of size 2^-level: a chain of `level` nodes"""
    child = np.zeros((level, 2, 2, 2), np.int32)
    data = np.zeros((level, 2, 2, 2, 3 * basis + 1), np.float16)
    for n in range(level):
        ix, iy, iz = [(int(v) >> (level - 1 - n)) & 1 for v in q]
        if n < level - 1:
            child[n, ix, iy, iz] = 1
        else:
            data[n, ix, iy, iz, :-1] = np.random.default_rng(5).normal(0.0, 0.6, 3 * basis)
            data[n, ix, iy, iz, -1] = sigma
    return synth.SynthTree(child, data, frame[0], frame[1], "SH%d" % basis, level, {})


def cell_world(tree, q, level):
    """centre (as the float32 the device holds) and half-widths of the culling cell of leaf q, in world coordinates"""
    lc = min(level, OCC_LEVEL)
    qc = np.array([int(v) >> (level - lc) for v in q], np.float64)
    size = 2.0 ** -lc
    scale, offset = tree.scale.astype(np.float64), tree.offset.astype(np.float64)
    centre = (((qc + 0.5) * size - offset) / scale).astype(np.float32).astype(np.float64)
    return centre, (0.5 * size + MARGIN) / np.abs(scale)


def dev(t):
    return R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)


def camera(pose, fx, fy=None):
    fx, fy = float(np.float32(fx)), float(np.float32(fx if fy is None else fy))  # (the values the kernels get)
    c = R.Camera(W, H, abs(fx), abs(fy))
    c.fx, c.fy = fx, fy  # (the constructor takes positive values only)
    c.set_c2w(pose)
    return c


def pose_with_point_at(point, pos, u, v, fx, fy):
    """a look-at pose near `pos` under which `point` projects to the pixel coordinates (u, v): look at the point, then move
    the camera sideways without turning it (pixel x = W / 2 + fx a / d, y = H / 2 - fy b / d)"""
    pose = synth.look_at_c2w(pos, point)
    dist = np.linalg.norm(np.asarray(pos, np.float64) - point)
    pose[:3, 3] += pose[:3, 0] * (-(u - 0.5 * W) * dist / fx) + pose[:3, 1] * ((v - 0.5 * H) * dist / fy)
    return pose


def tile_marks(ctx, n):
    ptr, words, _s0, frames, _bg = ctx.tile_marks()
    assert frames == n
    torch.cuda.synchronize()
    m = torch.as_tensor(_DevArray(ptr, (n * words,), ctx), device="cuda:0").cpu().numpy().view(np.uint32).reshape(n, words)
    bits = np.unpackbits(m.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :TX * TY].astype(bool)
    return (bits | (m[:, -1:] != 0)).reshape(n, TY, TX)  # (the last word: keep every tile of the frame)


def render(dt, cams, ctx, cull, lean, jumps):
    n = len(cams)
    ctx.set_tuning("cull", int(cull))
    ctx.set_lean_outputs(1 if lean else 0)
    ctx.rng_seed()
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=6, denoise=bool(lean)), ctx, rng_jumps=jumps)
    ctx.set_lean_outputs(0)
    torch.cuda.synchronize()
    aux, noisy, image = (torch.as_tensor(v, device="cuda:0")[:n].cpu().numpy() for v in ctx.batch_views())
    live, total = ctx.queue_stats()
    assert total == n * TX * TY
    return {"aux": aux, "noisy": noisy, "image": image}, (tile_marks(ctx, n) if cull else None), live


def check_on_equals_off(dt, cams, ctxs, what):
    """culling on == culling off, bit for bit, in batches of 1 and of 5, full outputs and lean; the marks hold every tile with a
    hit pixel.  -> the marks [len(cams), TY, TX]"""
    marks_all = np.zeros((len(cams), TY, TX), bool)
    for size in (1, 5):
        ctx = ctxs[size]
        for f0 in range(0, len(cams), size):
            part = cams[f0:f0 + size]
            jumps = [100 + f for f in range(f0, f0 + len(part))]
            for lean in (False, True):
                on, marks, live = render(dt, part, ctx, True, lean, jumps)
                off, _, live_off = render(dt, part, ctx, False, lean, jumps)
                assert live_off == len(part) * TX * TY and live == int(marks.sum())
                for k in on:
                    assert_bits_equal(on[k], off[k], "%s: %s, frames %d.., batch of %d, lean %d" % (what, k, f0, size, lean))
                if not lean:
                    hit = np.zeros((len(part), TY * 8, TX * 8), bool)
                    hit[:, :H, :W] = off["aux"][:, 3] > 0
                    hit = hit.reshape(len(part), TY, 8, TX, 8).any(axis=(2, 4))
                    assert not np.any(hit & ~marks), "%s: a tile with a hit pixel is not marked (frames %d..)" % (what, f0)
                    if size == 1:
                        marks_all[f0] = marks[0]
                    else:
                        assert np.array_equal(marks_all[f0:f0 + len(part)], marks), "the marks depend on the batch"
    return marks_all


@pytest.fixture(scope="module")
def ctxs():
    return {1: R.RenderContext(W, H, frames=1), 5: R.RenderContext(W, H, frames=5)}


# where the leaf's centre lands: (u, v) pixel coordinates; 8 | u: a tile edge.  The level-5 leaf is ~5 pixels across from 2 units away
SPOTS = {
    "tile corner": (5, 2.0, [(32.0, 24.0), (32.4, 23.7), (40.0, 16.0), (31.0, 25.0), (33.5, 22.5)]),
    "tile edge": (5, 2.0, [(32.0, 28.0), (36.0, 24.0), (31.6, 44.0), (20.0, 40.3), (48.2, 12.0)]),
    "image border": (5, 2.0, [(0.0, 28.0), (71.5, 28.0), (36.0, 0.0), (36.0, 55.6), (-1.5, -1.5)]),
    "sub-pixel": (8, 5.0, [(32.0, 24.0), (31.7, 24.3), (12.5, 4.5), (0.2, 28.0), (71.0, 55.0)]),  # the level-7 cell is 0.6 pixels
    "coarse leaf": (3, 4.0, [(32.0, 24.0), (20.0, 30.0), (70.0, 50.0), (-3.0, 28.0), (36.0, 28.0)]),  # a cell above the culling level
}


@pytest.mark.parametrize("spot", list(SPOTS))
def test_a_single_dense_leaf_is_never_culled(ctxs, spot):
    level, dist, uvs = SPOTS[spot]
    q = [(5 << level) >> 4, (9 << level) >> 4, (11 << level) >> 4]  # a cell away from the volume's centre
    tree = leaf_tree(q, level)
    centre, _ = cell_world(tree, q, level)
    leaf = ((np.array(q) + 0.5) * 2.0 ** -level - 0.5) * 3.0  # the leaf's own centre (below the culling level: not its cell's)
    fx, fy = 110.0, 95.0
    cams = []
    for i, (u, v) in enumerate(uvs):
        direction = np.array([np.cos(1.3 * i), np.sin(1.3 * i), 0.35 + 0.1 * i])
        cams.append(camera(pose_with_point_at(leaf, leaf + dist * direction / np.linalg.norm(direction), u, v, fx, fy), fx, fy))
    dt = dev(tree)
    marks = check_on_equals_off(dt, cams, ctxs, spot)
    assert marks.any(axis=(1, 2)).all() and (marks.sum(axis=(1, 2)) <= (9 if level > 3 else TX * TY - 1)).all(), marks.sum(axis=(1, 2))
    dt.free()


def stress_cameras(t0, t):
    """cameras of t0's world (synth.make_tree's) mapped into t's"""
    def look(pos, target=(0, 0, 0)):
        return reframe_pose(synth.look_at_c2w(pos, target), t0, t, target=np.asarray(target, np.float64))

    orbit = [reframe_pose(p, t0, t, target=aim_point(p)) for p in synth.orbit_poses(4)]
    cams = [camera(orbit[0], 90.0, 120.0), camera(orbit[1], -90.0, 120.0), camera(orbit[2], 100.0, -70.0), camera(orbit[3], -80.0, -80.0)]
    scaled = camera(orbit[1], 90.0)
    scaled.transform[:3] *= np.float32(1.7)    # a scaled camera matrix: directions are normalised anyway
    sheared = camera(orbit[2], 90.0, 110.0)
    sheared.transform[0] += np.float32(0.3) * sheared.transform[1]
    sheared.transform[2] -= np.float32(0.2) * sheared.transform[0]
    cams += [scaled, sheared]
    cams.append(camera(look((0.2, 0.1, 0.3)), 90.0))                            # inside the volume
    cams.append(camera(look((1.2, 1.2, 0.4)), 90.0, 75.0))                      # close, grazing a corner
    cams.append(camera(look((0.75, 0.0, 0.1), (0.75, 3.0, 0.1)), 60.0))         # near the surface, looking along it: cells on both sides of the camera plane
    cams.append(camera(look((0.0, -0.9, 0.5), (2.0, -0.9, 0.4)), 45.0, 60.0))   # the same from another side, wide angle
    cams.append(camera(look((3.0, 0.0, 1.0), (9.0, 0.0, 1.0)), 90.0))           # looking away: every cell behind the camera
    cams.append(camera(look((2.5, 2.5, 0.2), (0.0, 3.0, 0.0)), 90.0))           # the object at the edge of the frame
    cams.append(camera(look((9.0, 0.5, 1.0)), 90.0))                            # far away: the object is a few tiles
    nan_centre = camera(orbit[0], 90.0)
    nan_centre.transform[3, 1] = np.nan
    nan_axis = camera(orbit[3], 90.0)
    nan_axis.transform[0, 2] = np.nan
    cams += [nan_centre, nan_axis]
    return cams


@pytest.mark.parametrize("frame", ["cube", "aniso"])
def test_culled_frames_equal_marched_ones_under_stress_cameras(ctxs, frame):
    t0 = synth.make_tree(depth_limit=7, basis_dim=9, seed=21, shell=2.0)
    t = t0 if frame == "cube" else reframe(t0, *FRAMES["aniso"])  # (0.5, 0.25, 0.3) / (0.55, 0.4, 0.5): tests/test_reframed_trees.py
    cams = stress_cameras(t0, t)
    assert len(cams) == 15
    dt = dev(t)
    marks = check_on_equals_off(dt, cams, ctxs, frame)
    n = marks.sum(axis=(1, 2))
    assert (n[:4] < TX * TY).all() and (n[:4] > 0).all()   # the orbit poses see an object in empty space
    assert n[6] == TX * TY                                 # inside the volume: every tile
    assert n[10] == 0                                      # looking away: none
    assert n[13] == TX * TY and n[14] == TX * TY           # a NaN pose keeps every tile
    dt.free()


def sphere_rule(centre, hw, cam):
    """the tiles the sphere rule marks, in float64 (see the module's text) -> [TY, TX]"""
    m = np.asarray(cam.transform, np.float64)
    M = m[:3].T  # columns: the camera axes
    Mi = np.linalg.inv(M)
    a, b, c = Mi @ (centre - m[3])
    d = -c
    r = np.sqrt(np.sum(hw * hw)) * 1.001 * np.sqrt(np.sum(Mi * Mi)) * 1.0001
    out = np.zeros((TY, TX), bool)
    if d <= -r:
        return out
    if not d > 2.0 * r:
        return ~out
    k = r / (d - r)
    pxc, pyc = 0.5 * W + cam.fx * a / d, 0.5 * H - cam.fy * b / d
    rx, ry = abs(cam.fx) * k * (1.0 + abs(a / d)) + 1.5, abs(cam.fy) * k * (1.0 + abs(b / d)) + 1.5
    x0, x1 = int(np.floor((pxc - rx) / 8.0)), int(np.floor((pxc + rx) / 8.0))
    y0, y1 = int(np.floor((pyc - ry) / 8.0)), int(np.floor((pyc + ry) / 8.0))
    out[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
    return out


def test_marks_are_a_subset_of_the_sphere_rules():
    rng = np.random.default_rng(20240611)
    cells = [((37, 90, 61), 7, ((1.0 / 3.0,) * 3, (0.5,) * 3)),      # a cell of the culling level
             ((150, 33, 201), 8, FRAMES["aniso"]),                   # a finer leaf: the cell is its parent's cube; anisotropic frame
             ((9, 20, 14), 5, FRAMES["aniso_perm"]),                 # a coarse leaf is its own cell
             ((1, 2, 1), 2, ((0.01, 0.012, 0.008), (0.45, 0.5, 0.6)))]  # a quarter of a world some hundred units across
    n = 96
    ctx = R.RenderContext(W, H, frames=n)
    gpu_tiles = model_tiles = boxes = 0
    for q, level, frame in cells:
        tree = leaf_tree(q, level, frame)
        centre, hw = cell_world(tree, q, level)
        size = 2.0 * float(np.max(hw))
        cams = []
        for i in range(n):
            direction = rng.normal(size=3)
            direction /= np.linalg.norm(direction)
            dist = size * float(np.exp(rng.uniform(np.log(0.3), np.log(60.0))))  # inside the sphere's keep-all range ... a speck
            pos = centre + dist * direction
            target = centre + rng.normal(size=3) * dist * (0.4 if i % 3 else 1.5)  # mostly in view; some out of it or behind
            if abs(np.dot((target - pos) / np.linalg.norm(target - pos), (0, 0, 1))) > 0.99:
                target = target + np.array([0.3, 0.0, 0.0]) * dist  # (look_at_c2w's up vector)
            fx, fy = rng.uniform(30.0, 300.0, 2) * rng.choice([1.0, 1.0, -1.0], 2)
            c = camera(synth.look_at_c2w(pos, target), fx, fy)
            if i % 4 == 1:
                c.transform[:3] += rng.normal(0.0, 0.15, (3, 3)).astype(np.float32)  # not orthonormal
            cams.append(c)
        dt = dev(tree)
        ctx.set_tuning("cull", 1)
        ctx.rng_seed()
        R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=1, denoise=False), ctx, rng_jumps=list(range(n)))
        got = tile_marks(ctx, n)
        for f in range(n):
            want = sphere_rule(centre, hw, cams[f])
            assert not np.any(got[f] & ~want), "cell %r, camera %d: tiles %s marked beyond the sphere rule's" % (
                q, f, np.argwhere(got[f] & ~want).tolist())
            gpu_tiles += int(got[f].sum())
            model_tiles += int(want.sum())
            boxes += int(want.all() and not got[f].all())
        dt.free()
    print("tiles marked: %d, by the sphere rule: %d; frames the sphere rule keeps whole and the box rule does not: %d"
          % (gpu_tiles, model_tiles, boxes))
    # and it is tighter: the cameras between ~1 and ~3 cell sizes away that look at the cell see all of it in front of them while
    # the sphere rule (2 r = 6 half-edges for an orthonormal camera) still keeps the whole frame
    assert gpu_tiles < model_tiles and boxes > 0
