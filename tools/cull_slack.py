"""How loose is the empty-space culling?  On the bench scene (C2: 800 x 800, SPP 6) and a sample of the bench orbit's poses, per frame:
  (a) the 8x8 tiles the launch marks (the tile marks of the batched launch = the tiles whose rays are marched),
  (b) the tiles that hold at least one pixel with a hit (alpha > 0 in the aux planes of the full-output render),
and (b) / (a): the share of the marched tiles any tighter marking rule could keep at most.  One run prints both sets of culling
cells: the bounds of each cell's dense leaves (the default) and the cells' whole cubes (tuning "cull_cubes"; a library from
before that key prints its one rule).
python3 tools/cull_slack.py [--poses 25] [--size 800] [--out profiles/cull_slack.txt]   (RTO_LIB: another build of the library)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=25, help="poses sampled evenly from the 200 of the bench orbit")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import bench
    import rt_octree_amd as R
    from rt_octree_amd import synth
    from rt_octree_amd.volrend import _DevArray

    args = bench.parse_args(["--size", str(a.size)])
    path = bench.tree_cache_path(args)
    if not os.path.exists(path):
        th = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=args.radius,
                             sdf=bench.parallel_sdf(synth.scene_variant(0), bench.usable_cores()), seed=20230418)
        th.save_npz(path + ".tmp.npz")
        os.replace(path + ".tmp.npz", path)
    tree = R.N3Tree(path)
    W = H = a.size
    poses = synth.orbit_poses(200, radius=args.cam_radius)
    idx = [int(round(i * 200 / a.poses)) % 200 for i in range(a.poses)]
    fx = synth.blender_focal(W)
    cams = []
    for i in idx:
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(poses[i])
        cams.append(c)
    ctx = R.RenderContext(W, H, frames=len(cams))
    tx, ty = (W + 7) // 8, (H + 7) // 8
    lines = ["# %s: %d x %d, SPP %d, %d poses of the bench orbit; library %s" % (os.path.basename(path), W, H, args.spp, len(idx),
                                                                                os.environ.get("RTO_LIB", "this tree's"))]
    totals = {}
    for cubes in (0, 1):
        try:
            ctx.set_tuning("cull_cubes", cubes)
        except R.RtoError:  # (a library without the key: its only rule, once)
            if cubes:
                break
        rule = "cells = whole cubes (cull_cubes 1)" if cubes else "cells = the library's default (bounds of the dense leaves, where it has them)"
        ctx.rng_seed()
        R.launch_renderer_batch(tree, cams, R.RenderOptions(spp=args.spp, denoise=False), ctx, rng_jumps=[100 + i for i in idx])
        live, total = ctx.queue_stats()
        ptr, words, _s0, frames, _bg = ctx.tile_marks()
        marks = torch.as_tensor(_DevArray(ptr, (frames * words,), ctx), device="cuda:0").cpu().numpy().view(np.uint32).reshape(frames, words)
        lines += ["# ---- " + rule, "# pose  tiles  (a) marked  (b) with a hit pixel  (b)/(a)   (b) dilated by one tile / (a)"]
        sa = sb = sd = 0
        for f, i in enumerate(idx):
            bits = np.unpackbits(marks[f].view(np.uint8), bitorder="little")
            marked = np.ones(tx * ty, bool) if marks[f, -1] else bits[:tx * ty].astype(bool)
            ctx.select_frame(f)
            alpha = ctx.download_aux()[3] > 0  # (aux plane 3: the accumulated opacity)
            pad = np.zeros((ty * 8, tx * 8), bool)
            pad[:H, :W] = alpha
            hit = pad.reshape(ty, 8, tx, 8).any(axis=(1, 3))
            assert not np.any(hit.reshape(-1) & ~marked), "a tile with a hit pixel is not marked"
            grown = np.zeros((ty + 2, tx + 2), bool)  # a tile or one of its 8 neighbours holds a hit: what a rule that errs by < 8 px keeps
            for dy in range(3):
                for dx in range(3):
                    grown[dy:dy + ty, dx:dx + tx] |= hit
            na, nb, nd = int(marked.sum()), int(hit.sum()), int(grown[1:-1, 1:-1].sum())
            sa, sb, sd = sa + na, sb + nb, sd + nd
            lines.append("%5d  %5d  %10d  %20d  %7.3f  %7.3f" % (i, tx * ty, na, nb, nb / max(na, 1), nd / max(na, 1)))
        lines.append("# all   %5d  %10d  %20d  %7.3f  %7.3f   (queue_stats: %d live of %d tile slots)"
                     % (tx * ty * len(idx), sa, sb, sb / max(sa, 1), sd / max(sa, 1), live, total))
        totals[cubes] = sa
    if len(totals) == 2:
        lines.append("# marked from the bounds / marked from the cubes: %d / %d = %.4f" % (totals[0], totals[1], totals[0] / max(totals[1], 1)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
