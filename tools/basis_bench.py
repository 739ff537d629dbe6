"""Render frames/s of the same tree shaded through three bases: SH16, SG16 and ASG16 (GPU box).

The C2 shape of bench.py (depth-10 synthetic tree, shell 2.5, 800x800, SPP 6, batches of 100 orbit poses); the SG / ASG trees
are synth.with_lobes of the SH tree -- same child[], sigma and coefficients, so the traversal is the same and only the basis the
shading kernel evaluates per hit entry differs (SH16: ~220 instructions; SG16 / ASG16: 16 x (dot products + the full-range expf
+ a division)).  Render only (denoise off: the noisy image is the output).  Prints one JSON line per basis: frames/s over the timed
batches and the per-launch milliseconds of the traversal and shading kernels (HIP events)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import synth  # noqa: E402


def sh_tree(depth, basis, shell, threads):
    args = bench.parse_args(["--depth", str(depth), "--basis", str(basis), "--shell", str(shell)])
    path = bench.tree_cache_path(args).replace(".npz", "_basis_bench.npz")
    if os.path.exists(path):
        z = np.load(path)
        return synth.SynthTree(z["child"], z["data"], z["invradius3"], z["offset"], str(z["data_format"]), depth, {})
    t = synth.make_tree(depth_limit=depth, basis_dim=basis, shell=shell, sdf=bench.parallel_sdf(synth.scene_sdf, threads))
    t.save_npz(path)
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batches", type=int, default=10, help="timed batches per basis")
    ap.add_argument("--warmup", type=int, default=2, help="untimed batches per basis")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    t0 = time.time()
    sh = sh_tree(args.depth, args.basis, args.shell, args.threads)
    print("tree: capacity %d, %.1f s" % (sh.capacity, time.time() - t0), file=sys.stderr, flush=True)
    W = H = args.size
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(args.batch):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    opt = R.RenderOptions(spp=args.spp, denoise=False)
    for kind in ("SH", "SG", "ASG"):
        t = sh if kind == "SH" else synth.with_lobes(sh, kind, seed=1)
        dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format, extra_data=t.extra)
        ctx = R.RenderContext(W, H, frames=args.batch)
        ctx.rng_seed()
        for _ in range(args.warmup):
            R.launch_renderer_batch(dt, cams, opt, ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.batches):
            R.launch_renderer_batch(dt, cams, opt, ctx)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t1
        ctx.kernel_timing(True)
        for _ in range(args.batches):
            R.launch_renderer_batch(dt, cams, opt, ctx)
        kt = ctx.kernel_timing_read()
        print(json.dumps({"basis": t.data_format, "size": W, "spp": args.spp, "frames": args.batches * args.batch,
                          "frames_per_s": round(args.batches * args.batch / wall, 1),
                          "traverse_ms_per_launch": round(kt["traverse_ms"], 3), "shade_ms_per_launch": round(kt["shade_ms"], 3)}),
              flush=True)
        ctx.freeResource()
        dt.free()


if __name__ == "__main__":
    main()
