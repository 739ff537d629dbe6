"""Rays/s of rto_launch_rays on the C2 tree at SPP 6 (GPU box), against the single-frame operator on the same camera.

(a) the C2 camera's 800x800 rays in raster order, (b) the same rays in 8x8-tile order, (c) 1 M random rays through the box
(incoherent: random origins on a sphere around it, aimed at random points inside), (d) launch_renderer on that camera with the
culling of the single-frame kernel off ("cull" 0, "cull_single" 0) -- the like-for-like baseline.  Each ray order is timed for
both workgroup-to-ray maps ("ray_order" 0: consecutive blocks of 256 rays, 1: one contiguous range per XCD).  Prints one JSON
line per measurement: the median of --reps timed runs of --iters back-to-back launches each (HIP events)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import synth  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from basis_bench import sh_tree  # noqa: E402


def timed(fn, iters, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--random", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    t = sh_tree(args.depth, args.basis, args.shell, args.threads)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    W = H = args.size
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(synth.orbit_poses(200)[0])
    opt = R.RenderOptions(spp=args.spp, denoise=False)
    ctx = R.RenderContext(W, H)
    ctx.rng_seed()
    dev = torch.device("cuda", 0)

    o, d = R.camera_rays(cam)
    raster = (torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev))
    ys, xs = np.divmod(np.arange(W * H), W)
    tile = np.lexsort((xs % 8, ys % 8, xs // 8, ys // 8))  # 8x8 tiles in raster order, pixels row-major inside a tile
    tiled = (raster[0][torch.as_tensor(tile, device=dev)].contiguous(), raster[1][torch.as_tensor(tile, device=dev)].contiguous())
    rng = np.random.default_rng(0)
    n = args.random
    u = rng.normal(size=(n, 3))
    lo, hi = (0 - t.offset) / t.scale, (1 - t.offset) / t.scale
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    start = (centre + radius * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    aim = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    rand = (torch.as_tensor(start, device=dev), torch.as_tensor(aim - start, device=dev))
    out = torch.empty((max(W * H, n), 4), dtype=torch.float32, device=dev)

    def line(case, rays, ms, **kw):
        print(json.dumps(dict(case=case, rays=rays, spp=args.spp, ms=round(ms, 4), rays_per_s=round(rays / ms * 1e3 / 1e9, 4),
                              unit="Grays/s", **kw)), flush=True)

    for order in (0, 1):
        ctx.set_tuning("ray_order", order)
        for case, (ro, rd) in (("a_raster", raster), ("b_tiles8", tiled), ("c_random", rand)):
            k = ro.shape[0]
            ms = timed(lambda: R.render_rays(dt, ro, rd, opt, ctx, out=out[:k]), args.iters, args.reps)
            line(case, k, ms, ray_order=order)
    ctx.set_tuning("cull", 0)
    ctx.set_tuning("cull_single", 0)
    ms = timed(lambda: R.launch_renderer(dt, cam, opt, ctx, stream=torch.cuda.current_stream().cuda_stream), args.iters, args.reps)
    line("d_frame", W * H, ms)


if __name__ == "__main__":
    main()
