"""Frames/s of batched launches over the layers of rto_ctx_set_layers, on the C2 tree and poses (GPU box).

100 frames of 800x800 at SPP 6 per launch, (a) offscreen, (b) over a depth layer, (c) over a depth and a colour layer -- render
only (denoise off, full outputs) and render + rto_denoise (RTO_FILTER_FACTORISED, full outputs).  The depth layer is the plane
through the volume centre that faces each camera (it cuts the object in half); the colour layer a gradient.  Prints one JSON line
per measurement: the median of --reps timed runs of --iters back-to-back launches each (HIP events), after warm-up launches, and
the ratio to the offscreen case of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import denoiser, synth  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from basis_bench import sh_tree  # noqa: E402
from rays_bench import timed  # noqa: E402


def plane_depth(t, cam):
    """[H, W] float32: distance along each pixel's unit ray to the plane through the volume centre that faces the camera"""
    _, d = R.camera_rays(cam)
    d = d.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = np.asarray(cam.transform, np.float64)
    centre = (0.5 - t.offset.astype(np.float64)) / t.scale.astype(np.float64)
    axis = -m[2]
    return (float(np.dot(centre - m[3], axis)) / (d @ axis)).reshape(cam.height, cam.width).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    t = sh_tree(args.depth, args.basis, args.shell, args.threads)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    W = H = args.size
    n = args.frames
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(200)[:n]:
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dev = torch.device("cuda", 0)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    for f, c in enumerate(cams):
        depth[f] = torch.from_numpy(plane_depth(t, c)).to(dev)
    u = torch.linspace(0, 1, W, device=dev)[None, None, :].expand(n, H, W)
    v = torch.linspace(0, 1, H, device=dev)[None, :, None].expand(n, H, W)
    color = torch.stack([0.1 + 0.8 * u, 0.9 - 0.7 * v, 0.2 + 0.3 * u * v, torch.ones_like(u)], -1).contiguous()
    torch.manual_seed(0)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval())
    ctx = R.RenderContext(W, H, frames=n)
    ctx.rng_seed()
    stream = torch.cuda.current_stream().cuda_stream
    base = {}
    for denoise in (False, True):
        opt = R.RenderOptions(spp=args.spp, denoise=denoise)

        def run():
            R.launch_renderer_batch(dt, cams, opt, ctx, stream=stream)
            if denoise:
                ctx.select_frame(0)
                net.denoise(ctx, n=n, mode=R.FILTER_FAST)

        for case, layers in (("a_offscreen", (None, None)), ("b_depth", (depth, None)), ("c_depth_colour", (depth, color))):
            ctx.set_layers(*layers)
            ms = timed(run, args.iters, args.reps)
            base.setdefault(denoise, ms)
            print(json.dumps(dict(case=case, stage="render+denoise" if denoise else "render", frames=n, size=W, spp=args.spp,
                                  ms_per_launch=round(ms, 4), frames_per_s=round(n / ms * 1e3, 1),
                                  ratio_to_offscreen=round(base[denoise] / ms, 4))), flush=True)


if __name__ == "__main__":
    main()
