"""What the depth outputs cost on the C2 tree at SPP 6 (GPU box): rays/s of rto_launch_rays_ex with and without depth / t_near, and
single-frame frames/s of rto_launch_renderer on a context with and without rto_ctx_enable_depth.

Rays: the C2 camera's 800x800 rays in raster order and 1 M random rays through the box (tools/rays_bench.py's cases a and c),
each with rgba alone (render_rays: the yardstick, the kernel rto_launch_rays runs), with rgba + depth + t_near
(render_rays_depth) and with the two depth outputs alone (no colour computed).  Frames: launch_renderer on that camera, the
fast kernel, without depth (render_fast), with it (render_fast_layers_depth), and over a depth + colour layer without / with it
(render_fast_layers / render_fast_layers_depth).  Prints one JSON line per measurement -- the median of --reps timed runs of
--iters back-to-back launches each (HIP events) -- and one line of ratios (with / without) at the end.

Batch (--cases batch): --batch-frames frames (100) of the C2 orbit in one rto_launch_renderer_batch, render only, on three contexts --
(a) no depth outputs, (b) rto_ctx_enable_depth(1): frame by frame through the single-frame depth kernels, (c) RTO_DEPTH_BATCHED:
the persistent kernels with render_persist_depth.  ms per launch from HIP events: 3 warm-up launches each, then 7 rounds in which
the three take turns with 5 back-to-back launches each, all in this one process; median and minimum of the 7 per route, the
ratios (c) / (b) and (c) / (a), and whether the median of (c) lies below the fastest repeat of (b)."""
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
from rays_bench import timed  # noqa: E402


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
    ap.add_argument("--cases", default="rays,frames,batch", help="comma-separated: rays, frames, batch")
    ap.add_argument("--batch-frames", type=int, default=100)
    args = ap.parse_args()
    cases = set(args.cases.split(","))
    import ctypes as C

    import torch
    from rt_octree_amd import _lib
    t = sh_tree(args.depth, args.basis, args.shell, args.threads)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    W = H = args.size
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    cam.set_c2w(synth.orbit_poses(200)[0])
    opt = R.RenderOptions(spp=args.spp, denoise=False)
    dev = torch.device("cuda", 0)
    ctx = R.RenderContext(W, H)
    ctx.rng_seed()

    o, d = R.camera_rays(cam)
    raster = (torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev))
    rng = np.random.default_rng(0)
    n = args.random
    u = rng.normal(size=(n, 3))
    lo, hi = (0 - t.offset) / t.scale, (1 - t.offset) / t.scale
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    start = (centre + radius * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    aim = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    rand = (torch.as_tensor(start, device=dev), torch.as_tensor(aim - start, device=dev))
    cap = max(W * H, n)
    rgba = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    depth = torch.empty((cap,), dtype=torch.float32, device=dev)
    near = torch.empty((cap,), dtype=torch.float32, device=dev)
    co = opt.to_c()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = {}

    def line(case, count, ms, unit, **kw):
        results[case] = ms
        rate = count / ms * 1e3
        print(json.dumps(dict(case=case, spp=args.spp, ms=round(ms, 4), rate=round(rate / 1e9, 4) if unit == "Grays/s" else round(rate, 1),
                              unit=unit, **kw)), flush=True)

    for name, (ro, rd) in (("raster", raster), ("random", rand)) if "rays" in cases else ():
        k = ro.shape[0]
        r = _lib.CRays()
        r.origins, r.dirs, r.n, r.first_ray = ro.data_ptr(), rd.data_ptr(), k, 0
        for outs, (p_rgba, p_depth, p_near) in (("rgba", (rgba, None, None)), ("rgba_depth_tnear", (rgba, depth, near)),
                                                ("depth_tnear", (None, depth, near))):
            out = _lib.CRaysOut()
            out.rgba = p_rgba.data_ptr() if p_rgba is not None else None
            out.depth = p_depth.data_ptr() if p_depth is not None else None
            out.t_near = p_near.data_ptr() if p_near is not None else None
            ms = timed(lambda: _lib.check(R.lib().rto_launch_rays_ex(dt._h, C.byref(r), C.byref(co), ctx._h, C.byref(out), stream)),
                       args.iters, args.reps)
            line("rays_%s_%s" % (name, outs), k, ms, "Grays/s", rays=k)

    layer_depth = torch.full((1, H, W), 1e9, dtype=torch.float32, device=dev)
    layer_color = torch.ones((1, H, W, 4), dtype=torch.float32, device=dev)
    for layered in (False, True) if "frames" in cases else ():
        for with_depth in (False, True):
            fctx = R.RenderContext(W, H)
            fctx.rng_seed()
            fctx.set_kernel(R.KERNEL_FAST)
            if layered:
                fctx.set_layers(layer_depth, layer_color)
            if with_depth:
                fctx.enable_depth()
            ms = timed(lambda: R.launch_renderer(dt, cam, opt, fctx, stream=stream.value or None), args.iters, args.reps)
            line("frame%s%s" % ("_layers" if layered else "", "_depth" if with_depth else ""), 1, ms, "frames/s")
    ratios = {}
    if "rays" in cases:
        ratios.update({"rays_raster": results["rays_raster_rgba_depth_tnear"] / results["rays_raster_rgba"],
                       "rays_random": results["rays_random_rgba_depth_tnear"] / results["rays_random_rgba"],
                       "rays_raster_depth_only": results["rays_raster_depth_tnear"] / results["rays_raster_rgba"]})
    if "frames" in cases:
        ratios.update({"frame": results["frame_depth"] / results["frame"], "frame_layers": results["frame_layers_depth"] / results["frame_layers"]})
    if ratios:
        print(json.dumps(dict(case="ratios_time_with_over_without", **{k: round(v, 4) for k, v in ratios.items()})), flush=True)
    if "batch" in cases:
        batch_case(dt, args, W, H, fx, opt, stream)


def batch_case(dt, args, W, H, fx, opt, stream):
    """(a) no depth, (b) mode 1, (c) mode 2: ms per launch of one batch of args.batch_frames frames, the three alternating"""
    import torch
    n = args.batch_frames
    cams = []
    for p in synth.orbit_poses(200)[:n]:
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    jumps = list(range(n))
    routes = {}
    for name, mode in (("a_no_depth", 0), ("b_mode_1", 1), ("c_mode_2", 2)):
        ctx = R.RenderContext(W, H, frames=n)
        ctx.rng_seed()
        if mode:
            ctx.enable_depth(batched=mode == 2)
        routes[name] = ctx

    def launch(ctx):
        R.launch_renderer_batch(dt, cams, opt, ctx, stream.value or None, rng_jumps=jumps)

    for ctx in routes.values():
        for _ in range(3):
            launch(ctx)
    torch.cuda.synchronize()
    assert routes["c_mode_2"].tile_marks() is not None and routes["b_mode_1"].tile_marks() is None  # (the routes are what they claim)
    ms = {name: [] for name in routes}
    for _ in range(7):
        for name, ctx in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                launch(ctx)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / 5)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for name, v in ms.items():
        print(json.dumps(dict(case="batch_" + name, frames=n, size=W, spp=args.spp, ms_per_launch_median=round(med[name], 4),
                              ms_per_launch_min=round(min(v), 4), ms_per_launch_max=round(max(v), 4),
                              frames_per_s=round(n / med[name] * 1e3, 1), repeats=[round(x, 4) for x in v])), flush=True)
    print(json.dumps(dict(case="batch_ratios", c_over_b=round(med["c_mode_2"] / med["b_mode_1"], 4),
                          c_over_a=round(med["c_mode_2"] / med["a_no_depth"], 4),
                          median_c_below_fastest_b=bool(med["c_mode_2"] < min(ms["b_mode_1"])))), flush=True)


if __name__ == "__main__":
    main()
