"""What the image metrics cost (GPU box): ms per 100 frames of 800 x 800 for ONE batched rto_metrics_compute_async call, RGBA32F
against RGBA32F, beside a torch restatement of the same formula (grouped conv2d, separable 11-tap window) in fp32 and in fp64.

Device events; every route is warmed up first; then --rounds rounds in which the routes take turns in this one process, each
timing a window of back-to-back calls; per route the median, minimum and maximum of the windows.  The file also records how
far the fp32 and fp64 torch values lie from the kernel's (the reason the kernel is float64), and the operation and byte
counts of the kernel computed from the shapes.  No threshold is set on any of it.  Output: profiles/metrics_bench.txt (--out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402


def torch_metrics(p, t, dtype, chunk):
    """[n,H,W,4] float32 x 2 -> [n,4] (mse, psnr, smape, ssim) in `dtype`, `chunk` frames at a time"""
    import torch
    import torch.nn.functional as F
    g = torch.exp(-((torch.arange(11, dtype=torch.float64, device=p.device) - 5.0) ** 2) / 4.5)
    g = (g / g.sum()).to(dtype)
    wh, ww = g.view(1, 1, 11, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, 11).repeat(3, 1, 1, 1)

    def G(x):
        return F.conv2d(F.conv2d(x, wh, groups=3), ww, groups=3)

    rows = []
    for k in range(0, p.shape[0], chunk):
        x = p[k:k + chunk, ..., :3].permute(0, 3, 1, 2).to(dtype)
        y = t[k:k + chunk, ..., :3].permute(0, 3, 1, 2).to(dtype)
        d = x - y
        mse = (d * d).mean(dim=(1, 2, 3))
        smape = (d.abs() / (x.abs() + y.abs() + 1e-5)).mean(dim=(1, 2, 3))
        mx, my = G(x), G(y)
        vxx, vyy, vxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
        m = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * ((2 * vxy + 9e-4) / (vxx + vyy + 9e-4))
        rows.append(torch.stack([mse, -10 * torch.log10(mse), smape, m.mean(dim=(1, 2, 3))], 1))
    return torch.cat(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="back-to-back calls per timed window of the kernel route")
    ap.add_argument("--chunk", type=int, default=10, help="frames per step of the torch routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n, H, W = args.frames, args.size, args.size
    gen = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand((n, H, W, 4), device=dev, generator=gen)
    truth = (pred + 0.05 * torch.randn((n, H, W, 4), device=dev, generator=gen)).clamp_(0, 1)
    met = R.ImageMetrics(0)
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    routes = {
        "hip_float64": (lambda: met.compute_async(pred, truth, out=out), args.calls),
        "torch_fp32": (lambda: torch_metrics(pred, truth, torch.float32, args.chunk), 1),
        "torch_fp64": (lambda: torch_metrics(pred, truth, torch.float64, args.chunk), 1),
    }
    values = {}
    for name, (fn, _) in routes.items():  # warm-up (allocator, kernel selection, the handle's scratch), and the values
        for _ in range(2):
            v = fn()
        torch.cuda.synchronize()
        values[name] = v.double().cpu().numpy().copy()
    ms = {name: [] for name in routes}
    for _ in range(args.rounds):
        for name, (fn, calls) in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / calls * (100.0 / n))
    lines = ["# tools/metrics_bench.py: ms per 100 frames of %d x %d, one batched call of %d frames, RGBA32F against RGBA32F" % (W, H, n),
             "# device events; %d rounds, the routes taking turns in one process; window = %d calls (hip) / 1 call (torch, %d frames a step)"
             % (args.rounds, args.calls, args.chunk), "# device: %s" % torch.cuda.get_device_name(0)]
    for name, v in ms.items():
        lines.append(json.dumps(dict(route=name, ms_per_100_frames_median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4),
                                     spread_pct=round(100.0 * (max(v) - min(v)) / float(np.median(v)), 2), windows=[round(x, 4) for x in v])))
    ref = values["hip_float64"]
    for name in ("torch_fp32", "torch_fp64"):
        dv = np.abs(values[name] - ref)
        lines.append(json.dumps(dict(route=name, max_abs_diff_from_hip=dict(mse=float(dv[:, 0].max()), psnr_db=float(dv[:, 1].max()),
                                                                             smape=float(dv[:, 2].max()), ssim=float(dv[:, 3].max())))))
    # the kernel's work, from the shapes: tiles of 32 x 16 with a 42 x 26 staged region
    tiles = -(-W // 32) * -(-H // 16) * n
    map_tiles = -(-(W - 10) // 32) * -(-(H - 10) // 16) * n
    flops = map_tiles * 3 * (16 * 42 * 11 * 13 + 32 * 16 * (11 * 10 + 14)) + tiles * 32 * 16 * 3 * 8
    lds_bytes = map_tiles * 3 * (16 * 42 * 11 * 2 * 4 + 16 * 42 * 5 * 8 + 32 * 16 * 11 * 5 * 8) + tiles * 42 * 26 * 6 * 4
    hbm_bytes = tiles * 42 * 26 * 2 * 16
    med = float(np.median(ms["hip_float64"])) * n / 100.0
    lines.append(json.dumps(dict(kernel_work=dict(workgroups=tiles, fp64_flops=flops, lds_bytes=lds_bytes, global_bytes_requested=hbm_bytes,
                                                  image_bytes=2 * n * H * W * 16, fp64_gflops_per_s=round(flops / med / 1e6, 1),
                                                  lds_gb_per_s=round(lds_bytes / med / 1e6, 1), image_gb_per_s=round(2 * n * H * W * 16 / med / 1e6, 1)))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
