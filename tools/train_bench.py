"""Times one GuidanceNet training step -- forward + loss + backward, the optimiser apart -- on the two routes of the trainer
(rt-octree_amd/train.py --route): `torch` (the model under fp16 autocast, torch's SMAPE, GradScaler) and `fused` (the float32
HIP training kernels of csrc/guidance_train_kernels.hip + the device loss), alternating in ONE process.  Device events, both
routes warmed up, median of 7 windows with the spread; next to the times the floors the shapes give: multiply-adds of the
effective 3x3 kernels (forward, dW per layer, dX for every layer but the first) at the part's 157.3 TFLOP/s fp32 rate and the
bytes that must move at least once at 6.3 TB/s.

usage: python tools/train_bench.py [--steps 10] [--windows 7] [--out profiles/train_bench.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rt_octree_amd import denoiser  # noqa: E402

# (n, H, W, c1, levels, layers): blender.txt's chunks, tools/train_guidance.py's frames, the widest net at the chunk shape
CONFIGS = [(32, 80, 80, 32, 4, 2), (4, 800, 800, 32, 4, 2), (32, 80, 80, 64, 6, 3)]
PEAK_FP32, PEAK_HBM = 157.3e12, 6.3e12


def floors(n, H, W, c1, levels, layers):
    chans = [8] + [c1] * (layers - 1) + [2 * levels]
    macs = sum(9 * a * b for a, b in zip(chans[:-1], chans[1:]))
    back = 2 * macs - 9 * chans[0] * chans[1]  # dW for every layer, dX for all but the first
    flop = 2.0 * (macs + back) * n * H * W
    # aux + noisy + truth read once, every activation written by the forward and read by the backward, the image written
    byts = 4.0 * n * H * W * (8 + 4 + 4 + 4 + 2 * sum(chans[1:]))
    return flop, byts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_bench needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    lines = ["# %s; torch %s; one process, routes alternating; %d windows of %d steps, median [min .. max] ms per step"
             % (torch.cuda.get_device_name(0), torch.__version__, args.windows, args.steps)]

    def smape(p, t):
        return ((p - t).abs() / (p.abs() + t.abs() + 1e-5)).mean()

    for n, H, W, c1, levels, layers in CONFIGS:
        rs = np.random.RandomState(0)
        rgba = torch.tensor(rs.rand(n, 4, H, W).astype(np.float32), device=dev)
        aux = torch.cat([rgba, rgba * rgba], 1).contiguous()
        img = rgba.permute(0, 2, 3, 1).contiguous()
        tgt = torch.tensor(rs.rand(n, H, W, 4).astype(np.float32), device=dev)
        routes = {}
        for route in ("torch", "fused"):
            torch.manual_seed(0)
            model = denoiser.GuidanceNet(8, c1, 5, layers, levels).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-4)
            scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16) if route == "torch" else None
            routes[route] = (model, opt, scaler)

        def step(route):
            model, opt, scaler = routes[route]
            opt.zero_grad(set_to_none=True)
            if route == "torch":
                out = denoiser.filtering(model, aux, img, requires_grad=True)
                scaler.scale(smape(out[..., :3], tgt[..., :3])).backward()
            else:
                denoiser.image_loss(denoiser.filtering(model, aux, img, requires_grad=True, fused=True), tgt).backward()

        def optimise(route):
            model, opt, scaler = routes[route]
            if scaler is None:
                opt.step()
            else:
                scaler.step(opt)
                scaler.update()

        def window(fn, route):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn(route)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.steps

        for route in routes:  # warm-up of both: kernels loaded, scratch grown, MIOpen's choices made
            for _ in range(5):
                step(route)
                optimise(route)
        torch.cuda.synchronize()
        times = {(r, k): [] for r in routes for k in ("step", "opt")}
        for _ in range(args.windows):
            for route in routes:
                times[(route, "step")].append(window(step, route))
                times[(route, "opt")].append(window(optimise, route))
        flop, byts = floors(n, H, W, c1, levels, layers)
        lines.append("%d x %dx%d, net (%d, %d, %d): floors %.2f GFLOP = %.3f ms at 157.3 TFLOP/s, %.1f MB = %.3f ms at 6.3 TB/s"
                     % (n, H, W, c1, levels, layers, flop / 1e9, flop / PEAK_FP32 * 1e3, byts / 1e6, byts / PEAK_HBM * 1e3))
        med = {}
        for route in routes:
            for k in ("step", "opt"):
                t = sorted(times[(route, k)])
                med[(route, k)] = t[len(t) // 2]
                lines.append("    %-5s %-4s %8.3f  [%8.3f .. %8.3f]" % (route, k, med[(route, k)], t[0], t[-1]))
        lines.append("    fused / torch step time: %.3f" % (med[("fused", "step")] / med[("torch", "step")]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
