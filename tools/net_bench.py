"""Development harness: the fused GuidanceNet kernel alone (the bench's route: squares implied, packed fp16 maps) and
the factorised filter behind it, ms per 50-frame batch at 800x800.
--shapes: the general kernel (guidance_general.inc) per network shape against torch's compact.half(), which is what such a
net cost before it ran fused: same process, alternating, warm-up, median of 7 repetitions of 5 launches each."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rt_octree_amd import denoiser  # noqa: E402


SHAPES = [(8, 6, 2), (16, 3, 2), (64, 1, 2), (32, 4, 3), (64, 6, 3), (20, 2, 3), (8, 5, 3), (8, 4, 2), (16, 4, 2), (32, 6, 2), (64, 4, 2)]


def shapes():
    n, H, W, reps, inner = 50, 800, 800, 7, 5
    aux = torch.rand(n, 8, H, W, device="cuda:0")
    aux[:, 4:] = aux[:, :4] * aux[:, :4]
    print("ms per %d frames at %dx%d, median of %d repetitions (min .. max); fp32 planes, all 8 aux planes read" % (n, W, H, reps))
    for c1, levels, layers in SHAPES:
        torch.manual_seed(0)
        compact = denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, c1, 5, layers, levels)).eval()
        fused = denoiser.FusedGuidanceNet(compact, device=0)
        half = copy.deepcopy(compact).half().cuda()

        def run_torch():
            with torch.no_grad():
                return half(aux)
        times = {"fused": [], "torch": []}
        for f in (lambda: fused(aux), run_torch):  # warm-up (MIOpen picks its algorithm here)
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        for _ in range(reps):
            for name, f in (("fused", lambda: fused(aux)), ("torch", run_torch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / inner)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print("c1 %2d levels %d layers %d: general kernel %7.3f (%.3f .. %.3f)   torch compact.half() %7.3f (%.3f .. %.3f)   x%.1f"
              % (c1, levels, layers, med["fused"], min(times["fused"]), max(times["fused"]), med["torch"], min(times["torch"]),
                 max(times["torch"]), med["torch"] / med["fused"]), flush=True)


def main():
    if "--shapes" in sys.argv[1:]:
        return shapes()
    n, H, W = 50, 800, 800
    torch.manual_seed(0)
    full = denoiser.GuidanceNet(8, 32, 5, 2, 4)
    net = denoiser.FusedGuidanceNet(denoiser.GuidanceNetCompact.from_full(full).eval(), device=0)
    aux = torch.rand(n, 8, H, W, device="cuda:0")
    aux[:, 4:] = aux[:, :4] * aux[:, :4]
    img = torch.rand(n, H, W, 4, device="cuda:0")
    out = torch.empty_like(img)
    for rep in range(3):
        net(aux)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            w, g = net(aux)
        e1.record()
        torch.cuda.synchronize()
        print("guidance_fused (fp32 planes): %.3f ms per %d frames" % (e0.elapsed_time(e1) / 20, n), flush=True)
        e0.record()
        for _ in range(20):
            net.forward_packed(aux, squares_implied=True)
        e1.record()
        torch.cuda.synchronize()
        t_net = e0.elapsed_time(e1) / 20
        e0.record()
        for _ in range(20):
            net.filter_packed(img, out)
        e1.record()
        torch.cuda.synchronize()
        print("guidance_fused (packed, squares implied): %.3f ms   filter_fast (packed): %.3f ms per %d frames"
              % (t_net, e0.elapsed_time(e1) / 20, n), flush=True)
    print("checksum %.6f %.6f %.6f" % (float(w.double().sum()), float(g.double().sum()), float(out.double().sum())))


if __name__ == "__main__":
    main()
