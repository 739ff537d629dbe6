"""What the tree fit costs (GPU box), on the C2 bench tree (the synthetic SH16 tree bench.py builds: depth 10, shell 2.5) with
--poses orbit cameras at --size x --size.  The targets are the composited images of the tree's own values; the fitted params
start perturbed (coefficients x 0.5, sigma x 0.8), so every ray carries a residual and every dense sample its atomics.

  forward       rto_tree_fit_grad with grad == NULL (images written): ms per camera
  forward+back  rto_tree_fit_grad with grad and stats: ms per camera
  step          rto_fit_sgd_step over the whole array: ms, and GB/s of params + grad read and written
  leaf_weights  beside them, rto_tree_leaf_weights over the same cameras in the same process: the bare walk

Wall ms around a synchronised call over all cameras; --runs runs, the median with the range.  Report only.
Output: profiles/fit_bench.txt (--out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    print("tree built in %.1f s: capacity %d" % (time.time() - t0, tree.capacity), file=sys.stderr, flush=True)
    W = H = args.size
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(args.poses):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
    fit = R.TreeFit(dt, data)
    del data
    n = len(cams)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    targets = fit.render(cams)  # (also the warm-up of the forward kernel)
    images = [torch.empty_like(t) for t in targets]
    fit.params[..., :-1] *= 0.5
    fit.params[..., -1] *= 0.8
    w = torch.zeros((tree.capacity, 2, 2, 2), dtype=torch.float32, device="cuda:0")
    R.leaf_weights(dt, cams, out=w)  # warm-up; the timed calls then mostly skip their updates, the bare walk
    fit.accumulate(cams[:1], targets[:1])  # warm-up
    fit.step(0.0)
    fit.loss()
    print("warm-up done at %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
    ms = {"forward": [], "forward_backward": [], "step": [], "leaf_weights": []}
    touched = 0
    for _ in range(args.runs):
        ms["forward"].append(timed(lambda: R.fit_grad(dt, fit.params, cams, None, images=images)))
        ms["forward_backward"].append(timed(lambda: fit.accumulate(cams, targets)))
        touched = int((fit.grad != 0).sum())
        loss, rays = fit.loss()
        ms["step"].append(timed(lambda: fit.step(0.0)))  # (lr 0: every run times the same field)
        ms["leaf_weights"].append(timed(lambda: R.leaf_weights(dt, cams, out=w)))
    count = fit.params.numel()
    lines = ["# tools/fit_bench.py: tree depth %d, SH%d, shell %.1f, %d nodes, %d parameters (params %.2f GB, grad %.2f GB); %d orbit cameras at "
             "%d x %d; device: %s" % (args.depth, args.basis, args.shell, tree.capacity, count, count * 4 / 1e9, count * 8 / 1e9, n, W, H,
                                      torch.cuda.get_device_name(0)),
             "# wall ms around one synchronised call over all cameras, median (min .. max) of %d runs; options: the defaults; targets: the "
             "unperturbed field's images, params perturbed (coefficients x 0.5, sigma x 0.8)" % args.runs]

    def per(v, k):
        return dict(median=round(float(np.median(v)) / k, 4), min=round(min(v) / k, 4), max=round(max(v) / k, 4))

    for name in ("forward", "forward_backward", "leaf_weights"):
        lines.append(json.dumps(dict(ms_per_camera=name, **per(ms[name], n),
                                     mrays_per_s=round(n * W * H / float(np.median(ms[name])) * 1e-3, 1))))
    step_med = float(np.median(ms["step"]))
    lines.append(json.dumps(dict(ms_per_step="sgd_step", **per(ms["step"], 1), gb_per_s=round(count * 24 / step_med * 1e-6, 1))))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append(json.dumps(dict(forward_over_leaf_weights=round(med["forward"] / med["leaf_weights"], 2),
                                 forward_backward_over_forward=round(med["forward_backward"] / med["forward"], 2),
                                 grad_words_touched=touched, psnr_db=round(-10 * np.log10(loss / (3.0 * rays)), 2), rays=rays)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
