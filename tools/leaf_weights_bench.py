"""What the per-leaf peak weights cost and what pruning by them buys (GPU box), on the C2 bench tree (the synthetic SH16 tree
bench.py builds: depth 10, shell 2.5) with --poses orbit cameras at --size x --size:

  cold / warm   rto_tree_leaf_weights over the first ten cameras into a zeroed array (most updates land) and over the last ten
                after all the others (most updates are skipped): ms per camera and M rays/s, the device synchronised around
                each group of ten; --runs runs, each from a zeroed array, the median
  render        beside them, rto_launch_renderer at SPP 1 (no denoise) of the same ten cameras in the same process
  prune         the tool's result at --weight_thresh: kill_unseen + simplify_tree(kill_thresh = 0), nodes and MB before / after, and the nodes
                simplify_tree(kill_thresh = 0) alone leaves (what the visibility kill adds to the merge)
  psnr          rto_metrics PSNR of the pruned against the unpruned tree's frames at SPP 32 over all poses (same RNG states:
                only the pruning differs), mean and minimum

Report only.  Output: profiles/leaf_weights_bench.txt (--out)."""
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
    ap.add_argument("--weight_thresh", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--psnr_spp", type=int, default=32, help="0 = skip the PSNR leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_weights_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    print("tree built in %.1f s: capacity %d" % (time.time() - t0, tree.capacity), file=sys.stderr)
    W = H = args.size
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(args.poses):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
    opt = R.RenderOptions()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    k = min(10, len(cams))
    R.leaf_weights(dt, cams[:1])  # warm-up: module load
    ctx = R.RenderContext(W, H)
    ropt = R.RenderOptions(spp=1, denoise=False)
    R.launch_renderer(dt, cams[0], ropt, ctx)  # warm-up
    w = torch.zeros((tree.capacity, 2, 2, 2), dtype=torch.float32, device="cuda:0")
    ms = {"cold": [], "middle": [], "warm": [], "render_first": [], "render_last": []}
    for _ in range(args.runs):  # every run starts from a zeroed array
        w.zero_()
        ms["cold"].append(timed(lambda: R.leaf_weights(dt, cams[:k], opt, out=w))[0])
        seen_cold = int((w > 0).sum())
        ms["middle"].append(timed(lambda: R.leaf_weights(dt, cams[k:len(cams) - k], opt, out=w))[0])
        before_warm = w.clone()
        ms["warm"].append(timed(lambda: R.leaf_weights(dt, cams[len(cams) - k:], opt, out=w))[0])
        raised_warm = int((w.view(torch.int32) != before_warm.view(torch.int32)).sum())
        del before_warm
        for name, group in (("render_first", cams[:k]), ("render_last", cams[len(cams) - k:])):
            def frames():
                for c in group:
                    R.launch_renderer(dt, c, ropt, ctx)
            ms[name].append(timed(frames)[0])
    med = {name: float(np.median(v)) for name, v in ms.items()}
    rays = k * W * H
    lines = ["# tools/leaf_weights_bench.py: tree depth %d, SH%d, shell %.1f, %d nodes; %d orbit cameras at %d x %d; device: %s"
             % (args.depth, args.basis, args.shell, tree.capacity, len(cams), W, H, torch.cuda.get_device_name(0)),
             "# wall ms around a synchronised group of %d cameras, median (min .. max) of %d runs, each from a zeroed array; options: the "
             "defaults (step_size 1e-4, sigma_thresh 1e-2, stop_thresh 1e-2)" % (k, args.runs)]

    def per(v, n):
        return dict(ms_per_camera=round(float(np.median(v)) / n, 4), min=round(min(v) / n, 4), max=round(max(v) / n, 4))

    lines.append(json.dumps(dict(leaf_weights="cold_first_%d" % k, **per(ms["cold"], k), mrays_per_s=round(rays / med["cold"] * 1e-3, 1),
                                 leaves_seen_after=seen_cold)))
    lines.append(json.dumps(dict(leaf_weights="warm_last_%d" % k, **per(ms["warm"], k), mrays_per_s=round(rays / med["warm"] * 1e-3, 1),
                                 words_raised=raised_warm)))
    lines.append(json.dumps(dict(leaf_weights="middle_%d" % (len(cams) - 2 * k), **per(ms["middle"], max(len(cams) - 2 * k, 1)))))
    for name in ("render_first", "render_last"):
        lines.append(json.dumps(dict(render_spp1=name[7:] + "_%d" % k, **per(ms[name], k), mrays_per_s=round(rays / med[name] * 1e-3, 1))))
    lines.append(json.dumps(dict(warm_over_render_spp1=round(med["warm"] / med["render_last"], 3),
                                 cold_over_render_spp1=round(med["cold"] / med["render_first"], 3))))
    # the tool's result
    wh = w.cpu().numpy()
    leaf = child == 0
    dense = leaf & (data[..., -1].astype(np.float32) > np.float32(opt.sigma_thresh))
    pruned = R.kill_unseen(child, data, wh, args.weight_thresh)
    t_s, (c1, d1, _, st) = timed(lambda: R.simplify_tree(child, pruned, 0.0, backend="hip"))
    st_plain = R.simplify_tree(child, data, 0.0, backend="hip")[3]  # the same merge step without the visibility kill
    lines.append(json.dumps(dict(prune_weight_thresh=args.weight_thresh, nodes=int(tree.capacity), nodes_after=int(st["capacity"]),
                                 nodes_after_simplify_alone=int(st_plain["capacity"]), dense_leaves=int(dense.sum()), seen=int((leaf & (wh > 0)).sum()),
                                 killed=int((pruned[..., -1].view(np.uint16) != data[..., -1].view(np.uint16)).sum()), merged=int(st["merged"]),
                                 mb=round((child.nbytes + data.nbytes) / 2.0 ** 20, 1), mb_after=round((c1.nbytes + d1.nbytes) / 2.0 ** 20, 1))))
    if args.psnr_spp > 0:
        dp = R.N3Tree.from_arrays(c1, d1, tree.scale, tree.offset, tree.data_format)
        m = R.ImageMetrics(0)
        popt = R.RenderOptions(spp=args.psnr_spp, denoise=False)
        psnr = []
        for i, c in enumerate(cams):
            imgs = []
            for t in (dt, dp):
                ctx.rng_seed()
                ctx.rng_advance(i << 32)
                R.launch_renderer(t, c, popt, ctx)
                imgs.append(torch.as_tensor(ctx.image_view(), device="cuda:0").clone())
            psnr.append(m.compute(imgs[1], imgs[0])[0].psnr)
        finite = [p for p in psnr if np.isfinite(p)]
        lines.append(json.dumps(dict(psnr_pruned_vs_unpruned_spp=args.psnr_spp, frames=len(psnr), identical_frames=len(psnr) - len(finite),
                                     mean_db=round(float(np.mean(finite)), 2) if finite else None,
                                     min_db=round(float(np.min(finite)), 2) if finite else None)))
        m.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
