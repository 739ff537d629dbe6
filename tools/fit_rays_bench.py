"""What the tree fit costs on rays the caller supplies (GPU box), beside the camera entry: the C2 bench tree (the synthetic SH16
tree bench.py builds: depth 10, shell 2.5), --poses orbit cameras at --size x --size, targets and perturbed params as
tools/fit_bench.py sets them up.  All rays of all cameras form one table (volrend.camera_rays: on them the ray entry gives the
camera entry's bytes), which is run in five orders:

  (a) cameras        rto_tree_fit_grad on the cameras -- the yardstick, measured in the same run
  (b) tile order     rto_tree_fit_grad_rays, the rays of each image in 8 x 8 tiles (a wave = the camera entry's wave)
  (c) raster order   the rays of each image row by row
  (d) shuffled       one permutation over all images
  (e) batch-sorted   the shuffled table in batches of --sort_batch rays, each batch sorted back into (image, tile) order before
                     its call; the sort and the gather are timed with it.  (d-batched) is the same loop without the sort.

forward = grad NULL, colours written; forward+backward = grad and stats.  M rays/s from the wall time around synchronised calls
over the whole table; --runs runs, the median.  Then: ms per call of one shuffled batch of R rays beside the full-array SGD
step, and (b) / (d) with workgroups of 128 and 256 threads instead of the library's 64 (RTO_FIT_RAYS_BLOCK).  Report only.
Output: profiles/fit_rays_bench.txt (--out)."""
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
    ap.add_argument("--sort_batch", type=int, default=1 << 22)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_rays_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()

    def say(msg):
        print("[%.1f s] %s" % (time.time() - t0, msg), file=sys.stderr, flush=True)

    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    say("tree built: capacity %d" % tree.capacity)
    W = H = args.size
    assert W % 8 == 0
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(args.poses):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
    fit = R.TreeFit(dt, data)
    del data
    dev = fit.params.device
    n_img, px = len(cams), W * H
    n = n_img * px

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    targets = fit.render(cams)  # (also the warm-up of the camera entry's forward kernel)
    images = [torch.empty_like(t) for t in targets]
    fit.params[..., :-1] *= 0.5
    fit.params[..., -1] *= 0.8
    # the table in raster order
    o = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d = torch.empty((n, 3), dtype=torch.float32, device=dev)
    for f, c in enumerate(cams):
        co, cd = R.camera_rays(c)
        o[f * px:(f + 1) * px] = torch.from_numpy(co).to(dev)
        d[f * px:(f + 1) * px] = torch.from_numpy(cd).to(dev)
    tg = torch.cat([t.reshape(-1, 3) for t in targets])
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    say("ray table on the device: %d rays, %.2f GB" % (n, n * 36 / 1e9))
    # raster index of the k-th ray in tile order, for one image and for all
    yy, xx = np.mgrid[0:H, 0:W]
    key = ((yy // 8) * (W // 8) + xx // 8) * 64 + (yy % 8) * 8 + xx % 8
    tile_of_image = torch.from_numpy(np.argsort(key.reshape(-1), kind="stable")).to(dev)
    tile_idx = (torch.arange(n_img, device=dev)[:, None] * px + tile_of_image[None, :]).reshape(-1)

    def forward(oo, dd):
        R.fit_grad_rays(dt, fit.params, oo, dd, None, out=out[:oo.shape[0]])

    def forward_backward(oo, dd, tt):
        fit.accumulate_rays(oo, dd, tt)

    # warm-up of both entries, the step and the loss
    fit.accumulate(cams[:1], targets[:1])
    forward(o[:px], d[:px])
    forward_backward(o[:px], d[:px], tg[:px])
    fit.step(0.0)
    fit.loss()
    say("warm-up done")
    ms = {}

    def measure(name, fwd, fb, runs=args.runs):
        ms[name] = {"forward": [], "forward_backward": []}
        for _ in range(runs):
            ms[name]["forward"].append(timed(fwd))
            ms[name]["forward_backward"].append(timed(fb))
            fit.step(0.0)  # (lr 0: clears grad; every run times the same field)
        loss, rays = fit.loss()
        assert rays == runs * n, (name, rays)
        say("%s: forward %.1f ms, forward+backward %.1f ms" % (name, np.median(ms[name]["forward"]), np.median(ms[name]["forward_backward"])))
        return loss

    loss_a = measure("a_cameras", lambda: R.fit_grad(dt, fit.params, cams, None, images=images), lambda: fit.accumulate(cams, targets))
    del images
    loss_c = measure("c_raster", lambda: forward(o, d), lambda: forward_backward(o, d, tg))
    assert loss_c == loss_a, "the ray entry's loss word differs from the camera entry's"
    # (b) the table in tile order -- from here on the table stays in tile order: a batch sorted by its indices is in (image, tile) order
    o, d, tg = o[tile_idx], d[tile_idx], tg[tile_idx]
    del tile_idx
    assert measure("b_tiles", lambda: forward(o, d), lambda: forward_backward(o, d, tg)) == loss_a
    for block in (128, 256):
        os.environ["RTO_FIT_RAYS_BLOCK"] = str(block)
        measure("b_tiles_block%d" % block, lambda: forward(o, d), lambda: forward_backward(o, d, tg), runs=3)
    os.environ.pop("RTO_FIT_RAYS_BLOCK")
    # (d) shuffled over all images
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).permutation(n)).to(dev)
    so, sd, st = o[perm], d[perm], tg[perm]
    assert measure("d_shuffled", lambda: forward(so, sd), lambda: forward_backward(so, sd, st)) == loss_a
    for block in (128, 256):
        os.environ["RTO_FIT_RAYS_BLOCK"] = str(block)
        measure("d_shuffled_block%d" % block, lambda: forward(so, sd), lambda: forward_backward(so, sd, st), runs=3)
    os.environ.pop("RTO_FIT_RAYS_BLOCK")
    # ms per call of one shuffled batch of R rays, beside the full-array step
    steps = []
    for r in (1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22):
        if r > n:
            continue
        v = []
        for k in range(args.runs):
            s = slice(k * r, (k + 1) * r) if (k + 1) * r <= n else slice(0, r)
            v.append(timed(lambda: forward_backward(so[s], sd[s], st[s])))
        steps.append((r, float(np.median(v))))
    step_ms = float(np.median([timed(lambda: fit.step(0.0)) for _ in range(args.runs)]))
    fit.loss()
    del so, sd, st
    # (d-batched) and (e): the epoch loop of a trainer over the tile-ordered table, batches of --sort_batch rays

    def epoch(sort, backward):
        for b in range(0, n, args.sort_batch):
            idx = perm[b:b + args.sort_batch]
            if sort:
                idx = torch.sort(idx)[0]
            if backward:
                forward_backward(o[idx], d[idx], tg[idx])
            else:
                forward(o[idx], d[idx])

    assert measure("d_batched", lambda: epoch(False, False), lambda: epoch(False, True)) == loss_a
    assert measure("e_batch_sorted", lambda: epoch(True, False), lambda: epoch(True, True)) == loss_a

    count = fit.params.numel()
    lines = ["# tools/fit_rays_bench.py: tree depth %d, SH%d, shell %.1f, %d nodes, %d parameters; %d orbit cameras at %d x %d = %d rays "
             "(table %.2f GB); device: %s" % (args.depth, args.basis, args.shell, tree.capacity, count, n_img, W, H, n, n * 36 / 1e9,
                                              torch.cuda.get_device_name(0)),
             "# wall ms around synchronised calls over all rays, median (min .. max) of %d runs (3 for the block variants); options: the "
             "defaults; targets: the unperturbed field's images, params perturbed (coefficients x 0.5, sigma x 0.8); every order gives "
             "the camera entry's loss word (asserted); workgroups of 64 threads unless named; batches of (d-batched) and (e): %d rays"
             % (args.runs, args.sort_batch)]
    for name, v in ms.items():
        row = {"order": name}
        for mode in ("forward", "forward_backward"):
            med = float(np.median(v[mode]))
            row[mode] = dict(ms=round(med, 2), min=round(min(v[mode]), 2), max=round(max(v[mode]), 2), mrays_per_s=round(n / med * 1e-3, 1),
                             over_a=round(med / float(np.median(ms["a_cameras"][mode])), 3))
        lines.append(json.dumps(row))
    lines.append(json.dumps(dict(ms_per_step="sgd_step", median=round(step_ms, 3))))
    for r, v in steps:
        lines.append(json.dumps(dict(shuffled_batch_rays=r, forward_backward_ms=round(v, 3), mrays_per_s=round(r / v * 1e-3, 1),
                                     step_share=round(step_ms / (step_ms + v), 3))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
