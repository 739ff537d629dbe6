"""What the sparse step of the tree fit costs and wins (GPU box), in the set-up of tools/fit_rays_bench.py: the C2 bench tree (the
synthetic SH16 tree bench.py builds: depth 10, shell 2.5), --poses orbit cameras at --size x --size, targets the unperturbed
field's images, params perturbed, all rays in one table shuffled by one permutation.  For a batch of R = 2^14, 2^16, 2^18, 2^20
and 2^22 rays (each of the --runs runs takes the next R rays of the table), ms around synchronised calls, the median:

  fb_old      forward + backward through rto_tree_fit_grad_rays
  fb_mark     the same through rto_tree_fit_grad_rays_touched (the lane reads the bitmap word, atomicOr only when the bit is clear)
  fb_noread   the marking entry with an unconditional atomicOr (RTO_FIT_MARK_NOREAD=1)
  list        rto_fit_touched_list with clear
  sgd / rmsprop / adam   rto_fit_step_sparse over the list
  dense       rto_fit_sgd_step over the whole array, in the same run
  touched     the number of listed leaves

and per R the whole batch both ways: fb_old + dense against fb_mark + list + sgd.  Report only.
Output: profiles/fit_sparse_bench.txt (--out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import fit as F  # noqa: E402
from rt_octree_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--poses", type=int, default=40, help="40 x 800 x 800 rays hold five distinct batches of 2^22")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_sparse_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()

    def say(msg):
        print("[%.1f s] %s" % (time.time() - t0, msg), file=sys.stderr, flush=True)

    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    say("tree built: capacity %d" % tree.capacity)
    W = H = args.size
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(args.poses):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
    fit = R.TreeFit(dt, data, optimizer="adam")  # (the bitmap, the list, the scratch, m and v: allocated once)
    del data
    dev = fit.params.device
    px = W * H
    n = len(cams) * px

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    targets = fit.render(cams)
    fit.params[..., :-1] *= 0.5
    fit.params[..., -1] *= 0.8
    o = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d = torch.empty((n, 3), dtype=torch.float32, device=dev)
    for f, c in enumerate(cams):
        co, cd = R.camera_rays(c)
        o[f * px:(f + 1) * px] = torch.from_numpy(co).to(dev)
        d[f * px:(f + 1) * px] = torch.from_numpy(cd).to(dev)
    tg = torch.cat([t.reshape(-1, 3) for t in targets])
    del targets
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).permutation(n)).to(dev)
    o, d, tg = o[perm], d[perm], tg[perm]
    del perm
    say("shuffled ray table on the device: %d rays, %.2f GB" % (n, n * 36 / 1e9))

    def fb_old(s):
        R.fit_grad_rays(dt, fit.params, o[s], d[s], tg[s], grad=fit.grad, stats=fit.stats)

    def fb_mark(s):
        R.fit_grad_rays(dt, fit.params, o[s], d[s], tg[s], grad=fit.grad, stats=fit.stats, touched=fit.touched)

    def the_list():
        F.touched_list(fit.touched, fit.slots, fit.list, fit.count, fit.scratch, clear=True)

    def step(kind, lr):
        opt = F.fit_optim(kind, lr, 1e-6, t=10)
        F.step_sparse(fit.params, fit.grad, fit.list, fit.count, opt, m=fit.m if kind == "adam" else None, v=fit.v if kind != "sgd" else None)

    def dense():
        F.sgd_step(fit.params, fit.grad, 0.0)

    # warm-up of every kernel (lr 0: params stay; every run times the same field)
    s0 = slice(0, 1 << 14)
    fb_old(s0)
    dense()
    for kind in ("sgd", "rmsprop", "adam"):
        fb_mark(s0)
        the_list()
        step(kind, 0.0)
    fit.loss()
    say("warm-up done")
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rows = []
    for r in (1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22):
        if r > n:
            continue
        batches = [slice(k * r, (k + 1) * r) if (k + 1) * r <= n else slice(0, r) for k in range(args.runs)]
        ms = {k: [] for k in ("fb_old", "dense", "fb_mark", "fb_noread", "list", "sgd", "rmsprop", "adam")}
        for s in batches:
            ms["fb_old"].append(timed(lambda: fb_old(s)))
            ms["dense"].append(timed(dense))
        touched = []
        for kind in ("sgd", "rmsprop", "adam"):
            for s in batches:
                ms["fb_mark"].append(timed(lambda: fb_mark(s)))
                ms["list"].append(timed(the_list))
                ms[kind].append(timed(lambda: step(kind, 0.0)))
                touched.append(int(fit.count.cpu()[0]))
        os.environ["RTO_FIT_MARK_NOREAD"] = "1"
        try:
            for s in batches:
                ms["fb_noread"].append(timed(lambda: fb_mark(s)))
                the_list()
                step("sgd", 0.0)
        finally:
            del os.environ["RTO_FIT_MARK_NOREAD"]
        assert not fit.grad.any() and not fit.touched.any()
        row = {"batch_rays": r, "touched_leaves": int(np.median(touched)), "touched_share": round(float(np.median(touched)) / fit.slots, 5)}
        row.update({k: med(v) for k, v in ms.items()})
        row["mark_over_old"] = round(row["fb_mark"] / row["fb_old"], 4)
        row["noread_over_old"] = round(row["fb_noread"] / row["fb_old"], 4)
        row["batch_dense_ms"] = round(row["fb_old"] + row["dense"], 3)
        row["batch_sparse_ms"] = round(row["fb_mark"] + row["list"] + row["sgd"], 3)
        row["sparse_over_dense"] = round(row["batch_sparse_ms"] / row["batch_dense_ms"], 4)
        rows.append(row)
        say(json.dumps(row))
    fit.loss()
    lines = ["# tools/fit_sparse_bench.py: tree depth %d, SH%d, shell %.1f, %d nodes, %d leaves and internal slots, %d parameters; %d orbit "
             "cameras at %d x %d = %d rays, shuffled (table %.2f GB); device: %s"
             % (args.depth, args.basis, args.shell, tree.capacity, fit.slots, fit.params.numel(), len(cams), W, H, n, n * 36 / 1e9,
                torch.cuda.get_device_name(0)),
             "# wall ms around synchronised calls, median of %d runs (fb_mark and list: of %d) in one process; every run takes the next "
             "batch of the table; lr 0, so every run times the same field; fb_*: forward + backward with stats; dense: rto_fit_sgd_step "
             "over all parameters; sgd / rmsprop / adam: rto_fit_step_sparse over the list; batch_dense = fb_old + dense, batch_sparse "
             "= fb_mark + list + sgd" % (args.runs, 3 * args.runs)]
    lines += [json.dumps(r) for r in rows]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
