"""Octree optimisation against the training images -- the last step of PlenOctree extraction (PlenOctrees'
octree/optimization.py): the structure stays fixed, the leaf values descend the squared error of the deterministic composited
render (include/rto.h "tree fit") by SGD.

    python -m rt_octree_amd.optimize_octree tree.npz --poses transforms_train.json
        [--dataset blender|tt] [--scale S] [--lr L] [--epochs E] [--batch_imgs K] [--max_imgs N]
        [--val_poses transforms_val.json] [--stop_thresh 1e-2] [--sigma_thresh 1e-2] [--step_size 1e-4]
        [--background 1.0] [--out_dir optimized] [--overwrite] [--backend hip|cpu]
        [--refine_rounds R] [--refine_nodes K] [--refine_weight_thresh 0.01] [--refine_max_level L]
        [--batch_rays R] [--seed S]
        [--optimizer sgd|rmsprop|adam] [--sparse_step] [--beta1 0.9] [--beta2 0.999] [--eps 1e-8]

One SGD step per batch of K images, in file order (no shuffling: a run is reproducible), E epochs.  --lr is the rate of a mean
squared error: a step uses lr * 2 / (3 * rays of the batch) on the summed gradient.  Per epoch the PSNR of the training images
as they were rendered during the epoch (-10 log10(loss / (3 rays))) is printed, and with --val_poses that of the validation
images after it.  Poses are read as prune_octree reads them; the images are the PNGs the pose file names (blender: file_path +
".png" beside the json; tt: the sorted files of ../rgb), 8-bit RGB or RGBA, alpha composited over --background, and must have the
cameras' size (with --scale: the scaled size).  The output holds `data` rounded to float16 and every other key unchanged: the
schema simplify_octree writes.  Refused: --dataset llff, a quantised file, an SG / ASG tree.  Skipped when the output exists
(without --overwrite).  --backend cpu uses the host twin and never touches a GPU; both backends write the same bytes.

--refine_rounds R (default 0: the structure stays fixed) makes the fit coarse to fine: after the E epochs of each of the first R
rounds the leaves that the training cameras see with a weight of at least --refine_weight_thresh are split, heaviest first, at
most --refine_nodes of them (include/rto.h "refiner"), never below level --refine_max_level; the float32 state of the fit is
carried into the new leaves unrounded, and E more epochs follow: (R + 1) * E in all.  The node count is printed per round; the
output's `child` is the refined one (parent_depth, n_free and n_internal are dropped then, as simplify_octree drops them).

--batch_rays R (default 0: the image batches above, the bytes of before) takes the steps on shuffled ray batches across all
images instead (include/rto.h "tree fit", rto_tree_fit_grad_rays): one table of all rays of all training images -- its size is
printed before it is made; on the device for hip, on the host for cpu -- walked per epoch in a permutation drawn from numpy's
PCG64(--seed + epoch index), one SGD step per R rays at lr * 2 / (3 * rays of the batch).  Both backends see the same batches and
write the same bytes; --val_poses and --refine_rounds (whose leaf weights still come from the cameras) work as before.  Measured
on a tree of 2.1 M nodes: the full-array SGD step is 35 % of a step's time at R = 2^18, 14 % at 2^20 and 4 % at
2^22, and shuffling costs 5 % of the gradient's rate; batches are not re-sorted by image (that won back 2.4 %).

--sparse_step steps only the leaves the batch reached (include/rto.h "tree fit", rto_fit_step_sparse): the ray
kernel marks them in a bitmap, the bitmap becomes a list, the step runs over the listed rows.  With --optimizer sgd it writes the
bytes of the run without the flag.  --optimizer rmsprop|adam (which imply --sparse_step) keep their moments per leaf value and
update them only where a batch reached (the lazy rule of torch.optim.SparseAdam and of Plenoxels); --lr is then the rate per
parameter, the gradient of the mean squared error enters as grad_scale = 2 / (3 * rays of the batch), and --lr must be given:
the default of 1000 is a rate for SGD on a mean squared error, a thousand units per step for an optimiser whose step has the
size of lr.  Image batches go through the ray entry on the cameras' rays then (the same bytes).  A refinement round starts the
moments and the step count afresh."""
import argparse
import json
import os
import os.path as osp
import sys

import numpy as np

from .prune_octree import load_poses, make_cameras, scaled_size
from .simplify_octree import QUANT_KEYS


def image_paths(dataset, poses_path):
    """the PNG of every pose, in the order load_poses returns the poses"""
    if dataset == "blender":
        with open(poses_path) as f:
            j = json.load(f)
        root = osp.dirname(osp.abspath(poses_path))
        return [osp.normpath(osp.join(root, fr["file_path"] + ".png")) for fr in j["frames"]]
    rgb = osp.join(poses_path, "..", "rgb")
    return [osp.join(rgb, n) for n in sorted(os.listdir(rgb))]


def load_target(path, width, height, background):
    """-> float32 [H,W,3]: rgb * a + background * (1 - a), every value / 255 in float32"""
    from .metrics import read_png
    u8 = read_png(path)
    if u8.shape[:2] != (height, width):
        raise ValueError("'%s' is %d x %d, the cameras %d x %d" % (path, u8.shape[1], u8.shape[0], width, height))
    f = u8.astype(np.float32) / np.float32(255)
    a = f[..., 3:]
    return np.ascontiguousarray(f[..., :3] * a + np.float32(background) * (np.float32(1) - a), np.float32)


def load_views(dataset, poses_path, scale, max_imgs, background):
    """-> (cameras, targets) of a pose file"""
    if dataset not in ("blender", "tt"):
        load_poses(dataset, poses_path)  # (raises: llff and unknown types, in prune_octree's words)
    paths = image_paths(dataset, poses_path)
    if not paths:
        raise ValueError("no images for '%s'" % poses_path)
    from .metrics import read_png
    first = read_png(paths[0])
    s = np.float32(scale)
    # the cameras' size before --scale: that of the images, undone
    w0, h0 = (first.shape[1], first.shape[0]) if s == np.float32(1) else (int(round(first.shape[1] / float(s))), int(round(first.shape[0] / float(s))))
    trans, width, height, fx, fy = load_poses(dataset, poses_path, w0, h0)
    if len(trans) != len(paths):
        raise ValueError("%d poses and %d images" % (len(trans), len(paths)))
    width, height, fx, fy = scaled_size(width, height, fx, fy, scale)
    if max_imgs > 0:
        trans, paths = trans[:max_imgs], paths[:max_imgs]
    return make_cameras(trans, width, height, fx, fy), [load_target(p, width, height, background) for p in paths]


def psnr_of(loss, rays):
    return float("nan") if rays == 0 else (float("inf") if loss <= 0 else -10.0 * np.log10(loss / (3.0 * rays)))


def fit_kw_of(fit):
    """the optimiser keywords a fit was made with: what a refinement hands to the next one"""
    return {"optimizer": fit.optimizer, "sparse": fit.sparse, "beta1": fit.beta1, "beta2": fit.beta2, "eps": fit.eps}


def make_fit(z, options, backend, fit_kw=None):
    """z: the dict of a dense tree.npz -> (a TreeFit or HostTreeFit, to_device: targets -> what its accumulate takes).  fit_kw:
    the optimiser keywords of TreeFit (optimizer, sparse, beta1, beta2, eps)"""
    fit_kw = fit_kw or {}
    from .fit import HostTreeFit, TreeFit
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    if data.ndim != 5 or child.ndim != 4 or data.shape[:4] != child.shape:
        raise ValueError("child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s" % (list(child.shape), list(data.shape)))
    scale = np.asarray(z["invradius3"] if "invradius3" in z else np.full(3, z["invradius"]), np.float32).reshape(-1)[:3]
    offset = np.asarray(z["offset"], np.float32).reshape(-1)[:3]
    fmt = str(z["data_format"]) if "data_format" in z else ""
    if not (fmt == "RGBA" or (fmt.startswith("SH") and fmt[2:].isdigit())):
        raise ValueError("the fit takes RGBA and SH trees, not data_format '%s'" % fmt)
    if backend == "cpu":
        return HostTreeFit(child, data, scale, offset, fmt, options, threads=min(16, os.cpu_count() or 1), **fit_kw), lambda ts: ts
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    import torch
    from .volrend import N3Tree
    tree = N3Tree.from_arrays(child, data, scale, offset, fmt)
    fit = TreeFit(tree, data, options, **fit_kw)
    return fit, lambda ts: [torch.from_numpy(t).to(fit.params.device) for t in ts]


def refine_fit(fit, z, cams, options, backend, max_nodes=-1, weight_thresh=0.01, max_level=31, refiner=None):
    """One refinement between two rounds of epochs: the leaves of the fitted tree that the training cameras see with a weight of
    at least weight_thresh are split, heaviest first, at most max_nodes of them (negative: all).  z: the dict the fit was made
    from -> (the dict of the refined tree, the new fit, its to_device, the refiner's stats).  The new fit's params are the old
    float32 params gathered by slot_src: the fit's state does not pass through fp16.  The new fit is a new TreeFit with the old
    one's optimiser: its moments are zero and its step count restarts (they are not carried across a refinement)."""
    from .refine import keys_from_weights, refine_tree
    from .refine_octree import weight_thresh_key
    from .simplify_octree import STALE_KEYS
    from .visibility import leaf_weights, leaf_weights_host
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    halves = fit.data_half()
    D = halves.shape[-1]
    if backend == "cpu":
        w = leaf_weights_host(child, halves, fit.scale, fit.offset, cams, options, threads=fit.threads)
    else:
        from .volrend import N3Tree
        old = fit.tree
        seen = N3Tree.from_arrays(child, halves, np.asarray(old.scale, np.float32), np.asarray(old.offset, np.float32), str(z["data_format"]))
        try:
            w = leaf_weights(seen, cams, options).cpu().numpy()
        finally:
            seen.free()
    c, d, slot_src, stats = refine_tree(child, halves, keys_from_weights(w), weight_thresh_key(weight_thresh), max_nodes, max_level,
                                        backend=backend, refiner=refiner)
    z = dict(z)
    for k in STALE_KEYS:
        z.pop(k, None)
    z["child"], z["data"] = c, d
    new_fit, to_device = make_fit(z, options, backend, fit_kw_of(fit))
    if backend == "cpu":
        new_fit.params[...] = fit.params.reshape(-1, D)[slot_src.reshape(-1)].reshape(new_fit.params.shape)
    else:
        import torch
        idx = torch.from_numpy(slot_src.reshape(-1).astype(np.int64)).to(fit.params.device)
        new_fit.params.copy_(fit.params.reshape(-1, D)[idx].reshape(new_fit.params.shape))
        fit.tree.free()
    return z, new_fit, to_device, stats


class RayTable:
    """All rays of all training images for --batch_rays: origins, dirs (volrend.camera_rays: on them the ray entry is the camera
    entry bit for bit) and targets, float32 [n,3] each, image after image in raster order, masked rays (a NaN in the target)
    dropped.  The table lives where the fit does: torch tensors on `device`, numpy arrays on the host (device None).
    epochs: how many permutations have been drawn -- the epoch index of the seed, carried across refinement rounds."""

    def __init__(self, cams, targets, seed, device=None, say=print):
        from .volrend import camera_rays
        n = sum(int(c.width) * int(c.height) for c in cams)
        say("ray table: %d rays of %d images, %.1f MB on %s" % (n, len(cams), n * 36 / 2.0 ** 20, device if device is not None else "the host"))
        o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        at = 0
        for c in cams:
            k = int(c.width) * int(c.height)
            o[at:at + k], d[at:at + k] = camera_rays(c)
            at += k
        t = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in targets]) if n else np.empty((0, 3), np.float32)
        keep = ~np.isnan(t).any(1)
        if not keep.all():
            o, d, t = o[keep], d[keep], t[keep]
            say("ray table: %d masked rays dropped" % int((~keep).sum()))
        self.n, self.seed, self.epochs, self.device = int(t.shape[0]), int(seed), 0, device
        self.arrays = [np.ascontiguousarray(a) for a in (o, d, t)]
        if device is not None:
            import torch
            self.arrays = [torch.from_numpy(a).to(device) for a in self.arrays]

    def batches(self, batch_rays):
        """the batches of one epoch: (origins, dirs, targets) of batch_rays rays each (the last may be shorter), drawn by a
        permutation of numpy's PCG64 seeded with seed + epoch index on the host -- the same batches on both backends"""
        perm = np.random.Generator(np.random.PCG64(self.seed + self.epochs)).permutation(self.n)
        self.epochs += 1
        if self.device is not None:
            import torch
            perm = torch.from_numpy(perm).to(self.device)
        for b in range(0, self.n, batch_rays):
            idx = perm[b:b + batch_rays]
            yield tuple(a[idx] for a in self.arrays)


def optimize(fit, to_device, cams, targets, lr, epochs, batch_imgs, val=None, say=print, losses=None, batch_rays=0, table=None):
    """the SGD loop -> the PSNR per epoch (losses: a list that takes every epoch's (loss, rays)).  batch_rays > 0: the steps are
    taken on shuffled batches of that many rays of `table` (a RayTable) instead of on batches of images"""
    if batch_rays <= 0:
        targets = to_device(targets)
    val = None if val is None else (val[0], to_device(val[1]))
    k = max(1, int(batch_imgs))
    out = []
    adaptive = getattr(fit, "optimizer", "sgd") != "sgd"  # lr per parameter, the mean's 2 / (3 rays) as grad_scale; else folded into lr as before

    def step(rays):
        if adaptive:
            fit.step(lr, grad_scale=2.0 / (3.0 * rays))
        else:
            fit.step(lr * 2.0 / (3.0 * rays))

    for epoch in range(epochs):
        if batch_rays > 0:
            for o, d, t in table.batches(batch_rays):
                fit.accumulate_rays(o, d, t)
                step(int(o.shape[0]))  # (no ray of the table is masked: stats counts the batch)
        else:
            for b in range(0, len(cams), k):
                bc, bt = cams[b:b + k], targets[b:b + k]
                fit.accumulate(bc, bt)
                rays = sum(int(c.width) * int(c.height) for c in bc)
                step(rays)
        loss = fit.loss()
        if losses is not None:
            losses.append(loss)
        line = "epoch %d: train psnr %.4f" % (epoch, psnr_of(*loss))
        if val is not None:
            line += ", val psnr %.4f" % psnr_of(*fit.evaluate(*val))
        say(line)
        out.append(line)
    return out


def optimize_rounds(z, fit, to_device, cams, targets, options, backend, lr, epochs, batch_imgs, rounds, max_nodes=-1, weight_thresh=0.01,
                    max_level=31, val=None, say=print, losses=None, batch_rays=0, table=None):
    """Coarse to fine: `epochs` epochs, then -- after each of the first `rounds` rounds -- refine_fit and `epochs` more.
    -> (the dict of the tree the last round ran on, its fit).  rounds == 0 is optimize()."""
    refiner = None
    try:
        for rnd in range(rounds + 1):
            optimize(fit, to_device, cams, targets, lr, epochs, batch_imgs, val, say=say, losses=losses, batch_rays=batch_rays, table=table)
            if rnd == rounds:
                break
            if backend == "hip" and refiner is None:
                from .refine import Refiner
                refiner = Refiner(0)
            z, fit, to_device, st = refine_fit(fit, z, cams, options, backend, max_nodes, weight_thresh, max_level, refiner)
            say("round %d: nodes %d -> %d (%d candidates, %d selected), %d levels"
                % (rnd, st["capacity_in"], st["capacity"], st["candidates"], st["selected"], st["levels"]))
    finally:
        if refiner is not None:
            refiner.free()
    return z, fit


# what --sparse_step's help says about when it pays (profiles/fit_sparse_bench.txt)
SPARSE_HELP = ("Measured on a 2.1 M node tree: a batch's time falls to 0.36x at 2^14 rays, 0.49x at 2^16, 0.72x at 2^18 and 0.94x at 2^20; "
               "at 2^22 rays (half of all leaves touched) the two steps are within 1 %%: the sparse path stops winning there and never "
               "loses below.  Marking the leaves costs 1 %% of the gradient's time at 2^20 rays (0.24 ms, beside the 3.8 ms dense step)")


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rt_octree_amd.optimize_octree", description=__doc__.split("\n\n")[0])
    parser.add_argument("input", type=str, nargs="+", help="Input npz(s)")
    parser.add_argument("--poses", type=str, required=True, help="transforms_train.json (blender) or the pose directory (tt)")
    parser.add_argument("--dataset", type=str, default="blender", help="blender|tt")
    parser.add_argument("--scale", type=float, default=1.0, help="The images are this fraction of the dataset's size")
    parser.add_argument("--lr", type=float, default=None,
                        help="SGD rate on the mean squared error (default 1000); with --optimizer rmsprop|adam the rate per parameter, no default")
    parser.add_argument("--epochs", type=int, default=1)
    parser.add_argument("--batch_imgs", type=int, default=4, help="Images per SGD step")
    parser.add_argument("--batch_rays", type=int, default=0,
                        help="Rays per SGD step, shuffled over all images; 0 (default): steps on batches of --batch_imgs images.  "
                             "The full-array step is 14 %% of a step's time at 2^20 rays and 4 %% at 2^22 on a 2.1 M node tree")
    parser.add_argument("--seed", type=int, default=0, help="Seed of the shuffles of --batch_rays (epoch e draws from seed + e)")
    parser.add_argument("--optimizer", choices=("sgd", "rmsprop", "adam"), default="sgd",
                        help="sgd (default), or rmsprop / adam with lazily updated moments (they imply --sparse_step and need --lr)")
    parser.add_argument("--sparse_step", action="store_true",
                        help="Step only the leaves a batch reached; the same bytes as the dense step.  " + SPARSE_HELP)
    parser.add_argument("--beta1", type=float, default=0.9, help="adam: decay of the first moment")
    parser.add_argument("--beta2", type=float, default=0.999, help="rmsprop, adam: decay of the second moment")
    parser.add_argument("--eps", type=float, default=1e-8, help="rmsprop, adam: added to the root of the second moment")
    parser.add_argument("--max_imgs", type=int, default=0, help="Use the first N poses only")
    parser.add_argument("--val_poses", type=str, default="", help="Pose file of a validation set, scored after every epoch")
    parser.add_argument("--stop_thresh", type=float, default=1e-2)
    parser.add_argument("--sigma_thresh", type=float, default=1e-2)
    parser.add_argument("--step_size", type=float, default=1e-4)
    parser.add_argument("--background", type=float, default=1.0, help="background_brightness: behind the rays and the PNGs' alpha")
    parser.add_argument("--out_dir", type=str, default="optimized", help="Where to write the optimised npz")
    parser.add_argument("--overwrite", action="store_true", help="Overwrite an existing output")
    parser.add_argument("--backend", choices=("hip", "cpu"), default="hip", help="The HIP kernels or the host twins")
    parser.add_argument("--refine_rounds", type=int, default=0, help="Refine the tree after each of the first R rounds of --epochs epochs")
    parser.add_argument("--refine_nodes", type=int, default=-1, help="Nodes a refinement adds at most (default: no bound)")
    parser.add_argument("--refine_weight_thresh", type=float, default=0.01, help="A refinement splits leaves seen with at least this weight")
    parser.add_argument("--refine_max_level", type=int, default=31, help="A refinement never makes a node below this level")
    args = parser.parse_args(argv)
    if args.lr is None:
        if args.optimizer != "sgd":
            print("optimize_octree: --optimizer %s needs an explicit --lr: the default of 1000 is an SGD rate on a mean squared error, and a "
                  "step of rmsprop / adam has the size of lr itself (try 1e-2)" % args.optimizer, file=sys.stderr)
            return 2
        args.lr = 1000.0
    if not (0 <= args.beta1 < 1 and 0 <= args.beta2 < 1 and args.eps >= 0):
        print("optimize_octree: --beta1 and --beta2 must be in [0, 1), --eps >= 0", file=sys.stderr)
        return 2
    fit_kw = {"optimizer": args.optimizer, "sparse": args.sparse_step or args.optimizer != "sgd", "beta1": args.beta1, "beta2": args.beta2,
              "eps": args.eps}
    if not (args.lr >= 0 and args.epochs >= 0):
        print("optimize_octree: --lr and --epochs must be numbers >= 0", file=sys.stderr)
        return 2
    if args.batch_rays < 0 or args.seed < 0:
        print("optimize_octree: --batch_rays and --seed must be >= 0", file=sys.stderr)
        return 2
    if not (args.refine_rounds >= 0 and args.refine_weight_thresh >= 0 and 1 <= args.refine_max_level <= 31):
        print("optimize_octree: --refine_rounds and --refine_weight_thresh must be >= 0, --refine_max_level in 1 .. 31", file=sys.stderr)
        return 2
    from ._lib import RtoError
    from .volrend import RenderOptions
    try:
        cams, targets = load_views(args.dataset, args.poses, args.scale, args.max_imgs, args.background)
        val = load_views(args.dataset, args.val_poses, args.scale, 0, args.background) if args.val_poses else None
    except (ValueError, OSError, KeyError, RtoError) as e:
        print("optimize_octree: %s" % e, file=sys.stderr)
        return 2
    options = RenderOptions(step_size=args.step_size, sigma_thresh=args.sigma_thresh, stop_thresh=args.stop_thresh,
                            background_brightness=args.background)
    print("Images %d, %d x %d, fx %.9g fy %.9g" % (len(cams), cams[0].width, cams[0].height, cams[0].fx, cams[0].fy))
    os.makedirs(args.out_dir, exist_ok=True)
    table = None  # (--batch_rays: built with the first tree, on its device)
    say = lambda s: print(" > " + s)  # noqa: E731
    for fname in args.input:
        fname_s = osp.join(args.out_dir, osp.basename(fname))
        print("Optimizing", fname, "to", fname_s)
        if not args.overwrite and osp.exists(fname_s):
            print(" > skip")
            continue
        fit = None
        try:
            with np.load(fname) as f:
                if any(k in f.files for k in QUANT_KEYS[:2]):
                    raise ValueError("the file is quantised (quant_colors / quant_map): optimise the dense tree first, then run compress_octree")
                if "child" not in f.files or "data" not in f.files:
                    raise ValueError("no child / data arrays: not a dense tree.npz")
                z = {k: f[k] for k in f.files}
            fit, to_device = make_fit(z, options, args.backend, fit_kw)
            if args.batch_rays > 0:
                if table is None:
                    table = RayTable(cams, targets, args.seed, fit.params.device if args.backend == "hip" else None, say=say)
                table.epochs = 0
            if args.refine_rounds > 0:
                z, fit = optimize_rounds(z, fit, to_device, cams, targets, options, args.backend, args.lr, args.epochs, args.batch_imgs,
                                         args.refine_rounds, args.refine_nodes, args.refine_weight_thresh, args.refine_max_level, val,
                                         say=say, batch_rays=args.batch_rays, table=table)
            else:
                optimize(fit, to_device, cams, targets, args.lr, args.epochs, args.batch_imgs, val, say=say, batch_rays=args.batch_rays,
                         table=table)
            z["data"] = fit.data_half()
        except (ValueError, RtoError) as e:
            print("optimize_octree: %s: %s" % (fname, e), file=sys.stderr)
            return 2
        finally:
            if fit is not None and hasattr(fit, "tree"):
                fit.tree.free()
        np.savez_compressed(fname_s, **z)
        print(" > Size %.2f MB -> %.2f MB" % (osp.getsize(fname) / 2.0 ** 20, osp.getsize(fname_s) / 2.0 ** 20))
    return 0


if __name__ == "__main__":
    sys.exit(main())
