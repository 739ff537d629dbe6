"""Octree pruning by camera visibility -- the pruning step of PlenOctree extraction: march every pixel's ray of every training
view, record for every leaf the largest compositing weight T * (1 - exp(-sigma * delta)) any ray gives it (include/rto.h "leaf
weights"), and empty the leaves that stay under a threshold.  A dense leaf buried behind an opaque surface has weight 0: no
density threshold (simplify_octree --sigma_thresh) finds it.

    python -m rt_octree_amd.prune_octree tree.npz --poses transforms_train.json
        [--dataset blender|tt] [-w W -h H --fx --fy | --scale S]
        [--weight_thresh 0.01] [--stop_thresh 1e-2] [--sigma_thresh 1e-2] [--step_size 1e-4]
        [--max_imgs N] [--no_merge] [--save_weights w.npy]
        [--out_dir pruned] [--overwrite] [--backend hip|cpu]

The density of every leaf whose weight is < --weight_thresh becomes +0 (kill_unseen; with --weight_thresh 0: of every leaf no
ray reaches); then, unless --no_merge, simplify_tree(kill_thresh=0) zeroes the dead records, merges the nodes that became
uniform and renumbers.  That step also zeroes the leaves that already had sigma <= 0 (or NaN): they are invisible for any
sigma_thresh >= 0, so no image changes.  Skipped when the output exists (without --overwrite); `child` and `data` are replaced;
parent_depth, n_free and n_internal describe the old numbering and are dropped if present; every other key passes through.  A
quantised file (quant_colors / quant_map) is refused: prune the dense tree first, then run compress_octree.  Poses: blender
transforms_*.json or a TanksAndTemple pose directory (intrinsics.txt beside it), read with volrend_headless's conventions;
--dataset llff is refused (the API, leaf_weights on a tree with set_ndc, handles NDC trees).  --backend cpu uses the host twin
and never touches a GPU; both backends write the same bytes."""
import argparse
import json
import os
import os.path as osp
import sys

import numpy as np

from .simplify_octree import QUANT_KEYS, STALE_KEYS


def _tanf(x):
    """the C library's tanf, which volrend_headless calls (numpy's float32 tan may differ in the last bit)"""
    import ctypes
    try:
        f = ctypes.CDLL("libm.so.6").tanf
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
        return np.float32(f(float(x)))
    except (OSError, AttributeError):
        return np.float32(np.tan(np.float32(x)))


def _read_matrices(path):
    """whitespace-separated 4x4 (or 3x4) row-major matrices, several per file -> list of float32 [4,3] (row c = column c)"""
    with open(path) as f:
        tok = [np.float32(t) for t in f.read().split()]
    out, i = [], 0
    while len(tok) - i >= 4:
        if len(tok) - i < 12:
            raise ValueError("'%s': a matrix is cut short" % path)
        r = np.array(tok[i:i + 12], np.float32).reshape(3, 4)
        i += 12
        i += min(4, len(tok) - i)  # the fourth row of a 4x4
        out.append(np.ascontiguousarray(r.T))
    return out


def load_poses(dataset, poses_path, width=800, height=800, fx=-1.0, fy=-1.0):
    """-> (transforms: list of float32 [4,3], Camera.transform's layout; width, height, fx, fy), as volrend_headless reads them:
    blender: fx = fy = 0.5f * width / tanf(0.5f * camera_angle_x), the matrices transposed; tt: 1920 x 1080, fx / fy from
    ../intrinsics.txt, the files of the directory in sorted order, OpenCV convention (columns y and z negated)."""
    fx = np.float32(1111.11) if fx < 0 else np.float32(fx)
    fy = fx if fy < 0 else np.float32(fy)
    trans = []
    if dataset == "blender":
        with open(poses_path) as f:
            j = json.load(f)
        ang = np.float32(j["camera_angle_x"])
        fx = fy = np.float32(np.float32(0.5) * np.float32(width)) / _tanf(np.float32(0.5) * ang)
        for fr in j["frames"]:
            m = np.array(fr["transform_matrix"], np.float64)[:3, :4].astype(np.float32)
            trans.append(np.ascontiguousarray(m.T))
    elif dataset == "tt":
        width, height = 1920, 1080
        intr = osp.join(poses_path, "..", "intrinsics.txt")
        if not osp.exists(intr):
            raise ValueError("intrin '%s' does not exist" % intr)
        with open(intr) as f:
            tok = f.read().split()
        fx, fy = np.float32(tok[0]), np.float32(tok[5])
        for name in sorted(os.listdir(poses_path)):
            trans += _read_matrices(osp.join(poses_path, name))
        for t in trans:
            t[1] = -t[1]
            t[2] = -t[2]
    elif dataset == "llff":
        raise ValueError("--dataset llff: an NDC tree is pruned through the API (N3Tree.set_ndc + leaf_weights), not by this tool")
    else:
        raise ValueError("unknown dataset type '%s' (blender|tt)" % dataset)
    return trans, int(width), int(height), float(fx), float(fy)


def scaled_size(width, height, fx, fy, scale):
    """--scale as volrend_headless applies it"""
    s = np.float32(scale)
    if s == np.float32(1):
        return width, height, fx, fy
    w, h = int(np.float32(width) * s), int(np.float32(height) * s)
    return w, h, float(np.float32(fx) * (np.float32(w) / np.float32(width))), float(np.float32(fy) * (np.float32(h) / np.float32(height)))


def make_cameras(trans, width, height, fx, fy):
    from .volrend import Camera
    cams = []
    for t in trans:
        c = Camera(width, height, fx, fy)
        c.transform = np.ascontiguousarray(t, np.float32)
        cams.append(c)
    return cams


def pose_weights(z, cams, options, backend="hip"):
    """z: the dict of a dense tree.npz -> numpy float32 [capacity,N,N,N] weights over `cams`"""
    from .visibility import leaf_weights, leaf_weights_host
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    scale = np.asarray(z["invradius3"] if "invradius3" in z else np.full(3, z["invradius"]), np.float32).reshape(-1)[:3]
    offset = np.asarray(z["offset"], np.float32).reshape(-1)[:3]
    if backend == "cpu":
        return leaf_weights_host(child, data, scale, offset, cams, options, threads=min(16, os.cpu_count() or 1))
    if backend != "hip":
        raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
    from .volrend import N3Tree
    fmt = str(z["data_format"]) if "data_format" in z else ""
    tree = N3Tree.from_arrays(child, data, scale, offset, fmt, extra_data=z["extra_data"] if "extra_data" in z else None)
    try:
        return leaf_weights(tree, cams, options).cpu().numpy()
    finally:
        tree.free()


def prune_arrays(z, cams, options, weight_thresh=0.01, merge=True, backend="hip", simplifier=None):
    """z: the dict of a dense tree.npz -> (the dict of the pruned file, weights, stats)"""
    from .simplify import simplify_tree
    from .visibility import kill_unseen
    z = dict(z)
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    if data.ndim != 5 or child.ndim != 4 or data.shape[:4] != child.shape:
        raise ValueError("child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s"
                         % (list(child.shape), list(data.shape)))
    w = pose_weights(z, cams, options, backend)
    leaf = child == 0
    sig = data[..., -1].astype(np.float32)
    dense = leaf & (sig > np.float32(options.sigma_thresh))
    pruned = kill_unseen(child, data, w, weight_thresh)
    killed = int(np.count_nonzero(leaf & (pruned[..., -1].view(np.uint16) != data[..., -1].view(np.uint16))))
    stats = {"capacity_in": int(child.shape[0]), "capacity": int(child.shape[0]), "leaves": int(np.count_nonzero(leaf)),
             "dense": int(np.count_nonzero(dense)), "seen": int(np.count_nonzero(leaf & (w > 0))), "killed": killed, "merged": 0}
    if merge:
        child, pruned, _, st = simplify_tree(child, pruned, 0.0, backend=backend, simplifier=simplifier)
        stats["capacity"], stats["merged"] = st["capacity"], st["merged"]
        for k in STALE_KEYS:
            z.pop(k, None)
    z["child"], z["data"] = child, pruned
    return z, w, stats


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rt_octree_amd.prune_octree", description=__doc__.split("\n\n")[0], add_help=False)
    parser.add_argument("--help", action="help")
    parser.add_argument("input", type=str, nargs="+", help="Input npz(s)")
    parser.add_argument("--poses", type=str, required=True, help="transforms_*.json (blender) or the pose directory (tt)")
    parser.add_argument("--dataset", type=str, default="blender", help="blender|tt")
    parser.add_argument("-w", "--width", type=int, default=800)
    parser.add_argument("-h", "--height", type=int, default=800)
    parser.add_argument("--fx", type=float, default=-1.0)
    parser.add_argument("--fy", type=float, default=-1.0)
    parser.add_argument("--scale", type=float, default=1.0, help="Scale the images (and focal lengths) by this factor")
    parser.add_argument("--weight_thresh", type=float, default=0.01, help="Kill leaves whose peak weight is below this")
    parser.add_argument("--stop_thresh", type=float, default=1e-2)
    parser.add_argument("--sigma_thresh", type=float, default=1e-2)
    parser.add_argument("--step_size", type=float, default=1e-4)
    parser.add_argument("--max_imgs", type=int, default=0, help="Use the first N poses only")
    parser.add_argument("--no_merge", action="store_true", help="Only zero densities: child stays as it is")
    parser.add_argument("--save_weights", type=str, default="", help="Also write the weights [capacity,N,N,N] as .npy")
    parser.add_argument("--out_dir", type=str, default="pruned", help="Where to write the pruned npz")
    parser.add_argument("--overwrite", action="store_true", help="Overwrite an existing output")
    parser.add_argument("--backend", choices=("hip", "cpu"), default="hip", help="The HIP kernels or the host twins")
    args = parser.parse_args(argv)
    if not args.weight_thresh >= 0:
        print("prune_octree: --weight_thresh must be a number >= 0", file=sys.stderr)
        return 2
    from .volrend import RenderOptions
    try:
        trans, width, height, fx, fy = load_poses(args.dataset, args.poses, args.width, args.height, args.fx, args.fy)
    except (ValueError, OSError, KeyError) as e:
        print("prune_octree: %s" % e, file=sys.stderr)
        return 2
    if not trans:
        print("prune_octree: no camera poses", file=sys.stderr)
        return 2
    width, height, fx, fy = scaled_size(width, height, fx, fy, args.scale)
    if args.max_imgs > 0:
        trans = trans[:args.max_imgs]
    cams = make_cameras(trans, width, height, fx, fy)
    options = RenderOptions(step_size=args.step_size, sigma_thresh=args.sigma_thresh, stop_thresh=args.stop_thresh)
    print("Poses %d, %d x %d, fx %.9g fy %.9g" % (len(cams), width, height, fx, fy))
    os.makedirs(args.out_dir, exist_ok=True)
    simplifier = None
    try:
        for fname in args.input:
            fname_s = osp.join(args.out_dir, osp.basename(fname))
            print("Pruning", fname, "to", fname_s)
            if not args.overwrite and osp.exists(fname_s):
                print(" > skip")
                continue
            try:
                with np.load(fname) as f:
                    if any(k in f.files for k in QUANT_KEYS[:2]):
                        raise ValueError("the file is quantised (quant_colors / quant_map): prune the dense tree first, then run compress_octree")
                    if "child" not in f.files or "data" not in f.files:
                        raise ValueError("no child / data arrays: not a dense tree.npz")
                    z = {k: f[k] for k in f.files}
                if args.backend == "hip" and simplifier is None and not args.no_merge:
                    from .simplify import Simplifier
                    simplifier = Simplifier(0)
                out, w, st = prune_arrays(z, cams, options, args.weight_thresh, not args.no_merge, args.backend, simplifier)
            except ValueError as e:
                print("prune_octree: %s: %s" % (fname, e), file=sys.stderr)
                return 2
            np.savez_compressed(fname_s, **out)
            if args.save_weights:
                np.save(args.save_weights, w)
            print(" > Nodes %d -> %d (%d merged)" % (st["capacity_in"], st["capacity"], st["merged"]))
            print(" > Leaves %d, above sigma_thresh %d, seen %d, killed %d" % (st["leaves"], st["dense"], st["seen"], st["killed"]))
            print(" > Size %.2f MB -> %.2f MB" % (osp.getsize(fname) / 2.0 ** 20, osp.getsize(fname_s) / 2.0 ** 20))
    finally:
        if simplifier is not None:
            simplifier.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
