"""Octree refinement: split the most important leaves into nodes of N^3 leaves that hold the leaf's record -- what svox's
N3Tree.refine(sel=...) does, and what PlenOctree extraction does where the weights are high (include/rto.h "refiner").  The output
stores the same field in more nodes: every point query returns the bits the input returns, and simplify_octree undoes it.

    python -m rt_octree_amd.refine_octree tree.npz [y.npz ...] [--weights w.npy] [--weight_thresh 0.01] [--sigma_thresh T]
                                          [--max_nodes K] [--max_level L] [--out_dir refined] [--overwrite] [--backend hip|cpu]

With --weights (the [capacity,N,N,N] float32 file prune_octree --save_weights writes) the leaves are taken by weight, largest
first: the key of a leaf is the bit pattern of its weight, 0 where --sigma_thresh is given and the density is not above it, and
a leaf is a candidate when its weight is at least --weight_thresh.  Without --weights the densest leaves go first: the key is the
float32 bit pattern of the density, 0 where the density is NaN or not above --sigma_thresh (default 0).  --max_nodes K splits the
first K candidates only (ties go to the lower slot index); --max_level L never makes a node below level L (default 31).  New nodes
are appended.  Per input: skipped when the output exists (without --overwrite); `child` and `data` are replaced; parent_depth,
n_free and n_internal describe the old tree and are dropped if present; every other key passes through, extra_data included: the
schema simplify_octree writes.  A quantised file (quant_colors / quant_map) is refused.  Written with savez_compressed.
--backend cpu uses the host twin and never touches a GPU; both backends write the same bytes."""
import argparse
import os
import os.path as osp
import sys

import numpy as np

from .simplify_octree import QUANT_KEYS, STALE_KEYS


def weight_thresh_key(weight_thresh):
    """key_thresh of a weight threshold: the bits of float32(weight_thresh), at least 1 (a weight of 0 is never a candidate)"""
    return max(1, int(np.array(max(float(weight_thresh), 0.0), np.float32).view(np.uint32)))


def keys_for(data, weights=None, weight_thresh=0.01, sigma_thresh=None):
    """(key uint32 [capacity,N,N,N], key_thresh) as the command builds them"""
    from .refine import keys_from_density, keys_from_weights
    if weights is None:
        return keys_from_density(data, 0.0 if sigma_thresh is None else sigma_thresh), 1
    weights = np.ascontiguousarray(weights, np.float32)
    if weights.shape != data.shape[:4]:
        raise ValueError("the weights are %s, the tree's slots %s" % (list(weights.shape), list(data.shape[:4])))
    key = keys_from_weights(weights)
    if sigma_thresh is not None:
        key = np.where(keys_from_density(data, sigma_thresh) != 0, key, np.uint32(0))
    return np.ascontiguousarray(key, np.uint32), weight_thresh_key(weight_thresh)


def refine_arrays(z, weights=None, weight_thresh=0.01, sigma_thresh=None, max_nodes=-1, max_level=31, backend="hip", refiner=None):
    """z: the dict of a dense tree.npz -> (the dict of the refined file, stats)"""
    from .refine import refine_tree
    z = dict(z)
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    if data.ndim != 5 or child.ndim != 4 or data.shape[:4] != child.shape:
        raise ValueError("child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s"
                         % (list(child.shape), list(data.shape)))
    key, key_thresh = keys_for(data, weights, weight_thresh, sigma_thresh)
    c, d, _, stats = refine_tree(child, data, key, key_thresh, max_nodes, max_level, backend=backend, refiner=refiner)
    for k in STALE_KEYS:
        z.pop(k, None)
    z["child"], z["data"] = c, d
    return z, stats


def refine_file(src, dst, **kw):
    """One file -> stats.  ValueError for a quantised file or one without child / data."""
    with np.load(src) as f:
        if any(k in f.files for k in QUANT_KEYS[:2]):
            raise ValueError("the file is quantised (quant_colors / quant_map): refine the dense tree first, then run compress_octree")
        if "child" not in f.files or "data" not in f.files:
            raise ValueError("no child / data arrays: not a dense tree.npz")
        z = {k: f[k] for k in f.files}
    out, stats = refine_arrays(z, **kw)
    np.savez_compressed(dst, **out)
    return stats


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rt_octree_amd.refine_octree", description=__doc__.split("\n\n")[0])
    parser.add_argument("input", type=str, nargs="+", help="Input npz(s)")
    parser.add_argument("--weights", type=str, default="", help="Leaf weights [capacity,N,N,N] float32 (prune_octree --save_weights)")
    parser.add_argument("--weight_thresh", type=float, default=0.01, help="With --weights: split leaves whose weight is at least this")
    parser.add_argument("--sigma_thresh", type=float, default=None, help="Never split leaves whose sigma is not above this")
    parser.add_argument("--max_nodes", type=int, default=-1, help="Add at most this many nodes (default: no bound)")
    parser.add_argument("--max_level", type=int, default=31, help="Never make a node below this level (1 .. 31)")
    parser.add_argument("--out_dir", type=str, default="refined", help="Where to write the refined npz")
    parser.add_argument("--overwrite", action="store_true", help="Overwrite an existing output")
    parser.add_argument("--backend", choices=("hip", "cpu"), default="hip", help="The HIP kernels or the host twin")
    args = parser.parse_args(argv)
    if (args.sigma_thresh is not None and np.isnan(args.sigma_thresh)) or np.isnan(args.weight_thresh):
        print("refine_octree: --sigma_thresh and --weight_thresh must be numbers", file=sys.stderr)
        return 2
    if args.weights and len(args.input) != 1:
        print("refine_octree: --weights belongs to one tree: give one input", file=sys.stderr)
        return 2
    from ._lib import RtoError
    os.makedirs(args.out_dir, exist_ok=True)
    refiner = None
    try:
        for fname in args.input:
            fname_s = osp.join(args.out_dir, osp.basename(fname))
            print("Refining", fname, "to", fname_s)
            if not args.overwrite and osp.exists(fname_s):
                print(" > skip")
                continue
            if args.backend == "hip" and refiner is None:
                from .refine import Refiner
                refiner = Refiner(0)
            try:
                weights = np.load(args.weights) if args.weights else None
                st = refine_file(fname, fname_s, weights=weights, weight_thresh=args.weight_thresh, sigma_thresh=args.sigma_thresh,
                                 max_nodes=args.max_nodes, max_level=args.max_level, backend=args.backend, refiner=refiner)
            except (ValueError, OSError, RtoError) as e:
                print("refine_octree: %s: %s" % (fname, e), file=sys.stderr)
                return 2
            print(" > Nodes %d -> %d (%d candidates, %d selected), %d levels"
                  % (st["capacity_in"], st["capacity"], st["candidates"], st["selected"], st["levels"]))
            print(" > Size %.2f MB -> %.2f MB" % (osp.getsize(fname) / 2.0 ** 20, osp.getsize(fname_s) / 2.0 ** 20))
    finally:
        if refiner is not None:
            refiner.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
