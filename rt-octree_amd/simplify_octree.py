"""Octree simplification: drop unreachable nodes, merge every node whose leaves all hold one record into its parent slot, and
renumber -- what svox's shrink_to_fit and the pruning of PlenOctree extraction do (include/rto.h "simplifier").  The output
stores the same field in fewer nodes; run it BEFORE compress_octree.

    python -m rt_octree_amd.simplify_octree x.npz [y.npz ...] [--sigma_thresh T] [--out_dir simplified] [--overwrite]
                                            [--backend hip|cpu]

The default is lossless: every point query of the output returns the bits the input returns.  --sigma_thresh T first kills the
leaves whose density is not above T (compared in fp16, as compress_octree compares): their record becomes zero, which lets
empty regions merge.  Per input: skipped when the output exists (without --overwrite); `child` and `data` are replaced;
parent_depth, n_free and n_internal describe the old numbering and are dropped if present; every other key passes through,
extra_data included.  A quantised file (quant_colors / quant_map) is refused: its codebook indices are per slot of the old
numbering -- simplify first, then compress.  Written with savez_compressed.  --backend cpu uses the host twin and never touches
a GPU; both backends write the same bytes."""
import argparse
import os
import os.path as osp
import sys

import numpy as np

STALE_KEYS = ("parent_depth", "n_free", "n_internal")
QUANT_KEYS = ("quant_colors", "quant_map", "data_retained", "sigma")


def simplify_arrays(z, sigma_thresh=None, backend="hip", simplifier=None):
    """z: the dict of a dense tree.npz -> (the dict of the simplified file, stats)"""
    from .simplify import simplify_tree
    z = dict(z)
    child = np.ascontiguousarray(z["child"], dtype=np.int32)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    if data.ndim != 5 or child.ndim != 4 or data.shape[:4] != child.shape:
        raise ValueError("child must be [capacity,N,N,N] and data [capacity,N,N,N,D], not %s and %s"
                         % (list(child.shape), list(data.shape)))
    c, d, _, stats = simplify_tree(child, data, sigma_thresh, backend=backend, simplifier=simplifier)
    for k in STALE_KEYS:
        z.pop(k, None)
    z["child"], z["data"] = c, d
    return z, stats


def simplify_file(src, dst, **kw):
    """One file -> stats.  ValueError for a quantised file or one without child / data."""
    with np.load(src) as f:
        if any(k in f.files for k in QUANT_KEYS[:2]):
            raise ValueError("the file is quantised (quant_colors / quant_map): simplify the dense tree first, then run compress_octree")
        if "child" not in f.files or "data" not in f.files:
            raise ValueError("no child / data arrays: not a dense tree.npz")
        z = {k: f[k] for k in f.files}
    out, stats = simplify_arrays(z, **kw)
    np.savez_compressed(dst, **out)
    return stats


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rt_octree_amd.simplify_octree", description=__doc__.split("\n\n")[0])
    parser.add_argument("input", type=str, nargs="+", help="Input npz(s)")
    parser.add_argument("--sigma_thresh", type=float, default=None, help="Kill leaves whose sigma is not above this (default: lossless)")
    parser.add_argument("--out_dir", type=str, default="simplified", help="Where to write the simplified npz")
    parser.add_argument("--overwrite", action="store_true", help="Overwrite an existing output")
    parser.add_argument("--backend", choices=("hip", "cpu"), default="hip", help="The HIP kernels or the host twin")
    args = parser.parse_args(argv)
    if args.sigma_thresh is not None and np.isnan(args.sigma_thresh):
        print("simplify_octree: --sigma_thresh must be a number", file=sys.stderr)
        return 2
    os.makedirs(args.out_dir, exist_ok=True)
    simplifier = None
    try:
        for fname in args.input:
            fname_s = osp.join(args.out_dir, osp.basename(fname))
            print("Simplifying", fname, "to", fname_s)
            if not args.overwrite and osp.exists(fname_s):
                print(" > skip")
                continue
            if args.backend == "hip" and simplifier is None:
                from .simplify import Simplifier
                simplifier = Simplifier(0)
            try:
                st = simplify_file(fname, fname_s, sigma_thresh=args.sigma_thresh, backend=args.backend, simplifier=simplifier)
            except ValueError as e:
                print("simplify_octree: %s: %s" % (fname, e), file=sys.stderr)
                return 2
            print(" > Nodes %d -> %d (%d unreachable, %d merged, %d leaves killed), %d levels"
                  % (st["capacity_in"], st["capacity"], st["unreachable"], st["merged"], st["killed"], st["levels"]))
            print(" > Size %.2f MB -> %.2f MB" % (osp.getsize(fname) / 2.0 ** 20, osp.getsize(fname_s) / 2.0 ** 20))
    finally:
        if simplifier is not None:
            simplifier.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
