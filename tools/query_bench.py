"""Points/s of rto_tree_query on the C2 tree (GPU box).

16 M points, (a) uniform random in the tree's box and (b) a regular 256^3 grid over it in raster order, each sigma-only (the
occupancy path: the walk alone) and with `values` ([n][data_dim] floats stored through LDS).  Prints one JSON line per
measurement: the median of --reps timed runs of --iters back-to-back launches each (HIP events)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from basis_bench import sh_tree  # noqa: E402
from rays_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    t = sh_tree(args.depth, args.basis, args.shell, args.threads)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    dev = torch.device("cuda", 0)
    g = args.grid
    n = g ** 3
    lo, hi = (0 - t.offset) / t.scale, (1 - t.offset) / t.scale
    rng = np.random.default_rng(0)
    rand = torch.as_tensor(rng.uniform(lo, hi, (n, 3)).astype(np.float32), device=dev)
    ax = [np.linspace(lo[i], hi[i], g, endpoint=False, dtype=np.float64) + (hi[i] - lo[i]) / (2 * g) for i in range(3)]
    grid = torch.as_tensor(np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32), device=dev)
    sigma = torch.empty((n,), dtype=torch.float32, device=dev)
    values = torch.empty((n, dt.data_dim), dtype=torch.float32, device=dev)
    import ctypes as C
    from rt_octree_amd._lib import CQueryOut, check, lib
    for name, pts in (("random", rand), ("grid", grid)):
        for what in ("sigma", "values"):
            q = CQueryOut()
            q.sigma = sigma.data_ptr() if what == "sigma" else None
            q.values = values.data_ptr() if what == "values" else None
            s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ms = timed(lambda: check(lib().rto_tree_query(dt._h, C.c_void_p(pts.data_ptr()), n, C.byref(q), s)), args.iters, args.reps)
            print(json.dumps(dict(case="%s/%s" % (name, what), points=n, data_dim=dt.data_dim, ms=round(ms, 4),
                                  gpoints_per_s=round(n / ms * 1e3 / 1e9, 4))), flush=True)


if __name__ == "__main__":
    main()
