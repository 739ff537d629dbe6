"""What the grid builder costs (GPU box).  The C2-style tree at depth 8 (synth.make_tree(depth_limit=8, basis_dim=9)) is sampled
to a 256^3 x 28 grid with tree_to_grid (0.94 GB) and built back:

  plan        rto_tree_build_plan with the grid on the device (reads the grid once; one synchronisation inside)
  write       rto_tree_build_write into buffers of the planned size
  copy        a device-to-device copy of the grid (Tensor.copy_: one hipMemcpyAsync) -- the yardstick: it reads and writes the
              grid where the plan reads it once, so half its time is the plan's floor
  hip         rt_octree_amd.build_tree(backend="hip"): numpy grid in, numpy child / data out
  host_twin   rto_tree_build_host, numpy in, numpy out (the counting call and the writing call)

Wall time around each call with the device synchronised before and after; every route is warmed up once, then --runs runs in
which the routes take turns; the median per route with the range.  The result is asserted to equal Simplifier.simplify of the
tree the grid was sampled from.  --big_depth 9 adds a 512^3 line (7.5 GB; plan, write and copy only).  Report only.
Output: profiles/grid_build_bench.txt (--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import grid_build, synth  # noqa: E402
from rt_octree_amd._lib import CGridBuildStats, check  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--basis", type=int, default=9)
    ap.add_argument("--big_depth", type=int, default=0, help="a second, larger grid for the device routes only (9 = 512^3), 0 = none")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_build_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grid_build_bench needs a HIP device")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def stat(v):
        return dict(ms_median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3), runs=[round(x, 3) for x in v])

    b = R.TreeBuilder(0)
    simp = R.Simplifier(0)
    lines = ["# tools/grid_build_bench.py: wall ms around a synchronised call; %d runs after one warm-up, the routes taking turns; device: %s"
             % (args.runs, torch.cuda.get_device_name(0))]
    for depth, with_host in ((args.depth, True),) + (((args.big_depth, False),) if args.big_depth else ()):
        t0 = time.time()
        tree = synth.make_tree(depth_limit=depth, basis_dim=args.basis, seed=20230418)
        child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
        dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
        grid = R.tree_to_grid(dt, depth)
        dt.free()
        torch.cuda.synchronize()
        print("depth %d: tree of %d nodes sampled in %.1f s" % (depth, tree.capacity, time.time() - t0), file=sys.stderr)
        D = grid.shape[-1]
        spare = torch.empty_like(grid)
        cap, st = C.c_int64(0), CGridBuildStats()
        nan = float("nan")

        def plan():
            check(R.lib().rto_tree_build_plan(b._h, None, C.c_void_p(grid.data_ptr()), depth, D, nan, C.byref(cap), C.byref(st)))
        plan()
        nodes = cap.value
        co = torch.empty((nodes, 2, 2, 2), dtype=torch.int32, device="cuda:0")
        do = torch.empty((nodes, 2, 2, 2, D), dtype=torch.float16, device="cuda:0")
        routes = {"plan": plan,
                  "write": lambda: check(R.lib().rto_tree_build_write(b._h, None, C.c_void_p(co.data_ptr()), C.c_void_p(do.data_ptr()))),
                  "copy": lambda: spare.copy_(grid)}
        if with_host:
            grid_np = grid.cpu().numpy()
            routes["hip"] = lambda: grid_build.build_tree(grid_np, None, backend="hip", builder=b)
            routes["host_twin"] = lambda: grid_build.build_tree_host(grid_np, None)
        outs = {name: timed(fn)[1] for name, fn in routes.items()}  # warm-up, and the values
        ms = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():
                if name == "write":
                    plan()  # (the hip route planned on its own grid in between)
                ms[name].append(timed(fn)[0])
        plan()
        routes["write"]()
        torch.cuda.synchronize()
        # the result is the simplified source tree
        sc, sd, _, sst = simp.simplify(torch.from_numpy(child).to("cuda:0"), torch.from_numpy(data).to("cuda:0"), None, want_node_map=False)
        same = bool(torch.equal(co, sc) and torch.equal(do.view(torch.int16), sd.view(torch.int16)))
        assert same and nodes == sc.shape[0], "the built tree differs from the simplified source tree"
        if with_host:
            hc, hd, hst = outs["host_twin"]
            gc, gd, gst = outs["hip"]
            twin = bool(np.array_equal(hc, gc) and np.array_equal(hd.view(np.uint16), gd.view(np.uint16)) and hst == gst)
            assert twin and np.array_equal(hc, co.cpu().numpy()), "the host twin differs from the kernels"
        med = {name: float(np.median(v)) for name, v in ms.items()}
        grid_bytes = grid.numel() * 2
        lines.append(json.dumps(dict(grid="%d^3 x %d" % (1 << depth, D), grid_gb=round(grid_bytes / 1e9, 3), source_nodes=int(tree.capacity),
                                     nodes=int(st.nodes), levels=int(st.levels), killed=int(st.killed),
                                     equals_simplified_source=same, scratch_mb=round(5 / 7 * (1 << (3 * depth)) / 2.0 ** 20, 1))))
        for name, v in ms.items():
            lines.append(json.dumps(dict(route=name, **stat(v))))
        summary = dict(plan_over_copy=round(med["plan"] / med["copy"], 2), copy_gb_per_s_read_plus_write=round(2 * grid_bytes / med["copy"] / 1e6, 1),
                       plan_gb_per_s_of_grid=round(grid_bytes / med["plan"] / 1e6, 1), write_over_copy=round(med["write"] / med["copy"], 3))
        if with_host:
            summary["ratio_host_twin_over_hip"] = round(med["host_twin"] / med["hip"], 2)
            summary["hip_equals_host_twin"] = twin
        lines.append(json.dumps(summary))
        del grid, spare, co, do, sc, sd
        torch.cuda.empty_cache()
    b.free()
    simp.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
