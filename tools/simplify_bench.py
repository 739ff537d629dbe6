"""What the tree simplifier costs and what it buys (GPU box), on the C2 bench tree (the synthetic SH16 tree bench.py builds:
depth 10, shell 2.5), lossless unless --sigma_thresh is given:

  hip_device  rto_tree_simplify with the tree already on the device and the result left there (the call drains its stream)
  hip         rt_octree_amd.simplify_tree(backend="hip"): numpy child / data in, numpy out
  host_twin   rto_tree_simplify_host, numpy in, numpy out

Wall time around each call with the device synchronised before and after; every route is warmed up once, then --runs runs in
which the routes take turns; the median per route.  hip_device is also given against the time its bytes take at the HBM rate
(--hbm_tbs): the tree read once plus the survivors written once.  Then the render stage of the C2 configuration (800 x 800,
SPP 6, batches of --batch frames along the orbit of bench.py, no denoise: the stage that walks the tree) on the original and on
the simplified tree, the two taking turns on the one card, frames/s per turn.  Report only.
Output: profiles/simplify_bench.txt (--out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import simplify, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--sigma_thresh", type=float, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--turns", type=int, default=5, help="turns of the frames/s comparison (0 = skip it)")
    ap.add_argument("--hbm_tbs", type=float, default=6.3, help="the HBM rate the device-resident time is held against, TB/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    print("tree built in %.1f s: capacity %d" % (time.time() - t0, tree.capacity), file=sys.stderr)
    s = R.Simplifier(0)
    dev_child, dev_data = torch.from_numpy(child).to("cuda:0"), torch.from_numpy(data).to("cuda:0")
    kill = args.sigma_thresh

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    routes = {"hip_device": lambda: s.simplify(dev_child, dev_data, kill, want_node_map=False),
              "hip": lambda: simplify.simplify_tree(child, data, kill, backend="hip", simplifier=s),
              "host_twin": lambda: simplify.simplify_tree_host(child, data, kill)}
    outs = {name: timed(fn)[1] for name, fn in routes.items()}  # warm-up, and the values
    ms = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, fn in routes.items():
            ms[name].append(timed(fn)[0])
    c1, d1, _, st = outs["hip"]
    host = outs["host_twin"]
    same = bool(np.array_equal(c1, host[0]) and np.array_equal(d1.view(np.uint16), host[1].view(np.uint16)) and st == host[3])
    med = {name: float(np.median(v)) for name, v in ms.items()}
    S = 8
    bytes_moved = (tree.capacity + st["capacity"]) * S * (4 + 2 * tree.data_dim)
    hbm_ms = bytes_moved / (args.hbm_tbs * 1e12) * 1e3
    lines = ["# tools/simplify_bench.py: tree depth %d, SH%d, shell %.1f; kill threshold %s" % (args.depth, args.basis, args.shell, kill),
             "# wall ms around a synchronised call; %d runs, the routes taking turns; device: %s" % (args.runs, torch.cuda.get_device_name(0)),
             json.dumps(dict(nodes=int(tree.capacity), slots=int(tree.capacity) * S, nodes_after=st["capacity"], slots_after=st["capacity"] * S,
                             merged=st["merged"], killed=st["killed"], unreachable=st["unreachable"], levels=st["levels"],
                             data_mb=round(data.nbytes / 2.0 ** 20, 1), data_mb_after=round(d1.nbytes / 2.0 ** 20, 1)))]
    for name, v in ms.items():
        lines.append(json.dumps(dict(route=name, ms_median=round(med[name], 3), min=round(min(v), 3), max=round(max(v), 3),
                                     runs=[round(x, 3) for x in v])))
    lines.append(json.dumps(dict(ratio_host_twin_over_hip=round(med["host_twin"] / med["hip"], 2), hip_equals_host_twin=same,
                                 bytes_read_once_plus_written_once=int(bytes_moved), ms_at_hbm_rate=round(hbm_ms, 3), hbm_tbs=args.hbm_tbs,
                                 hip_device_over_hbm_time=round(med["hip_device"] / hbm_ms, 2))))
    del dev_child, dev_data
    s.free()
    if args.turns > 0:
        W = H = args.size
        fx = synth.blender_focal(W)
        poses = synth.orbit_poses(200)
        cams = []
        for p in poses[:args.batch]:
            c = R.Camera(W, H, fx, fx)
            c.set_c2w(p)
            cams.append(c)
        opt = R.RenderOptions(spp=args.spp, denoise=False)
        trees = {"original": R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format),
                 "simplified": R.N3Tree.from_arrays(c1, d1, tree.scale, tree.offset, tree.data_format)}
        ctx = R.RenderContext(W, H, frames=len(cams))
        fps = {name: [] for name in trees}
        frames = {}
        for turn in range(args.turns + 1):  # turn 0 warms up
            for name, dt in trees.items():
                ctx.rng_seed()
                t, _ = timed(lambda: R.launch_renderer_batch(dt, cams, opt, ctx, rng_jumps=list(range(len(cams)))))
                if turn:
                    fps[name].append(len(cams) / (t * 1e-3))
                else:
                    ctx.select_frame(len(cams) // 2)
                    frames[name] = ctx.download_aux()
        for name, v in fps.items():
            lines.append(json.dumps(dict(render_stage=name, frames_per_s_median=round(float(np.median(v)), 1), min=round(min(v), 1),
                                         max=round(max(v), 1), turns=[round(x, 1) for x in v],
                                         device_bytes=int(trees[name].device_bytes), max_depth=int(trees[name].max_depth))))
        lines.append(json.dumps(dict(ratio_simplified_over_original=round(float(np.median(fps["simplified"]) / np.median(fps["original"])), 4),
                                     frames_bit_identical=bool(np.array_equal(frames["original"].view(np.uint32), frames["simplified"].view(np.uint32))),
                                     config="%dx%d SPP %d, %d frames per launch, render stage only" % (W, H, args.spp, len(cams)))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
