"""What the tree refiner costs (GPU box), on the C2 bench tree (the synthetic SH16 tree bench.py builds: depth 10, shell 2.5),
with the tree on the device and the result left there, in two modes:

  mask    every dense leaf (density > --sigma_thresh) is split: keys 1 / 0, no budget -- every lane of a wave in one bin
  top10   the leaves are ranked by their weight over --cams orbit cameras (rto_tree_leaf_weights) and the top 10 % of all leaves
          are split: the radix select runs all four passes

Per mode, wall ms around a synchronised call, every route warmed up once, then --runs runs in which the routes take turns, the
median per route:

  plan    rto_tree_refine_plan (links, levels, select, ranks; it drains its stream once)
  write   rto_tree_refine_write (child_out, data_out, slot_src), with its achieved GB/s: bytes read + bytes written
  copy    a device-to-device copy of the write's output bytes: the floor of the write
  torch   the same selection and output restated in torch on the same device: topk over the candidates' keys, gather, cat

Report only.  Output: profiles/refine_bench.txt (--out)."""
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


def torch_refine(child, data, key, K):
    """the restatement: child int32 [cap,8], data half [cap,8,D], key int64 [cap*8] (0 = no candidate) on the device"""
    import torch
    cap, S = child.shape
    flat = child.reshape(-1)
    cand = torch.nonzero((flat == 0) & (key > 0)).reshape(-1)
    if K < cand.numel():
        # key descending, slot ascending: one 64-bit sort key
        order = torch.topk((key[cand] << 32) | (0xFFFFFFFF - cand), K, sorted=False).indices
        cand = cand[order]
    sel = torch.sort(cand).values
    child_out = torch.cat([flat, torch.zeros(sel.numel() * S, dtype=torch.int32, device=flat.device)])
    child_out[sel] = (cap + torch.arange(sel.numel(), device=flat.device) - sel // S).to(torch.int32)
    slot_src = torch.cat([torch.arange(cap * S, device=flat.device), sel.repeat_interleave(S)])
    data_out = torch.cat([data.reshape(cap * S, -1), data.reshape(cap * S, -1)[sel].repeat_interleave(S, 0)])
    return child_out, data_out, slot_src.to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--sigma_thresh", type=float, default=0.0)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    child, data = np.ascontiguousarray(tree.child, np.int32), np.ascontiguousarray(tree.data, np.float16)
    cap, D = child.shape[0], data.shape[-1]
    print("tree built in %.1f s: capacity %d" % (time.time() - t0, cap), file=sys.stderr)
    dev_child, dev_data = torch.from_numpy(child).to("cuda:0"), torch.from_numpy(data).to("cuda:0")
    dt = R.N3Tree.from_arrays(child, data, tree.scale, tree.offset, tree.data_format)
    fx = synth.blender_focal(args.size)
    cams = []
    for p in synth.orbit_poses(args.cams):
        c = R.Camera(args.size, args.size, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    weights = R.leaf_weights(dt, cams)
    torch.cuda.synchronize()
    dt.free()
    leaves = int((dev_child == 0).sum())
    modes = {"mask": ((dev_data[..., -1].float() > args.sigma_thresh) & (dev_child == 0)).to(torch.int32).contiguous(),
             "top10": R.keys_from_weights(weights)}
    budgets = {"mask": -1, "top10": leaves // 10}
    r = R.Refiner(0)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    lines = ["# tools/refine_bench.py: tree depth %d, SH%d, shell %.1f: %d nodes, %d leaves" % (args.depth, args.basis, args.shell, cap, leaves),
             "# wall ms around a synchronised call; %d runs, the routes taking turns; device: %s" % (args.runs, torch.cuda.get_device_name(0))]
    for mode, key in modes.items():
        K = budgets[mode]
        capacity, st = r.plan(dev_child, key, 1, K)
        out_bytes = capacity * 8 * (4 + 4 + 2 * D)
        in_bytes = cap * 8 * (4 + 4 + 2 * D) + st["selected"] * (4 + 2 * D)  # child, rank, data of the old nodes; the picked slots and records
        buf_a = torch.empty(out_bytes, dtype=torch.uint8, device="cuda:0")
        buf_b = torch.empty(out_bytes, dtype=torch.uint8, device="cuda:0")
        key64 = key.to(torch.int64) & 0xFFFFFFFF
        routes = {"plan": lambda: r.plan(dev_child, key, 1, K),
                  "write": lambda: r.write(dev_child, dev_data, capacity),
                  "copy": lambda: buf_b.copy_(buf_a),
                  "torch": lambda: torch_refine(dev_child.reshape(cap, 8), dev_data.reshape(cap, 8, D), key64.reshape(-1), st["selected"])}
        outs = {name: timed(fn)[1] for name, fn in routes.items()}
        same = bool(torch.equal(outs["write"][0].reshape(-1), outs["torch"][0]) and torch.equal(outs["write"][2].reshape(-1), outs["torch"][2])
                    and torch.equal(outs["write"][1].reshape(-1, D).view(torch.int16), outs["torch"][1].view(torch.int16)))
        del outs
        ms = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():
                ms[name].append(timed(fn)[0])
        med = {name: float(np.median(v)) for name, v in ms.items()}
        lines.append(json.dumps(dict(mode=mode, budget=K, candidates=st["candidates"], selected=st["selected"], nodes_after=capacity,
                                     levels=st["levels"], cut_key=st["cut_key"], output_mb=round(out_bytes / 2.0 ** 20, 1),
                                     hip_equals_torch=same)))
        for name, v in ms.items():
            lines.append(json.dumps(dict(mode=mode, route=name, ms_median=round(med[name], 3), min=round(min(v), 3), max=round(max(v), 3),
                                         runs=[round(x, 3) for x in v])))
        lines.append(json.dumps(dict(mode=mode, write_gbs=round((in_bytes + out_bytes) / med["write"] / 1e6, 1),
                                     copy_gbs=round(2 * out_bytes / med["copy"] / 1e6, 1),
                                     write_over_copy=round(med["write"] / med["copy"], 2),
                                     plan_over_torch=round(med["plan"] / med["torch"], 3),
                                     plan_and_write_over_torch=round((med["plan"] + med["write"]) / med["torch"], 3))))
        del buf_a, buf_b, routes
        torch.cuda.empty_cache()
    r.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
