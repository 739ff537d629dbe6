"""What the median-cut quantiser costs (GPU box), on the C2 bench tree (the synthetic SH16 tree bench.py builds: depth 10,
shell 2.5) with the live-slot triples (sigma > 2.0, compress_octree's default) of one basis function, 16 bits:

  hip         rto_quantize_median_cut through rt_octree_amd.quantize_median_cut: numpy rows in, numpy palette and ids out
  hip_device  the same entry with the rows already on the device and the results left there (the call drains its stream)
  torch_gpu   synth.median_cut_ids on the GPU, the development helper as it stands: numpy rows in, numpy out, sixteen 64-bit sorts
  host_twin   rto_quantize_median_cut_host

Wall time around each call with the device synchronised before and after; every route is warmed up once, then --runs runs in
which the GPU routes take turns; the median per route.  Also m, the whole tree through the HIP entry (15 basis functions, upload
of the [m,3,16] coefficients included), and hip against torch_gpu on the medians.  Output: profiles/quantize_bench.txt (--out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import compress_octree, quantize, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--basis", type=int, default=16)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--basis_function", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host_runs", type=int, default=1, help="runs of the host twin (it is the slow route)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize_bench.txt"))
    args = ap.parse_args()
    import torch
    t0 = time.time()
    tree = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=1.5, seed=20230418)
    D = tree.data_dim
    flat = tree.data.reshape(-1, D)
    live = np.ascontiguousarray(flat[compress_octree.live_slots(flat[:, D - 1], 2.0), :D - 1].reshape(-1, 3, args.basis))
    m = live.shape[0]
    rows = np.ascontiguousarray(live[:, :, args.basis_function])
    print("tree built in %.1f s: capacity %d, m = %d live slots" % (time.time() - t0, tree.capacity, m), file=sys.stderr)
    q = R.Quantizer(0)
    dev_rows = torch.from_numpy(rows).to("cuda:0")
    rows32 = rows.astype(np.float32)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    routes = {"hip": lambda: R.quantize_median_cut(rows, 16, backend="hip", quantizer=q),
              "hip_device": lambda: q.median_cut(dev_rows, 16), "torch_gpu": lambda: synth.median_cut_ids(rows32, 16, device="cuda")}
    outs = {name: timed(fn)[1] for name, fn in routes.items()}  # warm-up, and the values
    ms = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, fn in routes.items():
            ms[name].append(timed(fn)[0])
    ms["host_twin"] = []
    for _ in range(args.host_runs):
        t = time.perf_counter()
        host = quantize.quantize_median_cut_host(rows, 16)
        ms["host_twin"].append((time.perf_counter() - t) * 1e3)
    hip_pal, hip_ids = outs["hip"]
    same_as_host = bool(np.array_equal(hip_ids, host[1]) and np.array_equal(hip_pal.view(np.uint16), host[0].view(np.uint16)))
    ids_equal_torch = float(np.mean(outs["torch_gpu"][1].astype(np.uint16) == hip_ids))

    def whole_tree():
        dev = torch.from_numpy(live).to("cuda:0")
        for k in range(1, args.basis):
            q.median_cut(dev[:, :, k].contiguous(), 16)

    whole = [timed(whole_tree)[0] for _ in range(args.runs)]
    med = {name: float(np.median(v)) for name, v in ms.items()}
    lines = ["# tools/quantize_bench.py: median cut of the live-slot triples of basis function %d, 16 bits; tree depth %d, SH%d, shell %.1f"
             % (args.basis_function, args.depth, args.basis, args.shell),
             "# wall ms around a synchronised call; %d runs, the GPU routes taking turns (host twin: %d); device: %s"
             % (args.runs, args.host_runs, torch.cuda.get_device_name(0)),
             json.dumps(dict(m=m, capacity=int(tree.capacity)))]
    for name, v in ms.items():
        lines.append(json.dumps(dict(route=name, ms_median=round(med[name], 3), min=round(min(v), 3), max=round(max(v), 3),
                                     runs=[round(x, 3) for x in v])))
    lines.append(json.dumps(dict(whole_tree_hip_ms_median=round(float(np.median(whole)), 3), basis_functions=args.basis - 1,
                                 runs=[round(x, 3) for x in whole])))
    lines.append(json.dumps(dict(ratio_torch_gpu_over_hip=round(med["torch_gpu"] / med["hip"], 2), hip_equals_host_twin=same_as_host,
                                 fraction_of_ids_equal_to_torch_route=round(ids_equal_torch, 6))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    q.free()


if __name__ == "__main__":
    main()
