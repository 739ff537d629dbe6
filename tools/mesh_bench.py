"""ms per frame of rto_draw_mesh_layers at 800x800 (GPU box).

Two sets: a drawlist of 100 camera frusta (800 segments + 99 connecting ones) and a sphere of about 50 k triangles (160 x 160);
lone frames (one call per frame) and batches of 100 cameras per call, depth + colour, line_px 1.  Beside them, at the same build:
rto_draw_grid_layers (max_depth 4) and one rendered frame (rto_launch_renderer, SPP 6, no denoise) of the C2 tree for the same
cameras.  Every figure is the median of --reps timed runs of --iters back-to-back calls (HIP events).  Prints a table; --out FILE
also writes it there (profiles/mesh_bench.txt is this tool's output)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import rt_octree_amd as R  # noqa: E402
from rt_octree_amd import synth  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from grid_bench import c2_tree  # noqa: E402
from rays_bench import timed  # noqa: E402


def frusta(n, W):
    """n camera frusta on the orbit the benchmark renders from, pulled halfway in, joined into a trajectory"""
    fr = R.Mesh.CameraFrustum(synth.blender_focal(W), W, W, -0.3, (0.0, 0.0, 0.0))
    base = fr.vert[:, :3].astype(np.float64)
    verts, faces = [], []
    for k, p in enumerate(synth.orbit_poses(n)):
        v = fr.vert.copy()
        v[:, :3] = (base @ p[:3, :3].T + 0.5 * p[:3, 3]).astype(np.float32)
        verts.append(v)
        faces.append(fr.faces + 5 * k)
    faces.append(np.stack([5 * np.arange(n - 1), 5 * np.arange(1, n)], 1).astype(np.uint32))
    return R.Mesh(np.concatenate(verts), np.concatenate(faces), 2, True, "frusta")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-tree", action="store_true", help="skip the grid pass and the rendered frame (no C2 tree needed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    W = H = args.size
    fx = synth.blender_focal(W)
    cams = []
    for p in synth.orbit_poses(200)[:args.batch]:
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    dev = torch.device("cuda", 0)
    depth = torch.empty((args.batch, H, W), dtype=torch.float32, device=dev)
    color = torch.empty((args.batch, H, W, 4), dtype=torch.float32, device=dev)
    sets = [("100 frusta", R.MeshSet([frusta(100, W)])), ("sphere 160 x 160", R.MeshSet([R.Mesh.Sphere(160, 160)]))]
    params = R.MeshParams()
    lines = ["mesh_bench: %dx%d, line_px 1, depth + colour; median of %d x %d calls" % (W, H, args.reps, args.iters),
             "set | primitives | BVH nodes | lone frame ms | batch of %d: ms per frame | hit pixels of pose 0" % args.batch]
    for name, ms in sets:
        k = [0]

        def lone():
            R.draw_mesh_layers(ms, [cams[k[0] % len(cams)]], params, depth=depth[:1], color=color[:1])
            k[0] += 1

        ms1 = timed(lone, args.iters * 4, args.reps)
        msb = timed(lambda: R.draw_mesh_layers(ms, cams, params, depth=depth, color=color), args.iters, args.reps) / len(cams)
        R.draw_mesh_layers(ms, [cams[0]], params, depth=depth[:1], color=color[:1])
        lines.append("%s | %d | %d | %.4f | %.4f | %d" % (name, ms.n_prims, ms.nodes, ms1, msb, int(torch.isfinite(depth[0]).sum())))
    if not args.no_tree:
        dt = c2_tree(args.threads)
        gp = R.GridParams(max_depth=4)
        k = [0]

        def grid():
            R.draw_grid_layers(dt, [cams[k[0] % len(cams)]], gp, depth=depth[:1], color=color[:1])
            k[0] += 1

        lines.append("rto_draw_grid_layers, max_depth 4, same cameras: lone frame %.4f ms, batch %.4f ms per frame" % (
            timed(grid, args.iters * 4, args.reps),
            timed(lambda: R.draw_grid_layers(dt, cams, gp, depth=depth, color=color), args.iters, args.reps) / len(cams)))
        ctx = R.RenderContext(W, H)
        ctx.rng_seed()
        opt = R.RenderOptions(spp=6, denoise=False)

        def frame():
            R.launch_renderer(dt, cams[k[0] % len(cams)], opt, ctx, stream=torch.cuda.current_stream().cuda_stream)
            k[0] += 1

        lines.append("rto_launch_renderer, C2 tree, same cameras, SPP 6, no denoise, one frame per launch: %.4f ms per frame"
                     % timed(frame, args.iters * 4, args.reps))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
