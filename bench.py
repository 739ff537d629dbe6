"""bench.py -- FPS of the RT-Octree hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one BATCH of synthetic input: --batch poses (default 100 = half of the
reference's 200-pose test loop) of config C2 -- batched-regular-tracking render (800x800, SPP 6) + GuidanceNet (the
compact network as one fused MFMA kernel; --torch-net runs it through PyTorch-ROCm/MIOpen) + guided filter, i.e. what
--batch iterations of the reference's timed loop do (main_headless.cpp:485-543) -- issued as one launch of the
persistent ray-queue traversal kernel + one shading launch, one batched GuidanceNet forward and one batched filter
launch: a frame alone cannot fill 256 CUs (DESIGN.md "Batching").  `value` is FRAMES per second whatever the step
size (frames = steps x batch x ranks); `reference_loop` reports the reference's own one-frame-per-launch loop shape
beside it.  Every image is bit-identical to rendering the poses one by one (tests/test_render_parity.py).

Inputs are synthetic (no dataset exists on either machine): a seeded lego-like SH16 PlenOctree of
~2.1 M nodes, a 200-pose blender orbit, the GuidanceNet trained by tools/train_guidance.py.
Everything is resident in HBM before the timed region.  Frames shard across ranks (frame g -> pose g of a 200 x N pose
orbit -> rank g mod N, RNG jump-ahead per pose so an image does not depend on who renders it); no data-path collective exists
or is invented -- the only collectives are the barrier and the max-reduction of the elapsed time.
--scenes K (config C3): K different synthetic scenes; --scene-map pose (every rank holds every scene,
frame g -> rank g mod N) or scene (scene s -> rank s mod N), or both.

A plain run (`--gpus N --steps K --warmup W`) does only what the headline needs: inputs, warm-up, the K timed steps, the
outputs if --dump-outputs DIR is given, and ONE JSON line from rank 0 with `metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step` (= the milliseconds of one timed step) and the workload's `config`.  --dump-outputs writes the
frames the timed path handed its caller in its last step (a fixed, seeded sample; see dump_outputs) as .npy files, so
that two builds can be compared output for output: the inputs are the same from run to run.

With --full the line also carries these objects, each measured or checked by passes of its own after the timed region:
  roofline       -- traversal kernel (render_persist).  `achieved` / `frac` = HBM bytes per launch from the
                    rocprofv3 counter passes committed under profiles/ (FETCH_SIZE + WRITE_SIZE, separate
                    passes, this workload) / this run's average launch duration (HIP events on the launch
                    stream, recorded around that kernel inside librto), against 8 TB/s.  The ALGORITHMIC
                    figure of SURVEY.md 8d (a root-restart walk priced at 4 B per level, which the kernel
                    does not perform) is kept as `algorithmic_gbps` / `algorithmic_frac`.  `tcp` relates the
                    kernel's L1 line accesses to the gather ceilings measured by tools/probe_ceiling.py --
                    the resource that actually bounds it.
  reference_loop -- the reference's own loop shape: ONE frame per launch with a host synchronisation per
                    frame (Timer::record, render_context.hpp:179-188), single-frame kernel; `pipelined` = the same
                    per-frame operator calls with --ref-loop-inflight frames in flight (frame i+1 is launched before
                    the host waits for frame i), wall-clock frames/s.
  parity_spot    -- untimed: pixels of frames of the LAST TIMED launch group compared bit for bit with the CPU oracle
                    (the checker, oracle/): a line can never be fast and wrong.
  value_exact    -- the same frames timed once more through the bit-exact route (exact filter, fp32 maps).
  cpu_baseline   -- the CPU oracle (oracle/, kind "port": the reference has no CPU renderer) on a
                    bounded sample of the same frames, all host cores.
"""
import argparse
import gc
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured float4 copy)
WARM_FRAMES_REF = 100  # main_headless.cpp:469-479: 100 warm-up frames each advance the RNG


def finite(o):  # strict JSON: no NaN / Infinity tokens in the driver's line
    if isinstance(o, float):
        return o if np.isfinite(o) else None
    if isinstance(o, dict):
        return {k: finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [finite(v) for v in o]
    if isinstance(o, (np.floating, np.integer)):
        return finite(o.item())
    return o


def emit(out):
    """the ONE JSON line of rank 0"""
    print(json.dumps(finite(out), allow_nan=False))
    sys.stdout.flush()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8, help="timed steps; one step = --groups-per-step launch groups of --batch frames")
    ap.add_argument("--warmup", type=int, default=2, help="untimed warm-up steps")
    ap.add_argument("--batch", type=int, default=100, help="frames per launch group (1..128)")
    ap.add_argument("--groups-per-step", type=int, default=12,
                    help="launch groups per step: one step = groups-per-step x batch frames (default 1200 = six passes over the "
                         "reference's 200-pose test trajectory), so that the driver's 20 steps keep the GPU busy for ~2 s")
    ap.add_argument("--size", type=int, default=800, help="square image size (config C2/C5)")
    ap.add_argument("--width", type=int, default=0, help="with --height: non-square frames (config C4: 1920x1080)")
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--psnr-frames", type=int, default=64, help="SPP-32 frames accumulated into the PSNR reference (0 = skip PSNR)")
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--basis", type=int, default=16, help="SH basis per channel (16 = the NeRF-synthetic PlenOctrees)")
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--shell", type=float, default=2.5)
    ap.add_argument("--radius", type=float, default=1.5, help="scene half-extent in world units (invradius = 1/(2 radius))")
    ap.add_argument("--fx", type=float, default=0.0, help="focal length in pixels (0 = the blender camera_angle_x of NeRF-synthetic; "
                                                          "config C4 uses the TanksAndTemple intrinsics, 1160)")
    ap.add_argument("--cam-radius", type=float, default=4.0311, help="radius of the camera orbit (world units)")
    ap.add_argument("--no-denoise", action="store_true", help="config C5: raw SPP render only")
    ap.add_argument("--cpu-frames", type=int, default=2, help="frames in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline (0 = all cores)")
    ap.add_argument("--ref-loop-frames", type=int, default=96,
                    help="frames of the one-frame-per-launch pass reported as reference_loop (0 = skip)")
    ap.add_argument("--ref-loop-inflight", type=int, default=4,
                    help="frames in flight in the pipelined variant of the reference loop (1 = skip it)")
    ap.add_argument("--spot-pixels", type=int, default=64, help="oracle spot pixels per checked frame of the last timed group (0 = skip)")
    ap.add_argument("--count-frames", type=int, default=64,
                    help="frames of the untimed work-unit count behind the algorithmic figures (0 = skip: profiling runs, whose "
                         "per-kernel counter means must hold the timed launches only)")
    ap.add_argument("--no-exact-pass", action="store_true", help="skip the second timed pass through the bit-exact filter route")
    ap.add_argument("--no-full-pass", action="store_true", help="skip the timed pass with the reference's full outputs (value_full_outputs)")
    ap.add_argument("--tree", default="", help="render this tree.npz instead of the synthetic one")
    ap.add_argument("--shuffle-nodes", type=int, default=0, metavar="SEED",
                    help="store the synthetic tree's nodes in a random order (seed > 0): svox-refined trees have no "
                         "ordering guarantee, make_tree's breadth-first order is the friendliest one; images are unchanged")
    ap.add_argument("--scenes", type=int, default=1, help="config C3: number of different synthetic scenes (1..8)")
    ap.add_argument("--scene-map", choices=("pose", "scene", "both"), default="pose",
                    help="with --scenes: 'pose' = every rank holds all scenes, frame g -> rank g mod N; 'scene' = scene s -> "
                         "rank s mod N; 'both' = time both, headline the pose mapping")
    ap.add_argument("--quant-direct", action="store_true",
                    help="with --tree <quantised tree.npz>: render from the codebooks instead of the expanded fp16 tree")
    ap.add_argument("--compact-records", action="store_true",
                    help="RTO_TREE_COMPACT_RECORDS: coefficient records for the leaves of positive density only (smaller footprint, one "
                         "more gather per hit leaf in the shading kernel)")
    ap.add_argument("--tuning", default="",
                    help="development: rto_ctx_set_tuning keys for the batched path, e.g. cu_queues=32,queue_group=16")
    ap.add_argument("--streams", type=int, default=2,
                    help="launch groups of the headline passes (`value`, `value_exact`, `value_full_outputs`) alternate over this many "
                         "HIP streams, each with its own context: the tail of one group's kernels overlaps the next group's head.  "
                         "With more than one, a single-stream pass of the same frames runs first and supplies the per-kernel "
                         "durations (roofline.*_ms, reference_timer): kernels that share the chip would not have clean ones")
    ap.add_argument("--torch-net", action="store_true", help="run GuidanceNet through PyTorch-ROCm (MIOpen) instead of the fused HIP kernel")
    ap.add_argument("--c4", action="store_true", help="shorthand for configs[3]: " + " ".join(C4_ARGS))
    ap.add_argument("--plan-only", action="store_true",
                    help="no GPU work: join the process group (gloo), print every rank's frame plan as JSON and exit -- "
                         "pins the rank / scene / pose / RNG-jump bookkeeping of a multi-GPU run on a CPU box")
    ap.add_argument("--net-cull", type=int, default=1, help="A/B: 0 = run GuidanceNet on every tile")
    ap.add_argument("--full-outputs", action="store_true",
                    help="A/B: the batched launches of the timed region store all 48 B per pixel (8 aux planes + noisy image) instead of "
                         "the 16 B the fused denoise stage reads (rto_ctx_set_lean_outputs; same denoised images)")
    ap.add_argument("--lean-level", type=int, default=2, choices=(1, 2),
                    help="lean outputs of the headline pass: 2 = sparse (nothing stored for the pixels of culled tiles: rto_ctx_set_lean_outputs "
                         "level 2, RTO_NET_INPUT_SPARSE), 1 = round 5's lean outputs")
    ap.add_argument("--no-filter-cull", action="store_true",
                    help="A/B: filter every tile, also those that see only culled (background) render tiles")
    ap.add_argument("--fp32-maps", action="store_true",
                    help="hand the GuidanceNet maps to the factorised filter as fp32 planes (the reference's tensors) instead "
                         "of the packed fp16 values the network actually produces: same pixels, twice the bytes")
    ap.add_argument("--exact-filter", action="store_true",
                    help="run the bit-exact guided filter (164 exps per pixel) instead of the factorised one")
    ap.add_argument("--full", action="store_true",
                    help="after the headline pass, run everything else the line reports: the single-stream, full-outputs and "
                         "bit-exact passes, the oracle spot check, the reference loop, the roofline counts, the copy bandwidth, "
                         "PSNR, the CPU baseline and (N > 1) the final gather.  Off: set-up, warm-up, timed steps, outputs, line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float32 / float64, < 64 MB)")
    args = ap.parse_args(argv)
    if args.c4:
        args = ap.parse_args((list(argv) if argv is not None else sys.argv[1:]) + C4_ARGS)
    return args


def tree_cache_path(args, scene=0):
    key = "d%d_s%g_b%d" % (args.depth, args.shell, args.basis)
    if args.radius != 1.5:
        key += "_r%g" % args.radius
    if scene:
        key += "_scene%d" % scene
    if args.shuffle_nodes:
        key += "_shuf%d" % args.shuffle_nodes
    tag = hashlib.sha1(open(os.path.join(ROOT, "rt-octree_amd", "synth.py"), "rb").read()).hexdigest()[:10]
    base = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    return os.path.join(base, "rto_bench_tree_%s_%s.npz" % (key, tag))


def parallel_sdf(sdf, threads):
    """`sdf` evaluated over blocks of points on a thread pool (numpy releases the GIL inside its loops).  Every point's
    distance depends on that point alone, so the values are the same bit for bit; generating the depth-10 bench tree
    spends more than half its time in the SDF, and a plain run must not spend it on one core."""
    if threads <= 1:
        return sdf
    from concurrent.futures import ThreadPoolExecutor

    def blocked(p):
        n = p.shape[0]
        if n < (1 << 16):
            return sdf(p)
        step = -(-n // (4 * threads))
        with ThreadPoolExecutor(threads) as ex:
            return np.concatenate(list(ex.map(lambda s: sdf(p[s:s + step]), range(0, n, step))))
    return blocked


def workload_id(args, W, H):
    """key into profiles/pmc_traffic.json: the BASELINE configurations the counter passes were taken on.  None for
    anything the committed counters do not describe: another scene or tree, development tuning, another library
    build (RTO_LIB).  (The stream count does not matter: the counters are per launch, and the launch durations they are divided by
    come from the single-stream pass.)"""
    if args.tree or args.shuffle_nodes or args.scenes != 1 or args.quant_direct or args.shell != 2.5:
        return None
    if args.tuning or os.environ.get("RTO_LIB") or args.compact_records:
        return None
    key = (W, H, args.spp, args.basis, args.depth, bool(args.no_denoise), args.radius, args.fx, args.cam_radius)
    return {(800, 800, 6, 16, 10, False, 1.5, 0.0, 4.0311): "c2", (800, 800, 1, 16, 10, True, 1.5, 0.0, 4.0311): "c5",
            (1920, 1080, 6, 25, 10, False, 1.12, 1160.0, 2.6): "c4"}.get(key)


KERNEL_SOURCES = ("render_kernels.hip", "rto_march_leaf.inc", "rto_kernel_types.h", "rto_device_math.h", "rto_launch.h")


def kernel_code_id():
    """identity of the traversal kernel's code: sha256 over the sources it is compiled from (what the counter passes in
    profiles/pmc_traffic.json are tied to -- tools/pmc_traffic.py stores the same value)"""
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "rt-octree_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


# BASELINE.json configs[3] (TanksAndTemple Truck 1920x1080 SPP 6 + denoise) as a synthetic stand-in: SH25, a tree
# twice the size of C2's (smaller world radius = the model fills the volume), T&T intrinsics, a close orbit
C4_ARGS = ["--width", "1920", "--height", "1080", "--basis", "25", "--depth", "10", "--radius", "1.12", "--fx", "1160",
           "--cam-radius", "2.6"]


def usable_cores():
    """CPU cores this process may actually use: the affinity mask, capped by the cgroup's CPU quota.  (The GPU boxes show
    256 logical CPUs and a quota of 16: a team of 256 OpenMP threads is then throttled to a fraction of one core each --
    rounds 1-3 quoted "256 cores" for a baseline that ran at single-core speed.)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:  # cgroup v1
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = float(f.read()), float(g.read())
                if q > 0:
                    quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(quota)))
    return max(1, n)


def n_poses_for(world):
    """Poses of the synthetic orbit.  One GPU renders the reference's 200-pose test trajectory; N ranks render an orbit N
    times as dense, frame g -> pose g -> rank g mod N: every rank's launch groups then hold DISTINCT poses at the angular
    spacing of the 1-GPU run (1/200 of the orbit) -- with 200 poses over 8 ranks a 100-frame group would hold every pose
    four times, and four identical frames per launch flatter the caches (weak scaling must not get easier per GPU)."""
    return 200 * max(1, int(world))


def scenes_of_rank(rank, world, n_scenes, scene_map):
    """scenes a rank must hold: all of them when frames are interleaved, its own share when scenes are dealt out"""
    if n_scenes == 1 or scene_map == "pose":
        return list(range(n_scenes))
    return [s for s in range(n_scenes) if s % world == rank] or [rank % n_scenes]


def pose_schedule(step, rank, world, n_poses, n_scenes, scene_map):
    """(scene, pose) of this rank's `step`-th frame.
    'pose': the global frame sequence g = 0, 1, 2, ... runs scene after scene (scene = (g // n_poses) mod
            n_scenes, pose = g mod n_poses) and frame g belongs to rank g mod world (one scene: pose i -> rank i mod N);
    'scene': rank r renders the scenes s with s mod world == r, one after the other, all poses each."""
    if n_scenes > 1 and scene_map == "scene":
        mine = scenes_of_rank(rank, world, n_scenes, scene_map)
        return mine[(step // n_poses) % len(mine)], step % n_poses
    g = step * world + rank
    return (g // n_poses) % n_scenes, g % n_poses


def plan_groups(n_frames, B, rank, world, n_poses, n_scenes, scene_map):
    """a rank's frames 0..n_frames-1 cut into launch groups of <= B frames of one scene: [(scene, [poses])]"""
    groups = []
    s = 0
    while s < n_frames:
        sc, first = pose_schedule(s, rank, world, n_poses, n_scenes, scene_map)
        idx = [first]
        while len(idx) < B and s + len(idx) < n_frames:
            sc2, p2 = pose_schedule(s + len(idx), rank, world, n_poses, n_scenes, scene_map)
            if sc2 != sc:
                break
            idx.append(p2)
        groups.append((sc, idx))
        s += len(idx)
    return groups


def plan_only(args):
    """--plan-only: what every rank WOULD render (no GPU): {"world", "plans": {map: [[(scene, [poses]) ...] per rank]},
    "rng_jumps": the per-frame jump of pose i}; ranks exchange their plans over gloo."""
    import torch.distributed as dist
    rank, world, _ = check_world(args)
    B = max(1, min(128, args.batch))
    n_scenes = 1 if args.tree else max(1, min(8, args.scenes))
    maps = ["pose", "scene"] if n_scenes > 1 else ["pose"]
    mine = {m: plan_groups(args.steps * B * max(1, args.groups_per_step), B, rank, world, n_poses_for(world), n_scenes, m) for m in maps}
    plans = [mine]
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        plans = [None] * world
        dist.all_gather_object(plans, mine)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"world": world, "steps": args.steps, "batch": B, "groups_per_step": max(1, args.groups_per_step), "frames_per_rank": args.steps * B * max(1, args.groups_per_step), "scenes": n_scenes,
                          "plans": {m: [plans[r][m] for r in range(world)] for m in maps},
                          "rng_jump_of_pose": "%d + pose" % WARM_FRAMES_REF}))


def self_launch(args, argv=None):
    """`bench.py --gpus N` with no launcher around it (WORLD_SIZE unset, N > 1): start the N ranks HERE, as a CHILD process
    running the driver's own line (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same
    args>`), relay its output and return its exit code.  Called before torch is imported: this process never touches a
    GPU (nothing is exec'ed from a process that initialised HIP; the child is started, not exec'ed into).  The
    reference has no multi-GPU mode -- it selects ONE device (main_headless.cpp:234-238, opts.cpp:13-14); SURVEY 8e."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    cmd += list(sys.argv[1:] if argv is None else argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               RTO_BENCH_SELF_LAUNCHED="1")
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cores() // args.gpus)))
    print("[bench] --gpus %d without a launcher: starting %d ranks as a child process: %s" % (args.gpus, args.gpus, " ".join(cmd)),
          file=sys.stderr)
    sys.stderr.flush()
    return subprocess.call(cmd, env=env)


def check_world(args):
    """(rank, world, local_rank) from the launcher's environment; a launcher whose WORLD_SIZE differs from --gpus is
    refused (N = 1 included: `--gpus 8` inside a 1-rank launcher must not print a one-GPU line as if it were 8)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %s: start bench.py with --gpus equal to the number of ranks "
                         "(or without a launcher: it starts its own ranks)" % (args.gpus, os.environ.get("WORLD_SIZE", "unset")))
    return rank, world, int(os.environ.get("LOCAL_RANK", "0"))


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.plan_only:
        return plan_only(args)
    import torch
    import torch.distributed as dist

    import rt_octree_amd as R
    from rt_octree_amd import denoiser, synth

    rank, world, local_rank = check_world(args)
    # one rank per GPU; RTO_BENCH_BACKEND=gloo lets several ranks share one GPU to smoke-test the
    # multi-process control flow on a single-GPU box (RCCL refuses two ranks on one device)
    backend = os.environ.get("RTO_BENCH_BACKEND", "nccl")
    n_dev = torch.cuda.device_count()  # (counting devices does not initialise HIP)
    if n_dev < 1 or not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the render path has no CPU fallback")
    if world > n_dev and backend == "nccl":
        raise SystemExit("--gpus %d but this node shows %d GPU(s): one rank per GPU over RCCL (RTO_BENCH_BACKEND=gloo lets "
                         "ranks share a GPU for a control-flow smoke test only)" % (world, n_dev))
    local_rank = local_rank % n_dev
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    def barrier():
        if world > 1:
            dist.barrier()

    # ---------------- inputs (untimed) ----------------
    W = H = args.size
    if args.width > 0 and args.height > 0:
        W, H = args.width, args.height
    B = max(1, min(128, args.batch))
    n_scenes = 1 if args.tree else max(1, min(8, args.scenes))
    maps = ["pose", "scene"] if (args.scene_map == "both" and n_scenes > 1) else [args.scene_map if args.scene_map != "both" else "pose"]
    tree_host = None
    if args.tree:
        paths = [args.tree]
    else:
        paths = [tree_cache_path(args, s) for s in range(n_scenes)]
        for s, path in enumerate(paths):
            # scene generation is spread over the ranks (rank r writes the scenes s with s mod world == r)
            if s % world == rank and not os.path.exists(path):
                t0 = time.time()
                th = synth.make_tree(depth_limit=args.depth, basis_dim=args.basis, shell=args.shell, radius=args.radius,
                                     sdf=parallel_sdf(synth.scene_variant(s), max(1, usable_cores() // world)), seed=20230418 + s)
                if args.shuffle_nodes:
                    th = synth.shuffle_nodes(th, args.shuffle_nodes)
                tmp = "%s.tmp%d.npz" % (path, rank)
                th.save_npz(tmp)
                os.replace(tmp, path)
                print("[bench] generated %s: %s in %.1fs" % (path, th.stats, time.time() - t0), file=sys.stderr)
                if s == 0:
                    tree_host = th
    barrier()
    need = set()
    for m in maps:
        need |= set(scenes_of_rank(rank, world, n_scenes, m))
    trees = {s: R.N3Tree(paths[s], device=local_rank, quant_direct=args.quant_direct, compact_records=args.compact_records)
             for s in sorted(need)}  # tree.npz -> device
    tree = trees[min(trees)]
    poses = synth.orbit_poses(n_poses_for(world), radius=args.cam_radius)
    fx = args.fx if args.fx > 0 else synth.blender_focal(W)
    cams = []
    for p in poses:
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(p)
        cams.append(c)
    ctx = R.RenderContext(W, H, device=local_rank, frames=B)
    for kv in filter(None, args.tuning.split(",")):
        ctx.set_tuning(kv.split("=")[0], int(kv.split("=")[1]))
    denoise = not args.no_denoise
    opt = R.RenderOptions(spp=args.spp, denoise=denoise)
    net = full = compact = None
    trained = False
    if denoise:
        torch.manual_seed(0)
        full = denoiser.GuidanceNet(8, 32, 5, 2, 4)
        # weights trained on MI355X by tools/train_guidance.py (this repository's renderer + the HIP filter
        # forward/backward) on the default synthetic scene; poses with index % 4 == 0 (pose 0 scored
        # below among them) were held out.  Without the file: seeded random weights.
        wpath = os.path.join(ROOT, "rt-octree_amd", "weights", "guidance_synth_lego.pt")
        trained = os.path.exists(wpath)
        if trained:
            full.load_state_dict(torch.load(wpath, map_location="cpu"))
        compact = denoiser.GuidanceNetCompact.from_full(full).eval()
        if args.torch_net:
            net = compact.half().to(dev)
        else:
            net = denoiser.FusedGuidanceNet(compact, device=local_rank)  # same weights, one HIP kernel
    stream = torch.cuda.current_stream(dev)
    aux_t = torch.as_tensor(ctx.batch_views()[0], device=dev)  # zero-copy [B,8,H,W]
    # lane = (context, stream, network instance with its own output buffers, aux view)
    lanes = [(ctx, stream, net, aux_t)]
    # lean outputs (round 5): the timed launch groups store (r, g, b, alpha) per pixel -- what GuidanceNet + filter read -- and
    # no aux planes; only with the fused network (PyTorch's reads the aux tensor) and with denoise on
    lean = denoise and not args.torch_net and not args.full_outputs
    noisy_of = {id(ctx): torch.as_tensor(ctx.batch_views()[1], device=dev)}  # zero-copy [B,H,W,4]
    # One pool of side streams for the whole process: the runtime maps streams onto FOUR hardware queues, and a fifth stream
    # shares a queue with another one -- round 6's first lines created a stream for the second lane and three more for the
    # pipelined reference loop, whose four frames "in flight" then ran on three queues (5.5 k instead of 6.7 k frames/s)
    side_streams = []

    def side_stream(k):
        while len(side_streams) <= k:
            side_streams.append(torch.cuda.Stream(dev))
        return side_streams[k]

    for _ in range(1, max(1, args.streams)):
        c2 = R.RenderContext(W, H, device=local_rank, frames=B)
        for kv in filter(None, args.tuning.split(",")):
            c2.set_tuning(kv.split("=")[0], int(kv.split("=")[1]))
        n2 = None
        if denoise:
            n2 = compact.half().to(dev) if args.torch_net else denoiser.FusedGuidanceNet(compact, device=local_rank)
        lanes.append((c2, side_stream(len(lanes) - 1), n2, torch.as_tensor(c2.batch_views()[0], device=dev)))
        noisy_of[id(c2)] = torch.as_tensor(c2.batch_views()[1], device=dev)

    filter_mode = R.FILTER_EXACT if args.exact_filter else R.FILTER_FAST
    FS = B * max(1, args.groups_per_step)  # frames per step
    n_frames = args.steps * FS  # timed frames of this rank
    # fused GuidanceNet + factorised filter: keep the maps in fp16 between the two kernels (same pixels, half the bytes)
    packed_route = denoise and not args.torch_net and not args.exact_filter and not args.fp32_maps

    def frame_of(step, scene_map):  # (scene, pose) of this rank's `step`-th frame
        return pose_schedule(step, rank, world, len(poses), n_scenes, scene_map)

    def group(scene, idx, ev, lane=0, exact=False, lean_g=None):
        """The frames `idx` (poses of one scene): traversal + shading, GuidanceNet, filter; all asynchronous
        on the lane's stream, no host sync (the reference synchronises once per frame,
        render_context.hpp:179-188).  Frame i of the reference run uses the RNG advanced (100 + i) times
        (SURVEY 8e).  exact: the bit-exact denoise route (fp32 maps + exact filter) whatever the command line says."""
        n = len(idx)
        lctx, lstream, lnet, laux = lanes[lane]
        lctx.rng_seed()
        use_lean = lean if lean_g is None else bool(lean_g)
        # sparse (level 2): only where both denoise kernels get the launch's tile marks and run the packed route
        sparse = bool(use_lean and args.lean_level == 2 and packed_route and not exact and not args.no_filter_cull and args.net_cull)
        lctx.set_lean_outputs(2 if sparse else (1 if use_lean else 0))
        net_in = dict(rgba=True) if use_lean else dict(squares_implied=True)
        if use_lean:
            laux = noisy_of[id(lctx)]  # the network reads the (r, g, b, alpha) image the launch leaves
        if ev:
            ev[0].record(lstream)
        R.launch_renderer_batch(trees[scene], [cams[i] for i in idx], opt, lctx, lstream,
                                rng_jumps=[WARM_FRAMES_REF + i for i in idx])
        lctx.set_lean_outputs(0)  # (every other pass of this script reads full outputs)
        if ev:
            ev[1].record(lstream)
        if denoise:
            lctx.select_frame(0)
            if packed_route and not exact:  # GuidanceNet -> fp16 maps in the handle's scratch -> factorised filter
                # (network / filter tiles that see only culled = background render tiles are filled, not computed: same bits)
                marks = None if args.no_filter_cull else lctx.tile_marks()
                lnet.forward_packed(laux[:n], stream=lstream, cull=marks if args.net_cull else None, sparse=sparse, **net_in)
                if ev:
                    ev[2].record(lstream)
                lnet.filter_packed(lctx.noisy_ptr, lctx.image_ptr, stream=lstream, shape=(n, H, W), cull=marks)
            elif not args.torch_net:  # fp32 weight / guidance planes (the reference's tensors); exact: the bit-exact filter
                marks = None if args.no_filter_cull else lctx.tile_marks()
                wm, gm = lnet(laux[:n], stream=lstream, cull=marks if args.net_cull else None, **net_in)
                if ev:
                    ev[2].record(lstream)
                lnet.filter_planes(wm, gm, lctx.noisy_ptr, lctx.image_ptr, mode=R.FILTER_EXACT if exact else filter_mode,
                                   stream=lstream, cull=marks)
            else:
                with torch.no_grad(), torch.cuda.stream(lstream):
                    wm, gm = lnet(laux[:n])
                if ev:
                    ev[2].record(lstream)
                R.filtering(lstream, wm, gm, lctx.noisy_ptr, lctx.image_ptr, mode=R.FILTER_EXACT if exact else filter_mode)
            if ev:
                ev[3].record(lstream)

    def plan(n_frames, scene_map):
        return plan_groups(n_frames, B, rank, world, len(poses), n_scenes, scene_map)

    def timed(scene_map, exact=False, nl=None, lean_g=None):
        """one timed pass: W warm-up steps, then exactly K steps between barrier + synchronize; the launch groups alternate over
        the first `nl` lanes (streams)"""
        lanes = all_lanes[:nl or len(all_lanes)]
        warm, work = plan(args.warmup * FS, scene_map), plan(n_frames, scene_map)
        events = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in work]
        if work:  # allocation pass (untimed, whatever --warmup is): every lane sees the largest group once, so no
            # buffer of the library or of torch's allocator is created inside the timed region
            big = max(work, key=lambda g: len(g[1]))
            for ln in range(len(lanes)):
                group(big[0], big[1], None, ln, exact, lean_g)
            torch.cuda.synchronize(dev)
        for g, (sc, idx) in enumerate(warm):
            group(sc, idx, None, g % len(lanes), exact, lean_g)
        torch.cuda.synchronize(dev)
        for lc, _, _, _ in lanes:
            lc.kernel_timing(True)
        barrier()
        torch.cuda.synchronize(dev)
        # No Python garbage collection inside the timed region: a full collection of a process that holds torch and the
        # host copy of the tree takes 35-40 ms, as long as the whole timed region of the SPP-1 configuration, and whether
        # one falls into the region depends on allocation counts (round 3: C5 read 10 k or 21 k frames/s from one run to
        # the next until this was found; the GPU timeline of both was the same).
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        host_ms = []
        for g, (sc, idx) in enumerate(work):
            t1 = time.perf_counter()
            group(sc, idx, events[g], g % len(lanes), exact, lean_g)
            host_ms.append((time.perf_counter() - t1) * 1e3)
        t_issued = time.perf_counter() - t0
        torch.cuda.synchronize(dev)
        barrier()
        elapsed = time.perf_counter() - t0
        gc.enable()
        if os.environ.get("RTO_BENCH_DEBUG"):
            print("[bench] host ms per group call: %s; issued after %.1f ms, done after %.1f ms" % (
                " ".join("%.2f" % h for h in host_ms), t_issued * 1e3, elapsed * 1e3), file=sys.stderr)
        if world > 1:
            t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        kts = [lc.kernel_timing_read() for lc, _, _, _ in lanes]
        for lc, _, _, _ in lanes:
            lc.kernel_timing(False)
        n_launch = max(sum(k["launches"] for k in kts), 1)  # per-launch means, weighted over the lanes
        kt = {"launches": sum(k["launches"] for k in kts),
              "raygen_ms": sum(k["raygen_ms"] * k["launches"] for k in kts) / n_launch,
              "traverse_ms": sum(k["traverse_ms"] * k["launches"] for k in kts) / n_launch,
              "shade_ms": sum(k["shade_ms"] * k["launches"] for k in kts) / n_launch}
        # Timer::report formula (render_context.hpp:190-206), per frame, from the per-group event pairs
        render_ms = sum(e[0].elapsed_time(e[1]) for e in events) / n_frames
        torch_ms = sum(e[1].elapsed_time(e[2]) for e in events) / n_frames if denoise else 0.0
        filter_ms = sum(e[2].elapsed_time(e[3]) for e in events) / n_frames if denoise else 0.0
        all_ms = render_ms + torch_ms + filter_ms
        return elapsed, kt, {"render_ms": render_ms, "torch_ms": torch_ms, "filter_ms": filter_ms,
                             "fps": 1000.0 / all_ms if all_ms > 0 else 0.0, "frames": n_frames}, work

    def dump_outputs(out_dir, work):
        """--dump-outputs: what the timed pass `work` handed its caller in its last step -- each frame's `image` buffer (the
        denoised image; the raw render with --no-denoise) -- for the frames of that step still held by the lanes (the last
        launch group of each lane).  A fixed, seeded sample, at most 64 MB: every such frame at the same pixels
        (images_sampled [F, P, 4], sample_pixels = y * W + x, sample_frames = (scene, pose) of each frame, in frame order) and
        the last frame whole (image_last [H, W, 4]) where it fits."""
        starts = np.cumsum([0] + [len(idx) for _, idx in work])
        pick, frames = [], []
        for g in range(max(0, len(work) - NL), len(work)):
            sc, idx = work[g]
            for k, pose in enumerate(idx):
                if starts[g] + k >= n_frames - FS:  # (a frame of the last step)
                    pick.append((g % NL, k))
                    frames.append((sc, pose))
        if not pick:
            return
        os.makedirs(out_dir, exist_ok=True)
        budget = 60 << 20
        whole = H * W * 4 * 4
        keep_whole = whole <= budget // 2
        P = int(min(8192, H * W, (budget - (whole if keep_whole else 0)) // (16 * len(pick))))
        pix = np.sort(np.random.default_rng(20230418).choice(H * W, P, replace=False))
        pix_t = torch.as_tensor(pix, device=dev)
        imgs = {ln: torch.as_tensor(lanes[ln][0].batch_views()[2], device=dev) for ln in {ln for ln, _ in pick}}
        torch.cuda.synchronize(dev)
        sampled = np.stack([imgs[ln][k].reshape(H * W, 4).index_select(0, pix_t).cpu().numpy() for ln, k in pick])
        np.save(os.path.join(out_dir, "images_sampled.npy"), sampled.astype(np.float32))
        np.save(os.path.join(out_dir, "sample_pixels.npy"), pix.astype(np.float64))
        np.save(os.path.join(out_dir, "sample_frames.npy"), np.asarray(frames, np.float64))
        if keep_whole:
            ln, k = pick[-1]
            np.save(os.path.join(out_dir, "image_last.npy"), imgs[ln][k].cpu().numpy().astype(np.float32))

    # ---------------- warm-up + timed region(s) ----------------
    if denoise and not args.torch_net:
        for _, _, lnet, _ in lanes:  # the packed-map scratch at its final size: no allocation (= device sync) in a timed region
            lnet.reserve(B, H, W)
    NL = len(lanes)
    all_lanes = lanes
    # (VERDICT r5 task 4) the headline passes overlap launch-group tails over NL streams; the per-kernel durations and the
    # Timer::report buckets come from a single-stream pass of the same frames, where no other kernel shares the chip
    single = timed(maps[0], nl=1) if (NL > 1 and args.full) else None
    elapsed, kt, tstats, work = timed(maps[0], nl=NL)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, work)
    frames_per_launch = n_frames / max(kt["launches"], 1)
    value_single = None
    if single:
        value_single = n_frames * world / single[0]
        kt, tstats = single[1], single[2]
    alt = None
    if len(maps) > 1:
        e2, _, t2, _ = timed(maps[1], nl=NL)
        alt = {"scene_map": maps[1], "value": n_frames * world / e2, "ms_per_step": e2 / args.steps * 1e3,
               "reference_timer_fps": t2["fps"]}

    # ---------------- the headline line: all of a plain run, the first keys of a --full one ----------------
    wid = workload_id(args, W, H)
    total_frames = n_frames * world
    head = {
        "metric": "FPS @ 800x800 (Lego SPP=6) + PSNR vs ref; 1/2/4/8 GPU scaling",
        "value": total_frames / elapsed,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if not denoise else "f32 (traversal, filter) + f16 x f16 -> f32 (GuidanceNet conv, %s)" % ("MIOpen" if args.torch_net else "fused MFMA kernel"),
        "data": "synthetic",
    }
    config = {
        "workload": "configs[%s]: %slego-like synthetic PlenOctree %s (%d nodes, depth %d), %dx%d SPP=%d%s, 1 step = %d launch groups of %d frames, frames sharded %s"
                    % ({"c2": "1", "c4": "3 stand-in", "c5": "4"}.get(wid, "2" if n_scenes > 1 else "1-like"),
                       ("%d scenes, " % n_scenes) if n_scenes > 1 else "",
                       tree.data_format, tree.capacity, tree.max_depth, W, H, args.spp,
                       " + GuidanceNet(8,32,5,2,4) denoise" if denoise else " raw (no denoise)", max(1, args.groups_per_step), B,
                       "scene s -> rank s mod N" if (maps[0] == "scene" and n_scenes > 1) else "frame g -> rank g mod N"),
        "tree_nodes": int(tree.capacity), "tree_device_mb": tree.device_bytes / 1e6,
        "frames_per_step": FS, "groups_per_step": max(1, args.groups_per_step), "frames_per_group": B, "frames_timed": total_frames, "frames_per_launch": frames_per_launch, "streams": len(lanes),
        "scenes": n_scenes, "scene_map": maps[0], "filter": "exact" if args.exact_filter else "factorised", "maps": "fp16 packed" if packed_route else "fp32 planes",
        "parallelism": "frames x%d" % world,
        # which clause of the north star each figure claims (VERDICT r4 task 4)
        "value_route": ("render stage bit-exact against oracle/ (fp32 aux planes / RGBA8 of the noisy frame: parity_spot); denoise "
                        "stage = fused fp16 GuidanceNet + %s" % ("the bit-exact filter" if (args.exact_filter or not packed_route) else
                        "FACTORISED filter on packed fp16 maps: the TOLERANCE route (north star: 'within 1e-4 PSNR otherwise'; "
                        "150 dB against the exact filter, psnr.rgba8_bytes_differing_factorised_vs_exact)")) if denoise else
                       "raw render, bit-exact against oracle/",
        "lean_outputs": bool(lean),
        "lean_level": (args.lean_level if lean else 0),  # 2: sparse -- the headline launches store nothing for the pixels of culled tiles
        "world": world, "backend": (backend if world > 1 else None), "gpus_visible": n_dev,
        "launcher": ("none" if world == 1 else "bench.py itself (child torch.distributed.run)"
                     if os.environ.get("RTO_BENCH_SELF_LAUNCHED") else "external (torchrun)"),
        "full": bool(args.full),
    }
    if not args.full:  # a plain run ends here: everything below measures or checks something beside the headline
        if rank == 0:
            emit(dict(head, config=config, alt_scene_map=alt))
        if world > 1:
            dist.destroy_process_group()
        return
    last_group, last_lane = work[-1], (len(work) - 1) % NL

    def snapshot_last_group():
        """frames of the last timed launch group, kept for the oracle spot check below (later passes reuse the buffers)"""
        out = []
        if rank == 0 and args.spot_pixels > 0 and not args.quant_direct and not args.tree:  # (rank 0 checks its own frames at any N)
            lctx = lanes[last_lane][0]
            nlast = len(last_group[1])
            for slot in sorted({0, nlast // 2, nlast - 1}):
                lctx.select_frame(slot)
                # (lean launch: no aux planes -- the noisy image holds planes 0..3 as (r, g, b, alpha); planes 4..7 are their squares)
                snap = (lctx.download_image(noisy=True, stream=lanes[last_lane][1]).transpose(2, 0, 1) if lctx.frames_are_lean(slot, 1)
                        else lctx.download_aux(stream=lanes[last_lane][1]))
                out.append((last_group[0], last_group[1][slot], snap))
            lctx.select_frame(0)
        return out

    spot_frames = snapshot_last_group()
    #  the same frames with the reference's full outputs (8 aux planes + image, 48 B per pixel): the like-for-like
    # figure next to the lean headline, and an 8-plane spot check
    full_pass, spot_frames_full = None, []
    if lean and not args.no_full_pass:
        e4, _, _, _ = timed(maps[0], nl=NL, lean_g=False)
        full_pass = {"value": n_frames * world / e4, "ms_per_step": e4 / args.steps * 1e3}
        spot_frames_full = snapshot_last_group()
    # the same frames once more through the bit-exact route (exact filter on fp32 maps): VERDICT r2 task 3
    exact_pass = None
    if denoise and not args.no_exact_pass and not args.exact_filter and not args.torch_net:
        e3, _, t3, _ = timed(maps[0], exact=True, nl=NL)
        exact_pass = {"value": n_frames * world / e3, "ms_per_step": e3 / args.steps * 1e3, "reference_timer": t3 if NL == 1 else None,
                      "route": "fused GuidanceNet -> fp32 weight / guidance planes -> filter_fused (bit-identical to the CPU oracle's filter)"}
    if full_pass or exact_pass:
        group(work[-1][0], work[-1][1], None, last_lane)  # leave the headline route's frames in the buffers
        torch.cuda.synchronize(dev)
    # empty-space culling: the share of 8x8 tile slots of the last launch group that was marched at all
    try:
        live_slots, all_slots = lanes[last_lane][0].queue_stats()
    except Exception:
        live_slots, all_slots = None, None

    # ---------------- untimed, N > 1: the path's one collective -- the final gather of RGBA8 frames to rank 0 ----------------
    # (rt-octree_amd/sharding.py gather_frames: one padded all_gather, RCCL over xGMI with device tensors; the same code
    #  tests/test_sharding.py runs over gloo on CPUs and, given two GPUs, over RCCL.)  K frames per rank, global frame
    #  g -> rank g mod N; rank 0 then renders a frame that ANOTHER rank owned and compares the bytes: images must not
    #  depend on N.
    gather = None
    if world > 1 and maps[0] == "pose":
        from rt_octree_amd import sharding
        K = 2
        steps_g = list(range(K))
        sc_g = [frame_of(st, "pose") for st in steps_g]
        if len({sc for sc, _ in sc_g}) == 1:
            ctx.rng_seed()
            R.launch_renderer_batch(trees[sc_g[0][0]], [cams[i] for _, i in sc_g], opt, ctx, stream,
                                    rng_jumps=[WARM_FRAMES_REF + i for _, i in sc_g])
            local = {}
            for k, st in enumerate(steps_g):
                ctx.select_frame(k)
                local[st * world + rank] = ctx.download_rgba8(noisy=denoise, stream=stream)
            ctx.select_frame(0)
            barrier()
            t0g = time.perf_counter()
            gather_err = None
            try:
                frames_g = sharding.gather_frames(local, K * world, rank, world, dist=dist, device=dev if backend == "nccl" else None)
            except Exception as e:  # the untimed collective must not cost the run its measured line
                frames_g, gather_err = None, repr(e)
                print("[bench] rank %d: final gather failed: %s" % (rank, gather_err), file=sys.stderr)
            barrier()
            tg = time.perf_counter() - t0g
            if rank == 0 and frames_g is None:
                gather = {"error": gather_err, "backend": backend, "world": world}
            elif rank == 0:
                other = 1  # global frame 1 belongs to rank 1: (scene, pose) = pose_schedule(0, 1, world, ...)
                sc_o, i_o = pose_schedule(0, 1, world, len(poses), n_scenes, "pose")
                same = None
                if sc_o in trees:
                    ctx.rng_seed()
                    R.launch_renderer_batch(trees[sc_o], [cams[i_o]], opt, ctx, stream, rng_jumps=[WARM_FRAMES_REF + i_o])
                    ctx.select_frame(0)
                    same = bool(np.array_equal(ctx.download_rgba8(noisy=denoise, stream=stream), frames_g[other]))
                nbytes = sum(f.nbytes for f in frames_g)
                gather = {"frames": len(frames_g), "bytes": nbytes, "seconds": tg, "backend": backend,
                          "world": dist.get_world_size(), "ranks_on_distinct_gpus": bool(world <= n_dev),
                          "frame_of_rank_1_rendered_on_rank_0_is_identical": same,
                          "note": "sharding.gather_frames: one padded all_gather of uint8 [K,H,W,4] per rank (host -> device -> "
                                  "RCCL -> host, untimed plumbing); the timed region has no collective"}

    ref_loop = None
    if args.ref_loop_frames > 0 and not args.quant_direct:
        nf = args.ref_loop_frames

        def one_frame(lctx, lstream, lnet, laux, sc, i, evs=None):
            """the reference's loop body (main_headless.cpp:485-543) for pose i: per-frame operator calls only"""
            lctx.rng_seed()
            lctx.rng_advance((WARM_FRAMES_REF + i) << 32)
            if evs:
                evs[0].record(lstream)
            R.launch_renderer(trees[sc], cams[i], opt, lctx, lstream)
            if evs:
                evs[1].record(lstream)
            if denoise:
                lctx.select_frame(0)
                if packed_route:
                    marks = None if args.no_filter_cull else lctx.tile_marks()  # (None after the single-frame kernels)
                    lnet.forward_packed(laux[:1], stream=lstream, squares_implied=True, cull=marks if args.net_cull else None)
                    if evs:
                        evs[2].record(lstream)
                    lnet.filter_packed(lctx.noisy_ptr, lctx.image_ptr, stream=lstream, shape=(1, H, W), cull=marks)
                else:
                    with torch.no_grad(), torch.cuda.stream(lstream):
                        wm, gm = lnet(laux[:1], stream=lstream, squares_implied=True) if not args.torch_net else lnet(laux[:1])
                    if evs:
                        evs[2].record(lstream)
                    R.filtering(lstream, wm, gm, lctx.noisy_ptr, lctx.image_ptr, mode=filter_mode)
                if evs:
                    evs[3].record(lstream)

        def lane_net():
            if not denoise:
                return None
            return compact.half().to(dev) if args.torch_net else denoiser.FusedGuidanceNet(compact, device=local_rank)

        def tune(c):
            for kv in filter(None, args.tuning.split(",")):
                c.set_tuning(kv.split("=")[0], int(kv.split("=")[1]))
            return c

        one = tune(R.RenderContext(W, H, device=local_rank, frames=1))
        one_aux = torch.as_tensor(one.batch_views()[0], device=dev)
        one_net = lane_net()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        sums = [0.0, 0.0, 0.0]
        t_wall = 0.0
        gc.collect()
        gc.disable()  # (wall-clock loops of 10-20 ms: see timed())
        for k in range(-8, nf):  # 8 untimed warm-up frames
            sc, i = frame_of(max(k, 0), maps[0])
            t1 = time.perf_counter()
            one_frame(one, stream, one_net, one_aux, sc, i, evs)
            (evs[3] if denoise else evs[1]).synchronize()  # Timer::record: the host waits for every frame
            if k >= 0:
                t_wall += time.perf_counter() - t1
                sums[0] += evs[0].elapsed_time(evs[1])
                if denoise:
                    sums[1] += evs[1].elapsed_time(evs[2])
                    sums[2] += evs[2].elapsed_time(evs[3])
        tot = sum(sums)
        seq_last = one.download_image()
        ref_loop = {"batch": 1, "frames": nf, "fps": 1000.0 * nf / tot if tot > 0 else 0.0,
                    "render_ms": sums[0] / nf, "torch_ms": sums[1] / nf, "filter_ms": sums[2] / nf,
                    "wall_fps": nf / t_wall if t_wall > 0 else 0.0,
                    "note": "one rto_launch_renderer (single-frame kernel) + GuidanceNet + filter per frame, host waits for each "
                            "frame like Timer::record (render_context.hpp:179-188); fps = 1000 / (render + torch + filter) from "
                            "the per-frame event pairs, wall_fps = frames / host wall clock of the same loop"}
        # The same per-frame operator calls, software-pipelined: frame k is launched on lane k mod D (its own context and
        # stream) BEFORE the host waits for frame k - D + 1 -- still one launch and one host wait per frame, but the
        # tail of a frame (a handful of long rays on an otherwise empty chip) overlaps the next frames' heads.
        D = max(1, min(8, args.ref_loop_inflight))
        if D > 1:
            plane = [(one, stream, one_net, one_aux)]
            for _ in range(1, D):
                c2 = tune(R.RenderContext(W, H, device=local_rank, frames=1))
                plane.append((c2, side_stream(len(plane) - 1), lane_net(), torch.as_tensor(c2.batch_views()[0], device=dev)))

            def pipelined_pass(cull_single):
                # (the figure an integrator gets from rto_launch_renderer in flight is the DEFAULT tuning's -- the
                #  library's cull_single is off; the pass with the key on is reported beside it, labelled)
                for lc, _, _, _ in plane:
                    lc.set_tuning("cull_single", int(cull_single))
                done = [torch.cuda.Event() for _ in range(D)]
                npipe = max(nf, 4 * D)
                t0p = None
                host_wait = host_issue = 0.0
                for k in range(-2 * D, npipe):
                    if k == 0:
                        torch.cuda.synchronize(dev)
                        t0p = time.perf_counter()
                    ln = k % D
                    tw0 = time.perf_counter()
                    if k >= -D:
                        done[ln].synchronize()  # the host waits for the frame this lane rendered D frames ago
                    tw1 = time.perf_counter()
                    sc, i = frame_of(max(k, 0) % max(nf, 1), maps[0])
                    lc, ls, lnn, la = plane[ln]
                    one_frame(lc, ls, lnn, la, sc, i)
                    done[ln].record(ls)
                    if k >= 0:
                        host_wait += tw1 - tw0
                        host_issue += time.perf_counter() - tw1
                torch.cuda.synchronize(dev)
                wall = time.perf_counter() - t0p
                last_ln = (npipe - 1) % D
                _, i_last = frame_of((npipe - 1) % max(nf, 1), maps[0])
                _, i_seq = frame_of(nf - 1, maps[0])
                same = None
                if i_last == i_seq:
                    same = bool(np.array_equal(plane[last_ln][0].download_image().view(np.uint32), seq_last.view(np.uint32)))
                return npipe, wall, host_issue, host_wait, same

            npipe, wall, host_issue, host_wait, same = pipelined_pass(False)
            _, wall_c, _, _, same_c = pipelined_pass(True)
            ref_loop["pipelined"] = {"frames_in_flight": D, "frames": npipe, "wall_fps": npipe / wall,
                                     "host_issue_ms_per_frame": host_issue / npipe * 1e3, "host_wait_ms_per_frame": host_wait / npipe * 1e3,
                                     "last_frame_bit_identical_to_the_sequential_loop": same,
                                     "tuning": "library defaults (cull_single = 0)",
                                     "wall_fps_with_cull_single": npipe / wall_c,
                                     "last_frame_bit_identical_with_cull_single": same_c,
                                     "note": "same operator calls per frame; lane k mod D = its own context + stream; the host waits for "
                                             "frame k - D before launching frame k.  wall_fps: what an integrator gets with the library's "
                                             "default tuning; wall_fps_with_cull_single: rto_ctx_set_tuning(ctx, 'cull_single', 1) on every "
                                             "context (the single-frame kernel then skips the tiles no culling cell projects into: same pixels)"}
            for c2, _, _, _ in plane[1:]:
                c2.free()
        gc.enable()
        one.free()

    # ---------------- untimed: work units of the same frames -> algorithmic bytes ----------------
    # Two figures (VERDICT r3 task 2).  (i) SURVEY 8d's: every ray, a root-restart walk priced at 4 B per level
    # (rt_core.cuh:241-270 + n3tree_query.hpp:22-47) -- what the reference does, NOT what these kernels do.  (ii) the work the
    # batched path performs: only the rays of the tiles its culling left marked, one top-grid entry (8 B) or one
    # traversal-image word (4 B) per node visit, the thresholds it reads and the hit entries it writes.  Both from the
    # counting instantiation of render_fast (never timed); for (ii) the same frames are first rendered by the batched path
    # and each is counted against its own tile marks.
    ctx.set_kernel(R.KERNEL_FAST)
    ctx.enable_stats(True, marched=True)
    ctx.get_stats(reset=True)
    ctx.get_march_stats(reset=True)
    opt_nd = R.RenderOptions(spp=args.spp, denoise=False)
    count_steps = max(0, min(n_frames, args.count_frames))  # per-frame means need no more
    marked_tiles = all_tiles = 0
    for sc, idx in (plan(count_steps, maps[0]) if count_steps else []):  # same poses, same RNG bases as the timed frames
        ctx.rng_seed()
        R.launch_renderer_batch(trees[sc], [cams[i] for i in idx], opt_nd, ctx, stream, rng_jumps=[WARM_FRAMES_REF + i for i in idx])
        lv, al = ctx.queue_stats()
        marked_tiles += lv
        all_tiles += al
        # the counting kernel shades from dense records: a codebook-direct tree is counted on its
        # expanded twin (same traversal, same hits)
        count_tree = R.N3Tree(paths[sc], device=local_rank) if args.quant_direct else trees[sc]
        for k, i in enumerate(idx):
            ctx.select_frame(k)
            ctx.rng_seed()
            ctx.rng_advance((WARM_FRAMES_REF + i) << 32)
            R.launch_renderer(count_tree, cams[i], opt_nd, ctx, stream)
        if args.quant_direct:
            torch.cuda.synchronize(dev)
            count_tree.free()
    units = ctx.get_stats(reset=True)
    march = ctx.get_march_stats(reset=True)
    ctx.enable_stats(False)
    ctx.select_frame(0)
    counted = count_steps > 0
    count_steps = max(count_steps, 1)  # (--count-frames 0: every unit is 0 and the algorithmic figures are reported as null)
    px = W * H
    alg_bytes_frame = (4 * units["levels"] + 2 * units["steps"] + 2 * (tree.data_dim - 1) * units["hit_leaves"]
                       + 48 * px * count_steps) / count_steps
    alg_bytes_launch = alg_bytes_frame * frames_per_launch
    t_launch = kt["traverse_ms"] * 1e-3
    alg_gbps = alg_bytes_launch / t_launch / 1e9 if t_launch > 0 else 0.0
    # (ii): bytes the traversal kernel itself moves for the marched rays ...
    wide = bool(getattr(tree, "wide_nodes", 0))  # the batched kernel walks the two-level image: one entry per two levels
    m_trav_frame = (8 * march["grid_loads"] + 4 * march["wide_loads" if wide else "node_loads"]        # node visits
                    + 4 * args.spp * march["rays_in_box"]                     # sorted thresholds read back (sample_kernel wrote them)
                    + 4 * march["hit_entries"]                                # hit entries written
                    + 4 * marked_tiles) / count_steps                         # queue list entries
    # ... and of traversal + shading together (the render stage of a frame): + the coefficient record of every hit entry
    # (2 B x 3 x basis), the entry read back, 48 B of aux planes + image per pixel of EVERY tile (culled ones are written too)
    m_render_frame = m_trav_frame + ((2 * (tree.data_dim - 1) + 4) * march["hit_entries"] + 48 * px * count_steps) / count_steps
    m_trav_launch, m_render_launch = m_trav_frame * frames_per_launch, m_render_frame * frames_per_launch
    m_trav_gbps = m_trav_launch / t_launch / 1e9 if t_launch > 0 else 0.0
    t_render = (kt["traverse_ms"] + kt["shade_ms"]) * 1e-3
    m_render_gbps = m_render_launch / t_render / 1e9 if t_render > 0 else 0.0

    # counter passes of THIS workload committed under profiles/ (tools/profile_round.sh); bytes and L1 line
    # accesses scale with the frames of a launch
    traffic = tcp = traffic_src = valu = None
    traffic_stale = None
    code_id = kernel_code_id()
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if wid and os.path.exists(pmc_path):
        try:
            doc = json.load(open(pmc_path))
            pj = doc.get("workloads", {}).get(wid)
            # the counters describe ONE build of the kernel: a run of other code must not wear them (VERDICT r2 task 7)
            traffic_stale = bool(pj) and pj.get("kernel_code_id") != code_id
            if pj and not traffic_stale:
                scale = frames_per_launch / float(pj["frames_per_launch"])
                traffic = (pj["fetch_bytes"] + pj["write_bytes"]) * scale
                traffic_src = "%s; counters of kernel code %s" % (pj.get("source"), pj.get("kernel_code_id"))
                vc = doc.get("valu_ceiling") or {}
                if pj.get("valu_insts") and pj.get("kernel_clocks") and vc.get("traversal_mix_insts_per_clk_per_simd"):
                    simds = float(pj.get("cus", 256)) * 4.0
                    rate = pj["valu_insts"] / simds / pj["kernel_clocks"]
                    ceil = vc.get("ceiling_insts_per_clk_per_simd") or vc["traversal_mix_insts_per_clk_per_simd"]
                    valu = {"wave_insts_per_launch": pj["valu_insts"] * scale,
                            "salu_insts_per_launch": (pj.get("salu_insts") or 0.0) * scale,
                            "insts_per_clk_per_simd": rate,
                            "salu_insts_per_clk_per_simd": (pj.get("salu_insts") or 0.0) / simds / pj["kernel_clocks"],
                            "ceiling_insts_per_clk_per_simd": ceil, "frac": rate / ceil,
                            "full_rate_opcode_ceiling": vc.get("full_rate_insts_per_clk_per_simd"),
                            "half_rate_opcode_ceiling": vc.get("half_rate_insts_per_clk_per_simd"),
                            "wait_any_frac": pj.get("wait_any_frac"), "wait_inst_any_frac": pj.get("wait_inst_any_frac"),
                            "active_inst_any_frac": pj.get("active_inst_any_frac"),
                            "lanes_per_valu_inst": pj.get("lanes_per_valu_inst"),
                            "note": "frac = SQ_INSTS_VALU / (SIMDs x kernel clocks) over the rate the traversal's instruction stream sustains "
                                    "with no memory in the way: the larger of the asm probe's figure for its opcode mix at 8 waves per "
                                    "SIMD (%.3f, profiles/r3_valu_calibration.json, counters on the probe itself) and the traversal "
                                    "loop's own with both gathers stubbed (%.3f, %s). " % (
                                        vc.get("traversal_mix_insts_per_clk_per_simd") or 0.0, vc.get("stubbed_loop_insts_per_clk_per_simd") or 0.0,
                                        vc.get("stubbed_loop_source", "no stubbed-loop pass committed")) +
                                    "A SIMD issues ~0.45 instructions per clock in all: plain add / mul / fma / logic opcodes at "
                                    "0.41-0.45, every other VALU opcode (3-operand, shifts left, min / max, conversions, compares, "
                                    "packed, SGPR operand) at 0.235-0.245, SALU instructions out of the same budget"}
                ce = doc.get("ceilings")
                if pj.get("tcp_line_accesses") and ce:
                    cus = float(pj.get("cus", 256))
                    clk = pj["kernel_clocks"]  # shader clocks of the profiled launch
                    lines = pj["tcp_line_accesses"] / cus
                    l1_miss = pj["tcp_tcc_read_req"] / cus
                    l2_miss = l1_miss * pj["tcc_miss"] / max(pj["tcc_hit"] + pj["tcc_miss"], 1)
                    model_clk = ((lines - l1_miss) / ce["l1_hit_lines_per_clk"] + (l1_miss - l2_miss) / ce["l2_lines_per_clk"]
                                 + l2_miss / ce["mall_lines_per_clk"])
                    ci = ce.get("independent")
                    lower = None
                    if ci:
                        lower = ((lines - l1_miss) / ci["l1_hit_lines_per_clk"] + (l1_miss - l2_miss) / ci["l2_lines_per_clk"]
                                 + l2_miss / ci["mall_lines_per_clk"]) / clk
                    tcp = {"line_accesses_per_clk_per_cu": lines / clk, "l1_hit_rate": 1.0 - l1_miss / lines,
                           "l2_hit_rate": 1.0 - l2_miss / max(l1_miss, 1.0),
                           "ceilings_lines_per_clk_per_cu": ce, "frac": model_clk / clk, "frac_lower": lower,
                           "note": "frac = (L1-hit lines / ceiling + L2-served lines / ceiling + lines from beyond L2 / ceiling) / "
                                   "kernel clocks, at the rates tools/probe_ceiling.py measured for DEPENDENT scattered dword loads, "
                                   "the traversal's shape (profiles/r2_probe_ceiling.json: one gather in flight per wave, so these are "
                                   "latency x concurrency figures -- taken at 6-8 waves per SIMD like the kernel -- not the L1's throughput "
                                   "limit, and the kernel may pass them where its gathers overlap better than the probe's); frac_lower "
                                   "prices the same lines at the rates of four independent gathers in flight per wave."}
        except Exception as e:  # a malformed profile must not break the bench line
            print("[bench] ignoring %s: %r" % (pmc_path, e), file=sys.stderr)
            traffic = tcp = valu = None
    achieved = traffic / t_launch / 1e9 if (traffic and t_launch > 0) else None

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    # STREAM-style copy on this box (report the achieved rate against the measured copy
    # bandwidth as well as against the 8 TB/s peak): 1 GiB device-to-device, read + write counted
    copy_gbps = None
    try:
        a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize(dev)
        copy_gbps = 10 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del a, b
    except Exception:
        copy_gbps = None

    # ---------------- CPU baseline (rank 0, N == 1 only; bounded sample) ----------------
    cpu = None
    cpu_cache = os.path.join("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp", "rto_bench_cpu_baseline_%s.json" % hashlib.sha256(
        repr((W, H, args.spp, args.basis, args.depth, args.shell, args.radius, args.tree, denoise, args.cpu_threads)).encode()).hexdigest()[:16])
    if world > 1 and args.cpu_frames > 0 and os.path.exists(cpu_cache):
        # (VERDICT r5 task 8) an N > 1 line carries the N = 1 run's CPU baseline of the same workload on this box
        try:
            cpu = dict(json.load(open(cpu_cache)), carried_from="the N = 1 run of this workload on this box (%s)" % cpu_cache)
        except Exception:
            cpu = None
    if cpu is None and args.cpu_frames > 0:
        import orc
        if world > 1:
            args.cpu_frames = 1  # (no N = 1 line ran here before: a one-frame sample on rank 0 after the other ranks are done)
        if tree_host is None:
            z = np.load(paths[0])
            child, data, scale, offset = z["child"], z["data"], z["invradius3"], z["offset"]
            fmt = str(z["data_format"])
        else:
            child, data, scale, offset, fmt = tree_host.child, tree_host.data, tree_host.scale, tree_host.offset, tree_host.data_format
        ht = orc.HostTree(child, data, scale, offset, fmt)
        cores = args.cpu_threads or usable_cores()
        oopt = orc.default_options(spp=args.spp, denoise=int(denoise))
        cpu_net = denoiser.GuidanceNetCompact.from_full(full).float() if denoise else None
        # One thread pool at a time: the three legs run one after the other over all sample frames --
        # the oracle's OpenMP team, torch's intra-op pool, the oracle's team again -- each warmed once untimed, so that no
        # leg is timed while the other runtime's idle threads still spin on the same cores or while a pool is being created.
        nf_cpu = args.cpu_frames
        ocams = [orc.camera(W, H, fx, fx, np.ascontiguousarray(poses[s % len(poses)][:3, :4].T, np.float32).reshape(-1))
                 for s in range(nf_cpu)]  # scene 0, poses 0, 1, ...
        bases = [orc.rng(frame=WARM_FRAMES_REF + (s % len(poses))) for s in range(nf_cpu)]
        tiny = orc.camera(64, 64, fx * 64.0 / W, fx * 64.0 / W, np.ascontiguousarray(poses[0][:3, :4].T, np.float32).reshape(-1))
        orc.render_frame(ht, tiny, oopt, bases[0], threads=cores)  # (creates the OpenMP team)
        rendered = []
        cpu_steps = 0
        t1 = time.perf_counter()
        for s in range(nf_cpu):
            aux, rgba, st = orc.render_frame(ht, ocams[s], oopt, bases[s], threads=cores)
            rendered.append((aux, rgba))
            cpu_steps += st["steps"]
        t_render = time.perf_counter() - t1
        t_net = t_filter = 0.0
        net_threads = filter_threads = None
        if denoise:
            x0 = torch.from_numpy(rendered[0][0])[None]
            best = None
            for nt in sorted({cores, max(1, cores // 2), max(1, cores // 4), min(cores, 32)}, reverse=True):
                torch.set_num_threads(nt)  # a 5.9 GFLOP convolution does not scale to every core count: take the fastest pool size
                with torch.no_grad():
                    cpu_net(x0)  # warm-up: primitive creation, the pool's threads
                    t2 = time.perf_counter()
                    cpu_net(x0)
                    dt_ = time.perf_counter() - t2
                if best is None or dt_ < best[0]:
                    best = (dt_, nt)
            net_threads = best[1]
            torch.set_num_threads(net_threads)
            maps_cpu = []
            with torch.no_grad():
                cpu_net(x0)
                t2 = time.perf_counter()
                for aux, _ in rendered:
                    wm, gm = cpu_net(torch.from_numpy(aux)[None])
                    maps_cpu.append((wm[0].numpy(), gm[0].numpy()))
                t_net = time.perf_counter() - t2
            torch.set_num_threads(1)  # park torch's pool before the oracle's team runs again
            filter_threads = min(cores, (H + 3) // 4)
            orc.filter_levels(maps_cpu[0][0], maps_cpu[0][1], rendered[0][1], threads=filter_threads)  # warm-up
            t3 = time.perf_counter()
            for (wm, gm), (_, rgba) in zip(maps_cpu, rendered):
                orc.filter_levels(wm, gm, rgba, threads=filter_threads)
            t_filter = time.perf_counter() - t3
        tc = t_render + t_net + t_filter
        cpu = {"value": nf_cpu / tc, "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "%d of the same %dx%d SPP%d frames (poses 0..%d)%s, CPU oracle with OpenMP over rows; each leg warmed once, "
                         "the legs run one after the other (one thread pool busy at a time)"
                         % (nf_cpu, W, H, args.spp, nf_cpu - 1,
                            " + fp32 PyTorch-CPU GuidanceNet + oracle filter" if denoise else ""),
               "threads_per_leg": {"render": cores, "net": net_threads, "filter": filter_threads},
               "logical_cpus_visible": os.cpu_count(), "cores_note": "cores = min(affinity mask, cgroup CPU quota): what the box grants this process",
               "render_s_per_frame": t_render / nf_cpu, "net_s_per_frame": t_net / nf_cpu,
               "filter_s_per_frame": t_filter / nf_cpu, "steps_per_frame": cpu_steps / nf_cpu}
        if world == 1:
            try:
                with open(cpu_cache + ".tmp", "w") as f:
                    json.dump(cpu, f)
                os.replace(cpu_cache + ".tmp", cpu_cache)
            except OSError:
                pass

    # ---------------- parity spot check (untimed): pixels of the last timed launch group vs the CPU oracle ----------------
    def spot_check(frames_list, what):
        if not frames_list:
            return None
        import ctypes as C

        import orc
        checked = mismatched = hit = 0
        rs = np.random.RandomState(12345)
        for sc, i, aux in frames_list:
            if sc not in spot_trees:
                z = np.load(paths[sc])
                spot_trees[sc] = orc.HostTree(z["child"], z["data"], z["invradius3"], z["offset"], str(z["data_format"]))
            ocam = orc.camera(W, H, fx, fx, np.ascontiguousarray(poses[i][:3, :4].T, np.float32).reshape(-1))
            oopt = orc.default_options(spp=args.spp, denoise=int(denoise))
            base = orc.rng(frame=WARM_FRAMES_REF + i)
            for idx in list(rs.randint(0, W * H, args.spot_pixels)) + [0, W * H - 1, (H // 2) * W + W // 2]:
                a8, px4 = (C.c_float * 8)(), (C.c_float * 4)()
                orc.lib().orc_render_pixel(C.byref(spot_trees[sc].c), C.byref(ocam), C.byref(oopt), C.byref(base), int(idx), a8, px4, None)
                y, x = divmod(int(idx), W)
                same = np.array_equal(np.array(a8[:aux.shape[0]], np.float32).view(np.uint32), np.ascontiguousarray(aux[:, y, x]).view(np.uint32))
                checked += 1
                mismatched += 0 if same else 1
                hit += 1 if a8[3] > 0 else 0
        if mismatched:
            print("[bench] PARITY FAILURE: %d of %d spot pixels differ from the oracle (%s)" % (mismatched, checked, what), file=sys.stderr)
        return {"pixels_checked": checked, "mismatches": mismatched, "pixels_with_hits": hit,
                "frames": [[sc, i] for sc, i, _ in frames_list],
                "values_per_pixel": int(frames_list[0][2].shape[0]),
                "what": what + ": aux planes (fp32 bits; after a lean launch: the 4 stored values = planes 0..3) of random pixels + "
                        "corners + centre of frames of the LAST launch group of that timed pass against oracle/'s render_kernel + "
                        "trace_ray for that pixel (orc_render_pixel); the oracle is the checker here, never the thing measured"}

    spot_trees = {}
    parity = spot_check(spot_frames, "headline pass")
    parity_full = spot_check(spot_frames_full, "full-outputs pass (all 8 planes)")

    # ---------------- PSNR (untimed, pose 0): SPP-6 raw / denoised vs a high-SPP reference ----------------
    psnr = None
    if args.psnr_frames > 0:
        def _psnr(a, b):  # denoiser/metrics.py:61-62 on rgb in [0,1]
            mse = float(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2))
            return float("inf") if mse == 0 else -10.0 * np.log10(mse)
        ctx.select_frame(0)
        ctx.set_kernel(R.KERNEL_FAST)
        acc = np.zeros((H, W, 4), np.float64)
        ref_opt = R.RenderOptions(spp=32, denoise=False)
        for k in range(args.psnr_frames):  # independently SEEDED frames (2^32-strided pcg32 streams are correlated)
            ctx.rng_seed(977 + 7919 * k)
            R.launch_renderer(tree, cams[0], ref_opt, ctx, stream)
            acc += ctx.download_image()
        ref_img = (acc / args.psnr_frames).astype(np.float32)
        ctx.rng_seed()
        R.launch_renderer_batch(tree, [cams[0]], opt, ctx, stream, rng_jumps=[WARM_FRAMES_REF])
        raw = ctx.download_image(noisy=denoise)
        psnr = {"reference": "%d x SPP32 = %d spp, pose 0" % (args.psnr_frames, 32 * args.psnr_frames),
                "raw_spp%d_db" % args.spp: _psnr(raw, ref_img)}
        if denoise:
            with torch.no_grad():
                wm, gm = net(aux_t[:1])
            R.filtering(stream, wm, gm, ctx.noisy_ptr, ctx.image_ptr, mode=R.FILTER_EXACT)
            exact = ctx.download_image()
            exact8 = ctx.download_rgba8()
            psnr["denoised_db"] = _psnr(exact, ref_img)
            R.filtering(stream, wm, gm, ctx.noisy_ptr, ctx.image_ptr, mode=R.FILTER_FAST)
            fast = ctx.download_image()
            fast8 = ctx.download_rgba8()
            psnr["denoised_factorised_filter_db"] = _psnr(fast, ref_img)
            psnr["factorised_vs_exact_filter_db"] = _psnr(fast, exact)
            d8 = fast8.astype(np.int16) - exact8.astype(np.int16)
            psnr["rgba8_bytes_differing_factorised_vs_exact"] = {
                "differing": int(np.count_nonzero(d8)), "of": int(d8.size), "max_abs_step": int(np.abs(d8).max()),
                "note": "(uint8_t)(f * 255) truncates (main_headless.cpp:535-538): the factorised filter's <= 2e-5 relative "
                        "difference steps over an integer boundary in these bytes -- the headline `value` is the tolerance "
                        "route, `value_exact` the bit-exact one"}
            psnr["note"] = ("GuidanceNet trained by tools/train_guidance.py on this synthetic scene (pose 0 held out); "
                            "no ts_*.ts of the reference exists offline" if trained else
                            "GuidanceNet has seeded RANDOM weights: the denoised figure shows the pipeline runs, not denoiser quality")
        psnr["hip_vs_cpu_oracle"] = ("traversal / shading / exact filter: bit-exact against this repository's CPU oracle "
                                     "(tests/), whose estimator semantics are pinned by tests/test_expectation.py; NOT a "
                                     "comparison with frames of the CUDA reference (none exist offline)")

    # without a counter pass for this workload the line falls back to the MARCHED algorithmic figure (bytes the kernel has
    # to move for the work it does: <= what any memory system moved), never to the every-ray one (which may exceed the peak)
    use = achieved if achieved is not None else m_trav_gbps
    if not counted:
        m_trav_launch = m_trav_gbps = m_render_launch = m_render_gbps = alg_bytes_launch = alg_gbps = None
        use = achieved
    frac_of = lambda g: (g / HBM_PEAK_GBS) if g is not None else None
    roof = {
        "kernel": "render_persist<%d>" % args.spp, "bound": "hbm",
        "achieved": use, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": frac_of(use),
        "basis": ("counters: FETCH_SIZE + WRITE_SIZE of this workload (profiles/pmc_traffic.json) / this run's launch duration"
                  if achieved is not None else
                  "ALGORITHMIC bytes of the marched work (no counter pass is committed for this workload): see algorithmic_marched_note"),
        "traffic": traffic, "traffic_source": traffic_src, "traffic_stale": traffic_stale, "kernel_code_id": code_id,
        "algorithmic_marched_bytes": m_trav_launch, "algorithmic_marched_gbps": m_trav_gbps,
        "algorithmic_marched_frac": frac_of(m_trav_gbps),
        "algorithmic_marched_render_bytes": m_render_launch, "algorithmic_marched_render_gbps": m_render_gbps,
        "algorithmic_marched_render_frac": frac_of(m_render_gbps),
        "algorithmic_marched_note": "the work the batched kernels perform, counted on the same frames: rays of the tiles the culling left "
                                    "marked only; per node visit the ONE load render_persist issues (8 B top-grid entry or 4 B traversal-image "
                                    "word); 4 B x SPP thresholds read per marched ray that enters the volume; 4 B per hit entry written; 4 B "
                                    "per queued tile -- per launch, over the traversal kernel's duration.  `_render_`: + the shading kernel's "
                                    "bytes (coefficient record 2 B x 3 x basis + 4 B per hit entry, 48 B of aux planes + image per pixel of "
                                    "every tile) over traversal + shading time.  Cache-served re-reads count (algorithmic, not DRAM)",
        "marched_units_per_frame": dict({k: v / count_steps for k, v in march.items()},
                                        tiles_marked=marked_tiles / count_steps, tiles=all_tiles / count_steps,
                                        traversal_image="two-level (wide_loads)" if wide else "one-level (node_loads)",
                                        loads_per_step=(march["grid_loads"] + march["wide_loads" if wide else "node_loads"]) / max(march["steps"], 1)) if counted else None,
        "survey_8d_every_ray_bytes_per_launch": alg_bytes_launch, "survey_8d_every_ray_gbps": alg_gbps,
        "survey_8d_every_ray_over_peak": frac_of(alg_gbps),
        "survey_8d_note": "root-restart walk, EVERY ray (SURVEY 8d formula: 4 B per level + 2 B per step + SH record per hit leaf + 48 B per "
                          "pixel): the reference's walk priced on this frame.  The kernels here never march the culled rays and skip most "
                          "levels (top grid, ancestor stack), so this is NOT a roofline of the timed kernel and may exceed the peak; kept for "
                          "continuity with rounds 1-3 (`algorithmic_frac` there)",
        "avg_launch_ms": kt["traverse_ms"],
        "avg_launch_ms_source": "HIP events around the kernel on its launch stream, %s" % (
            "single-stream pass (value_single_stream)" if NL > 1 else "the timed pass itself"),
        "measured_copy_bw": copy_gbps,
        "launches": kt["launches"], "frames_per_launch": frames_per_launch,
        "shade_kernel_avg_launch_ms": kt["shade_ms"], "thresholds_kernel_avg_launch_ms": kt["raygen_ms"],
        "tiles_marched_frac": (live_slots / all_slots) if all_slots else None,
        "culling_note": "8x8-pixel tiles that no culling cell of the tree projects into hold only rays that never meet density: they are "
                        "background pixels without marching (bit-identical, tests/test_culling.py); thresholds_kernel_avg_launch_ms "
                        "covers tile marking + queue lists + threshold draws",
        "units_per_frame": {k: v / count_steps for k, v in units.items()} if counted else None,
        "tcp": tcp,
        "valu": valu,
    }
    out = dict(head, value_exact=exact_pass["value"] if exact_pass else None,
               value_full_outputs=full_pass["value"] if full_pass else None, value_single_stream=value_single)
    out["config"] = dict(
        config,
        value_exact=exact_pass["value"] if exact_pass else None,  # the same frames through the bit-exact filter route
        reference_loop_fps=ref_loop["fps"] if ref_loop else None,  # the reference's loop shape: one launch + one host wait per frame
        reference_loop_pipelined_wall_fps=(ref_loop.get("pipelined") or {}).get("wall_fps") if ref_loop else None,
        value_full_outputs=full_pass["value"] if full_pass else None,  # ... storing all 48 B per pixel like volrend.cu:187-212
        value_single_stream=value_single,  # the headline route on ONE stream (the pass the per-kernel durations come from)
        streams_note=("`value`, `value_exact`, `value_full_outputs`: launch groups alternate over %d streams (contexts), the tail of "
                      "one group's kernels overlaps the next group's head; roofline.*_ms and reference_timer: a single-stream "
                      "pass of the same frames (`value_single_stream`)" % NL) if NL > 1 else "one stream",
    )
    out.update({
        "reference_timer": {  # Timer::report formula (render_context.hpp:190-206), rank 0, per frame
            "render_ms": tstats["render_ms"], "torch_ms": tstats["torch_ms"], "filter_ms": tstats["filter_ms"],
            "fps": tstats["fps"], "frames": tstats["frames"]},
        "reference_loop": ref_loop,
        "exact_route": exact_pass,
        "final_gather": gather,
        "parity_spot": parity,
        "parity_spot_full_outputs": parity_full,
        "alt_scene_map": alt,
        "roofline": roof,
        "psnr": psnr,
        "cpu_baseline": cpu,
    })
    emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
