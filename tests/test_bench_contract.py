"""bench.py prints ONE JSON line with the driver's contract keys (run here on a tiny workload)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--batch", "4", "--groups-per-step", "1", "--size", "160",
           "--depth", "6", "--cpu-frames", "1", "--psnr-frames", "2", "--ref-loop-frames", "4", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["value"] > 0
    # value = frames / elapsed, ms_per_step = elapsed / steps, one step = one batch of 4 frames
    assert abs(d["ms_per_step"] * d["value"] - 4000.0) < 4.0 and d["config"]["frames_per_step"] == 4 and d["config"]["frames_timed"] == 24
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["traffic"] is None and "ALGORITHMIC" in rf["basis"]  # counter passes exist for the BASELINE workloads only
    for k in ("algorithmic_marched_gbps", "algorithmic_marched_frac", "algorithmic_marched_render_frac", "survey_8d_every_ray_gbps",
              "avg_launch_ms", "frames_per_launch", "tcp"):
        assert k in rf, k
    # VERDICT r3 task 2: a roofline fraction describes the work the timed kernel does, so it cannot exceed 1; without a
    # counter pass the line falls back to the MARCHED figure (never to the every-ray root-restart one, which may)
    assert 0 < rf["frac"] <= 1 and 0 < rf["algorithmic_marched_frac"] <= 1 and 0 < rf["algorithmic_marched_render_frac"] <= 1
    assert abs(rf["achieved"] - rf["algorithmic_marched_gbps"]) < 1e-9 * rf["achieved"]
    mu, eu = rf["marched_units_per_frame"], rf["units_per_frame"]
    assert 0 < mu["rays"] <= eu["rays"] and 0 < mu["steps"] <= eu["steps"] and mu["hit_entries"] == eu["hit_leaves"]
    assert mu["tiles_marked"] <= mu["tiles"] and 1.0 <= mu["loads_per_step"] < 4.0
    assert mu["grid_loads"] + mu["node_loads"] < eu["levels"]  # fewer loads than a root-restart walk has levels
    assert d["config"]["frames_per_launch"] == rf["frames_per_launch"] == 4.0  # the actual value
    rl = d["reference_loop"]
    assert rl["batch"] == 1 and rl["fps"] > 0 and rl["render_ms"] > 0 and rl["fps"] < d["reference_timer"]["fps"] * 1.5
    assert d["psnr"]["factorised_vs_exact_filter_db"] > 100.0
    # round 3: the line checks itself -- spot pixels of the last timed group against the oracle, the bit-exact route
    # timed beside the headline, the RGBA8 bytes by which the two differ, the reference loop pipelined
    ps = d["parity_spot"]
    assert ps["pixels_checked"] >= 3 * 64 and ps["mismatches"] == 0 and ps["pixels_with_hits"] > 0
    assert d["value_exact"] > 0 and d["exact_route"]["value"] == d["value_exact"] and d["value_exact"] < d["value"] * 1.2
    b8 = d["psnr"]["rgba8_bytes_differing_factorised_vs_exact"]
    assert b8["of"] == 160 * 160 * 4 and b8["max_abs_step"] <= 1 and b8["differing"] < b8["of"] // 100
    # round 5 (VERDICT r4 task 4): config says which clause `value` claims and carries the figures of the other routes; the timed
    # launches are lean (16 instead of 48 bytes stored per pixel), the spot check then compares the 4 stored values
    cf = d["config"]
    assert "TOLERANCE route" in cf["value_route"] and "bit-exact" in cf["value_route"]
    assert cf["value_exact"] == d["value_exact"] and cf["reference_loop_fps"] == rl["fps"]
    assert cf["reference_loop_pipelined_wall_fps"] == rl["pipelined"]["wall_fps"] and cf["groups_per_step"] == 1 and cf["frames_per_group"] == 4
    assert cf["lean_outputs"] is True and ps["values_per_pixel"] == 4 and cf["lean_level"] == 2
    # round 6 (VERDICT r5 task 4): the headline passes run over two streams, the per-kernel durations come from a
    # single-stream pass; the full-output figure (48 B per pixel, like volrend.cu:187-212) and an 8-plane spot check beside it
    assert cf["streams"] == 2 and "single-stream" in cf["streams_note"] and "single-stream" in rf["avg_launch_ms_source"]
    assert d["value_single_stream"] > 0 and d["value_full_outputs"] > 0 and cf["value_full_outputs"] == d["value_full_outputs"]
    pf = d["parity_spot_full_outputs"]
    assert pf["values_per_pixel"] == 8 and pf["pixels_checked"] >= 3 * 64 and pf["mismatches"] == 0
    pl = rl["pipelined"]
    assert pl["frames_in_flight"] == 4 and pl["wall_fps"] > 0 and pl["last_frame_bit_identical_to_the_sequential_loop"] in (True, None)
    assert rf["traffic_stale"] is None and len(rf["kernel_code_id"]) == 16
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_its_outputs(tmp_path):
    """without --full the line holds the headline only (no pass of its own beside the timed one), and --dump-outputs writes
    the frames of the last timed step -- float .npy files under 64 MB -- bit for bit the same from run to run"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--groups-per-step", "2",
           "--size", "96", "--depth", "5"]
    dumps = []
    for k in range(2):
        out_dir = tmp_path / ("run%d" % k)
        r = subprocess.run(cmd + ["--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
            assert key in d, key
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["value"] > 0
        assert abs(d["ms_per_step"] * d["value"] - 8000.0) < 8.0 and d["config"]["frames_timed"] == 24 and d["config"]["full"] is False
        for key in ("roofline", "cpu_baseline", "parity_spot", "reference_loop", "psnr", "value_exact", "value_single_stream"):
            assert key not in d, key
        files = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
        assert set(files) == {"images_sampled.npy", "sample_pixels.npy", "sample_frames.npy", "image_last.npy"}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        img, pix, fr, last = (files[f] for f in ("images_sampled.npy", "sample_pixels.npy", "sample_frames.npy", "image_last.npy"))
        # the last step = frames 16..23 (two launch groups of 4 on the two lanes), each at the same 8192 pixels
        assert img.shape == (8, 8192, 4) and fr.tolist() == [[0.0, float(p)] for p in range(16, 24)] and last.shape == (96, 96, 4)
        assert np.array_equal(last.reshape(-1, 4)[pix.astype(np.int64)], img[-1]) and np.isfinite(img).all() and np.any(img != 0)
        dumps.append(files)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f].view(np.uint8), dumps[1][f].view(np.uint8)), f


def test_counter_based_roofline_for_the_baseline_workloads():
    """profiles/pmc_traffic.json (what bench.py reads for `roofline.achieved`): counter passes for c2 / c5 / c4 and the
    gather ceilings; the counter-based HBM fraction of the default workload is far below the algorithmic one."""
    doc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    assert set(doc["workloads"]) >= {"c2", "c5", "c4"}
    for w in doc["workloads"].values():
        for k in ("frames_per_launch", "fetch_bytes", "write_bytes", "tcp_line_accesses", "tcp_tcc_read_req", "tcc_hit",
                  "tcc_miss", "kernel_clocks"):
            assert w[k] > 0, k
    ce = doc["ceilings"]
    assert 0 < ce["mall_lines_per_clk"] < ce["l2_lines_per_clk"] < ce["l1_hit_lines_per_clk"] < 4
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args([])
    assert bench.workload_id(args, 800, 800) == "c2"
    assert bench.workload_id(bench.parse_args(["--spp", "1", "--no-denoise"]), 800, 800) == "c5"
    assert bench.workload_id(bench.parse_args(["--c4"]), 1920, 1080) == "c4"
    assert bench.workload_id(bench.parse_args(["--shuffle-nodes", "1"]), 800, 800) is None
    # counters describe ONE build of the kernel on ONE default configuration: development runs never wear them
    assert bench.workload_id(bench.parse_args(["--tuning", "refill=816"]), 800, 800) is None
    assert bench.workload_id(bench.parse_args(["--streams", "1"]), 800, 800) == "c2"  # (durations come from the single-stream pass either way)
    os.environ["RTO_LIB"] = "/nonexistent/librto.so"
    try:
        assert bench.workload_id(args, 800, 800) is None
    finally:
        del os.environ["RTO_LIB"]
    for w in doc["workloads"].values():  # tied to the code they were measured on, with the real frames per launch
        assert len(w["kernel_code_id"]) == 16 and w["frames_per_launch"] == 100
    assert 0.2 < doc["valu_ceiling"]["traversal_mix_insts_per_clk_per_simd"] < 0.5
    assert len(bench.kernel_code_id()) == 16


@pytest.mark.gpu
def test_bench_scenes_mode_reports_both_mappings():
    """config C3 shape on a tiny workload: 2 scenes, both rank mappings timed, groups never mix scenes"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "12", "--warmup", "2", "--batch", "4", "--groups-per-step", "1", "--size", "128",
           "--depth", "5", "--cpu-frames", "0", "--psnr-frames", "0", "--ref-loop-frames", "0", "--scenes", "2",
           "--scene-map", "both"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["scenes"] == 2 and d["config"]["scene_map"] == "pose" and d["value"] > 0
    assert d["alt_scene_map"]["scene_map"] == "scene" and d["alt_scene_map"]["value"] > 0
    assert "2 scenes" in d["config"]["workload"]


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu_over_gloo():
    """the driver's torchrun line with two ranks (both on GPU 0, gloo instead of RCCL: RCCL refuses two ranks on one
    device): rank / pose bookkeeping, the barrier + max-reduction of the elapsed time, one JSON line from rank 0 with
    the whole-job frame count."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4", "--groups-per-step", "1",
           "--size", "128", "--depth", "5", "--cpu-frames", "0", "--psnr-frames", "0", "--ref-loop-frames", "2", "--full"]
    env = dict(os.environ, RTO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["frames_timed"] == 24 and d["value"] > 0
    assert d["cpu_baseline"] is None  # N == 1 only
    assert d["parity_spot"]["mismatches"] == 0 and d["parity_spot"]["pixels_checked"] > 0  # rank 0 checks its frames at any N
    # the one collective of the path ran: 2 frames per rank gathered to rank 0, and the frame rank 1 rendered equals the
    # one rank 0 renders itself (images do not depend on N)
    fg = d["final_gather"]
    assert fg["frames"] == 4 and fg["bytes"] == 4 * 128 * 128 * 4 and fg["frame_of_rank_1_rendered_on_rank_0_is_identical"] is True


def test_bench_gpus_n_without_a_launcher_starts_its_own_ranks():
    """VERDICT r3 task 1: `bench.py --gpus 2` started the way the driver starts `--gpus 1` (no torchrun, WORLD_SIZE unset)
    must run TWO ranks -- as a child torch.distributed.run, before torch is imported here -- not one rank that prints
    n_gpus 1.  CPU form: --plan-only (gloo, no GPU)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plan-only", "--steps", "2", "--batch", "4", "--groups-per-step", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "starting 2 ranks as a child process" in r.stderr
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["world"] == 2 and len(d["plans"]["pose"]) == 2
    assert d["plans"]["pose"][0][0][1] == [0, 2, 4, 6] and d["plans"]["pose"][1][0][1] == [1, 3, 5, 7]


@pytest.mark.parametrize("ws", ["1", "4"])
def test_bench_refuses_a_launcher_whose_world_size_differs_from_gpus(ws):
    env = dict(os.environ, WORLD_SIZE=ws, RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plan-only"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "does not match WORLD_SIZE" in r.stderr and not r.stdout.strip()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--plan-only"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(env, WORLD_SIZE="2"))
    assert r.returncode != 0 and "does not match WORLD_SIZE" in r.stderr


@pytest.mark.gpu
def test_bench_gpus_2_without_torchrun_measures_two_ranks():
    """the same on the GPU box: no launcher, two ranks sharing its one GPU over gloo (RCCL wants one device per rank; with
    the default backend and fewer GPUs than ranks the ranks refuse instead of measuring a flat curve)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RTO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4", "--groups-per-step", "1",
           "--size", "128", "--depth", "5", "--cpu-frames", "0", "--psnr-frames", "0", "--ref-loop-frames", "0", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world"] == 2 and d["config"]["frames_timed"] == 24
    assert d["config"]["backend"] == "gloo" and "bench.py itself" in d["config"]["launcher"]
    assert d["final_gather"]["world"] == 2 and d["final_gather"]["backend"] == "gloo"
    assert d["final_gather"]["frame_of_rank_1_rendered_on_rank_0_is_identical"] is True
    import torch
    if torch.cuda.device_count() < 2:  # default backend (RCCL) with more ranks than GPUs: refused, never a silent 1-rank line
        env.pop("RTO_BENCH_BACKEND")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode != 0 and "one rank per GPU" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]
