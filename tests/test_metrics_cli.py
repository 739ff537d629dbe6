"""volrend_headless --gt_dir: every rendered pose is scored against its ground-truth PNG (PSNR, SSIM, SMAPE on the float image,
the true image composited over the run's background), the report gains three lines after the five timing lines and -o DIR
gains metrics.json.  One binary run per step; 3 poses at 64 x 48.  (--gpus is not run here -- the suite has one device; the
RANK_METRICS merge is covered on the CPU by tools/sanitize/png_fuzz.cpp through tests/test_png_reader.py.)"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_ref
import rt_octree_amd as R
from rt_octree_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "rt-octree_amd", "bin", "volrend_headless")
W, H, N, WARMUP = 64, 48, 3, 2
TIMING = r"render: [0-9.]+ ms per frame\ntorch:  [0-9.]+ ms per frame\nfilter: [0-9.]+ ms per frame\nall:    [0-9.]+ ms per frame\nFPS:    [0-9.]+\n"


def _run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=600)


def _scene(tmp_path):
    tree = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(N)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    return tp, poses, pp


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _as_dict(m):
    return {"mse": m.mse, "psnr": m.psnr, "smape": m.smape, "ssim": m.ssim}


def _check_report(r, out_dir, want):
    """metrics.json per-pose values against `want` (FrameMetrics per pose, tolerances of tests/test_metrics.py), the printed
    means against the mean of the file's values, the five timing lines in place before them"""
    doc = json.load(open(os.path.join(out_dir, "metrics.json")))
    assert [f["pose"] for f in doc["frames"]] == list(range(N)) and [f["name"] for f in doc["frames"]] == ["r_%d" % i for i in range(N)]
    assert doc["count"] == N
    for i, f in enumerate(doc["frames"]):
        metrics_ref.assert_close(R.FrameMetrics(f["mse"], f["psnr"], f["smape"], f["ssim"]), _as_dict(want[i]), "pose %d" % i)
    m = re.search(TIMING + r"psnr:   ([-0-9.]+)\nssim:   ([-0-9.]+)\nsmape:  ([-0-9.]+)\n", r.stdout)
    assert m, r.stdout
    for k, name in enumerate(("psnr", "ssim", "smape")):
        mean = float(np.mean([f[name] for f in doc["frames"]]))
        assert abs(float(m.group(k + 1)) - mean) < 1e-9, (name, m.group(k + 1), mean)
        assert abs(doc["mean"][name] - mean) < 1e-12


def test_frames_scored_against_their_own_pngs(tmp_path):
    """-o A, then --gt_dir A -o B: the float frames against their own truncated 8-bit PNGs; B/metrics.json equals
    ImageMetrics.compute(float image of the same launch through the Python API, read_png), over the default white"""
    tp, poses, pp = _scene(tmp_path)
    op = synth.write_opt_json(str(tmp_path / "opt.json"), denoise=False, spp=6)
    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    base = [tp, pp, "--options", op, "-w", str(W), "-h", str(H), "--warmup", str(WARMUP)]
    ra = _run(base + ["-o", a])
    assert ra.returncode == 0, ra.stderr
    assert re.search(TIMING, ra.stdout) and "psnr:" not in ra.stdout and not os.path.exists(os.path.join(a, "metrics.json"))
    rb = _run(base + ["-o", b, "--gt_dir", a])
    assert rb.returncode == 0, rb.stderr
    for i in range(N):  # scoring changes no frame
        assert open(os.path.join(a, "r_%d.png" % i), "rb").read() == open(os.path.join(b, "r_%d.png" % i), "rb").read()
    dt = R.N3Tree(tp)
    ctx = R.RenderContext(W, H)
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    opt = R.RenderOptions.from_json(op)
    met = R.ImageMetrics(0)
    want = []
    for i in range(N):
        cam.set_c2w(poses[i])
        ctx.rng_seed()
        ctx.rng_advance((WARMUP + i) << 32)
        R.launch_renderer(dt, cam, opt, ctx)
        truth = R.read_png(os.path.join(a, "r_%d.png" % i))
        assert np.array_equal(truth, ctx.download_rgba8())
        want.append(ctx.metrics(_t(truth[None]), over_background=1.0)[0])
        assert want[-1] == met.compute(_t(ctx.download_image()[None]), _t(truth[None]), over_background=1.0)[0]
        assert all(np.isfinite(v) for v in want[-1]) and want[-1].mse > 0
    _check_report(rb, b, want)
    # the per-frame loop scores the same frames
    c = str(tmp_path / "C")
    rc = _run(base + ["-o", c, "--gt_dir", a, "--batch", "1"])
    assert rc.returncode == 0, rc.stderr
    _check_report(rc, c, want)


def test_ground_truth_with_alpha_is_composited_over_the_runs_background(tmp_path):
    """PNGs with random alpha, written by the test; --bg 0.25 (no --options file: SPP 1, denoise on through the fused network):
    the denoised float image against rgb * a + 0.25 * (1 - a)"""
    import torch
    from PIL import Image
    from rt_octree_amd import denoiser
    tp, poses, pp = _scene(tmp_path)
    tsp = os.path.join(HERE, "golden", "ts_ref_format.ts")
    gt = tmp_path / "gt"
    gt.mkdir()
    rs = np.random.RandomState(17)
    truths = rs.randint(0, 256, (N, H, W, 4)).astype(np.uint8)
    for i in range(N):
        Image.fromarray(truths[i], "RGBA").save(str(gt / ("r_%d.png" % i)))
    out = str(tmp_path / "out")
    r = _run([tp, pp, "--ts_module", tsp, "--bg", "0.25", "-w", str(W), "-h", str(H), "--warmup", str(WARMUP), "--batch", "1", "-o", out,
              "--gt_dir", str(gt)])
    assert r.returncode == 0, r.stderr
    dt = R.N3Tree(tp)
    ctx = R.RenderContext(W, H)
    fx = synth.blender_focal(W)
    cam = R.Camera(W, H, fx, fx)
    opt = R.RenderOptions(spp=1, denoise=True, background_brightness=0.25)
    fused = denoiser.FusedGuidanceNet(torch.jit.load(tsp, map_location="cuda:0"))
    want, white = [], []
    for i in range(N):
        cam.set_c2w(poses[i])
        ctx.rng_seed()
        ctx.rng_advance((WARMUP + i) << 32)
        R.launch_renderer(dt, cam, opt, ctx)
        wm, gm = fused(torch.as_tensor(ctx.aux_view(), device="cuda:0"), squares_implied=True)
        R.filtering(None, wm[0].contiguous(), gm[0].contiguous(), ctx.noisy_ptr, ctx.image_ptr)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "r_%d.png" % i))), ctx.download_rgba8()), i
        want.append(ctx.metrics(_t(truths[i:i + 1]), over_background=0.25)[0])
        white.append(ctx.metrics(_t(truths[i:i + 1]), over_background=1.0)[0])
    _check_report(r, out, want)
    assert all(abs(a.mse - b.mse) > 1e-3 for a, b in zip(want, white))  # (the background matters to these values)


def test_ground_truth_errors_come_before_any_frame(tmp_path):
    from PIL import Image
    tp, poses, pp = _scene(tmp_path)
    op = synth.write_opt_json(str(tmp_path / "opt.json"), denoise=False, spp=6)
    rs = np.random.RandomState(1)

    def gt_dir(name, sizes, sixteen=None):
        d = tmp_path / name
        d.mkdir()
        for i, (w, h) in enumerate(sizes):
            p = str(d / ("r_%d.png" % i))
            if i == sixteen:
                Image.fromarray(rs.randint(0, 65536, (h, w)).astype(np.uint16)).save(p)
            else:
                Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(p)
        return str(d)

    cases = (
        (gt_dir("missing", [(W, H), (W, H)]), "r_2.png", "cannot open"),
        (gt_dir("size", [(W, H), (W + 1, H), (W, H)]), "r_1.png", "65 x 48"),
        (gt_dir("deep", [(W, H), (W, H), (W, H)], sixteen=2), "r_2.png", "bit depth 16"),
    )
    for k, (d, name, word) in enumerate(cases):
        out = str(tmp_path / ("out%d" % k))
        r = _run([tp, pp, "--options", op, "-w", str(W), "-h", str(H), "--warmup", "1", "-o", out, "--gt_dir", d])
        assert r.returncode != 0, r.stdout
        assert name in r.stderr and word in r.stderr, r.stderr
        assert "FPS:" not in r.stdout and not [f for f in os.listdir(out) if f.endswith(".png")], "a frame was rendered"
    r = _run(["--help"])
    assert r.returncode == 0 and "--gt_dir" in r.stdout
