"""The trainer (`python -m rt_octree_amd.train`; rt-octree_amd/train.py): its config reader, chunking and dataset listing on the
CPU, and train / resume / compact / test runs as child processes on the GPU over a small blender-style dataset."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLENDER_TXT = """logs_root = ./logs
exp_name = lego
data_dir = ./data/nerf_synthetic/lego

dataset_type = blender
spp = 6
preload = true
nx = 10
ny = 10

use_wandb = false
i_print = 1
i_save = 100
i_test = 100
save_image = true

lr = 0.0001
epochs = 2000
batch_size = 32

in_channels = 8
mid_channels = 32
num_layers = 2
num_branches = 5
kernel_levels = 4
loss_fn = smape
"""


# ---------------------------------------------------------------- CPU
def test_config_reader_and_defaults(tmp_path):
    from rt_octree_amd import train as T
    cfg = T.read_config(BLENDER_TXT)
    assert cfg["exp_name"] == "lego" and cfg["nx"] == "10" and cfg["preload"] == "true" and cfg["lr"] == "0.0001" and len(cfg) == 22
    assert T.read_config("# note\n\n a = b = c \n") == {"a": "b = c"}
    with pytest.raises(ValueError):
        T.read_config("no equals sign")
    p = tmp_path / "blender.txt"
    p.write_text(BLENDER_TXT)
    a = T.parse_args(["--config", str(p), "--task", "train", "--epochs", "7"])
    assert (a.spp, a.nx, a.ny, a.batch_size, a.mid_channels, a.num_layers, a.num_branches, a.kernel_levels) == (6, 10, 10, 32, 32, 2, 5, 4)
    assert a.preload is True and a.save_image is True and a.use_wandb is False and a.lr == 1e-4 and a.epochs == 7
    assert a.work_dir == os.path.join("./logs", "lego") and a.route in ("fused", "torch") and a.seed == 0
    # the reference's defaults (main.py:64-118) without a config
    d = T.parse_args(["--task", "test", "--exp_name", "x"])
    assert (d.logs_root, d.data_dir, d.dataset_type, d.spp, d.nx, d.ny) == ("../logs/", "../data/nerf_synthetic/lego", "blender", 1, 1, 1)
    assert (d.i_print, d.i_save, d.i_test, d.in_channels, d.mid_channels, d.num_layers, d.num_branches, d.kernel_levels) == (1, 100, 100, 8, 8, 8, 3, 8)
    assert (d.loss_fn, d.lr, d.epochs, d.batch_size, d.preload, d.save_image) == ("smape", 5e-4, 30000, 16, False, False)
    with pytest.raises(SystemExit):
        T.parse_args(["--task", "train", "--exp_name", "x", "--use_wandb"])


def _literal_chunks(nx, ny, aux, img_in, gt):
    """a restatement of dataset.py:88-124 with the ragged chunks left out"""
    H, W = aux.shape[1:]
    dh, dw = H // ny, W // nx
    keep = []
    for j in range(ny):
        for i in range(nx):
            c = gt[j * dh:(j + 1) * dh, i * dw:(i + 1) * dw]
            empty = (c[..., 3] == 0).mean() if c.shape[-1] == 4 else (c[..., :3] == 1).mean()
            if empty < 0.8:
                keep.append((j * dh, i * dw))
    return dh, dw, keep


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("H,W,nx,ny", [(20, 30, 3, 2), (23, 31, 4, 3)])  # the second leaves a remainder both ways
def test_chunks_and_valid_chunk(channels, H, W, nx, ny):
    from rt_octree_amd import train as T
    rs = np.random.RandomState(H + channels)
    aux = rs.rand(8, H, W).astype(np.float32)
    img_in = np.ascontiguousarray(aux[:4].transpose(1, 2, 0))
    gt = rs.rand(H, W, channels).astype(np.float32)
    dh, dw = H // ny, W // nx
    # chunk (0, 0) almost empty; chunk (0, 1) empty in exactly 0.8 of it (dropped: the test is `<`); chunk (1, 0) one value below 0.8
    size = dh * dw * (1 if channels == 4 else 3)
    flat_empty = lambda k: np.arange(size) < k  # noqa: E731

    def blank(y0, x0, k):
        view = gt[y0:y0 + dh, x0:x0 + dw]
        m = flat_empty(k).reshape(view.shape[:2] if channels == 4 else view.shape)
        if channels == 4:
            view[..., 3][m] = 0
        else:
            view[m] = 1

    blank(0, 0, size - 1)
    k80 = int(np.ceil(0.8 * size))
    blank(0, dw, k80)
    blank(dh, 0, k80 - 1)
    a, i, g = T.slice_chunks(nx, ny, aux, img_in, gt)
    _dh, _dw, keep = _literal_chunks(nx, ny, aux, img_in, gt)
    assert (_dh, _dw) == (dh, dw)
    assert len(a) == len(keep) and (0, 0) not in keep and (dh, 0) in keep
    assert ((0, dw) in keep) == (k80 / size < 0.8) and len(keep) >= nx * ny - 2
    for (y, x), ca, ci, cg in zip(keep, a, i, g):
        assert ca.shape == (8, dh, dw) and ci.shape == (dh, dw, 4) and cg.shape == (dh, dw, channels)
        assert np.array_equal(ca, aux[:, y:y + dh, x:x + dw]) and np.array_equal(ci, img_in[y:y + dh, x:x + dw])
        assert np.array_equal(cg, gt[y:y + dh, x:x + dw])
    assert T.valid_chunk(gt[dh:2 * dh, :dw]) and not T.valid_chunk(gt[:dh, :dw])


def test_valid_chunk_exactly_at_the_limit():
    from rt_octree_amd import train as T
    c = np.full((5, 10, 4), 0.5, np.float32)
    c.reshape(-1, 4)[:40, 3] = 0  # 40 of 50: exactly 0.8
    assert not T.valid_chunk(c)
    c.reshape(-1, 4)[39, 3] = 0.5
    assert T.valid_chunk(c)
    r = np.full((5, 10, 3), 0.5, np.float32)
    r.reshape(-1)[:120] = 1  # 120 of 150
    assert not T.valid_chunk(r)
    r.reshape(-1)[0] = 0.5
    assert T.valid_chunk(r)


def test_white_composite():
    from rt_octree_amd import train as T
    png = np.random.RandomState(2).randint(0, 256, (6, 7, 4)).astype(np.uint8)
    png[0, 0, 3], png[0, 1, 3] = 0, 255
    out = T.composite_white(png, True)
    f = png.astype(np.float32) / 255.0
    ref = f[..., :3] * f[..., 3:] + 1 * (1 - f[..., 3:])
    assert out.dtype == np.float32 and out.shape == (6, 7, 4)
    assert np.array_equal(out[..., :3], ref) and np.array_equal(out[..., 3], f[..., 3])
    assert np.all(out[0, 0, :3] == 1) and np.array_equal(out[0, 1, :3], f[0, 1, :3])
    rgb = T.composite_white(png, False)
    assert rgb.shape == (6, 7, 3) and np.array_equal(rgb, f[..., :3])


def test_dataset_layouts(tmp_path):
    from rt_octree_amd import train as T
    b = tmp_path / "blender"
    b.mkdir()
    (b / "transforms_train.json").write_text(json.dumps({"frames": [{"file_path": "./train/r_10"}, {"file_path": "./train/r_2"}]}))
    (b / "transforms_test.json").write_text(json.dumps({"frames": [{"file_path": "./test/r_0"}]}))
    got = T.list_frames(str(b), "blender", "train", 6)
    assert got == [("r_10", str(b / "spp_6" / "train" / "buf_r_10.bin"), str(b / "train" / "r_10.png")),
                   ("r_2", str(b / "spp_6" / "train" / "buf_r_2.bin"), str(b / "train" / "r_2.png"))]
    assert T.list_frames(str(b), "blender", "test", 1) == [("r_0", str(b / "spp_1" / "test" / "buf_r_0.bin"), str(b / "test" / "r_0.png"))]
    t = tmp_path / "tt"
    (t / "rgb").mkdir(parents=True)
    for n in ("1_b.png", "0_b.png", "0_a.png", "1_a.png"):
        (t / "rgb" / n).write_bytes(b"")
    assert [f[0] for f in T.list_frames(str(t), "tt", "train", 2)] == ["0_a", "0_b"]
    assert T.list_frames(str(t), "tt", "test", 2)[1] == ("1_b", str(t / "spp_2" / "buf_1_b.bin"), str(t / "rgb" / "1_b.png"))
    ll = tmp_path / "llff"
    (ll / "images_4").mkdir(parents=True)
    for i in range(17):
        (ll / "images_4" / ("img%02d.png" % i)).write_bytes(b"")
    assert [f[0] for f in T.list_frames(str(ll), "llff", "test", 1)] == ["img00", "img08", "img16"]
    tr = T.list_frames(str(ll), "llff", "train", 1)
    assert len(tr) == 14 and tr[0] == ("img01", str(ll / "spp_1" / "buf_img01.bin"), str(ll / "images_4" / "img01.png"))


def test_short_buffer_is_named(tmp_path):
    from rt_octree_amd import train as T
    p = tmp_path / "buf_r_0.bin"
    np.zeros(8 * 6 * 5 - 1, np.float32).tofile(p)
    with pytest.raises(ValueError, match="buf_r_0.bin"):
        T.load_buffer(str(p), 6, 5)
    with pytest.raises(ValueError, match="buf_r_0.bin"):
        T.check_buffers([("r_0", str(p), "x.png")], lambda png: (5, 6))
    np.zeros(8 * 6 * 5, np.float32).tofile(p)
    assert T.load_buffer(str(p), 6, 5).shape == (8, 6, 5)
    T.check_buffers([("r_0", str(p), "x.png")], lambda png: (5, 6))


# ---------------------------------------------------------------- GPU
H, W = 48, 64


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("lego")
    rs = np.random.RandomState(11)
    for split, count in (("train", 3), ("test", 2)):
        (d / split).mkdir()
        (d / "spp_2" / split).mkdir(parents=True)
        frames = []
        for i in range(count):
            name = "r_%d" % i
            frames.append({"file_path": "./%s/%s" % (split, name)})
            yy, xx = np.mgrid[0:H, 0:W]
            clean = np.stack([0.5 + 0.4 * np.sin(xx / (5.0 + i)), 0.5 + 0.4 * np.cos(yy / 7.0), (xx + yy) / float(H + W), np.ones((H, W))], -1)
            clean[:6, :, 3] = 0  # some background
            Image.fromarray((clean * 255).astype(np.uint8), "RGBA").save(d / split / (name + ".png"))
            over = clean[..., :3] * clean[..., 3:] + (1 - clean[..., 3:])
            noisy = np.concatenate([over + 0.1 * rs.randn(H, W, 3), clean[..., 3:]], -1).astype(np.float32).transpose(2, 0, 1)
            np.concatenate([noisy, noisy * noisy], 0).astype(np.float32).tofile(d / "spp_2" / split / ("buf_%s.bin" % name))
        (d / ("transforms_%s.json" % split)).write_text(json.dumps({"frames": frames}))
    return d


def run(dataset, logs, exp, *extra, timeout=120):
    cmd = [sys.executable, "-m", "rt_octree_amd.train", "--logs_root", str(logs), "--exp_name", exp, "--data_dir", str(dataset),
           "--spp", "2", "--mid_channels", "32", "--num_layers", "2", "--num_branches", "5", "--kernel_levels", "4", "--lr", "1e-3",
           "--preload"] + list(extra)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


TRAIN = ("--task", "train", "--nx", "2", "--ny", "2", "--batch_size", "4", "--i_save", "1", "--route", "fused")


@pytest.mark.gpu
def test_train_compact_test(dataset, tmp_path):
    import torch
    from rt_octree_amd import ImageMetrics, denoiser, read_png
    from rt_octree_amd import train as T
    out = run(dataset, tmp_path, "a", *TRAIN, "--epochs", "3")
    assert "train/loss" in out and "test/psnr" in out
    work = tmp_path / "a"
    ckpt = torch.load(work / "checkpoint_000003.tar", map_location="cpu", weights_only=False)
    assert set(ckpt) == {"epoch", "model", "optimizer", "lr_scheduler"} and ckpt["epoch"] == 4
    dn = denoiser.Denoiser(str(work / "ts_000003.ts"), fused=True)
    assert (dn.fused.c1, dn.fused.levels, dn.fused.num_layers) == (32, 4, 2)

    run(dataset, tmp_path, "a", "--task", "compact")
    model = denoiser.GuidanceNet(8, 32, 5, 2, 4)
    model.load_state_dict(ckpt["model"])
    compact = denoiser.GuidanceNetCompact.from_full(model).half()
    ts = torch.jit.load(str(work / "ts_latest.ts"), map_location="cpu")
    consts = denoiser.FusedGuidanceNet.graph_conv_constants(ts) or [(ts.state_dict()["layers.%d.conv.weight" % i], ts.state_dict()["layers.%d.conv.bias" % i]) for i in range(2)]
    for (w, b), blk in zip(consts, compact.layers):
        assert torch.equal(w.cpu(), blk.conv.weight) and torch.equal(b.cpu(), blk.conv.bias)

    out = run(dataset, tmp_path, "a", "--task", "test", "--save_image")
    log = json.loads([ln for ln in out.splitlines() if "test/psnr" in ln][-1].replace("===== ", ""))
    rec = json.loads((work / "test" / "metrics.json").read_text())
    assert all(abs(log["test/" + k] - rec["mean"][k]) < 1e-12 for k in ("psnr", "ssim", "smape")) and len(rec["frames"]) == 2
    # the frames again, from the module it wrote: the same network, filter and metrics
    args = T.parse_args(["--task", "test", "--exp_name", "a", "--data_dir", str(dataset), "--spp", "2"])
    aux, img_in, gt, names = T.load_split(args, "test")
    net = denoiser.FusedGuidanceNet(torch.jit.load(str(work / "ts_latest.ts"), map_location="cuda:0"))
    metrics = ImageMetrics(0)
    for i, frame in enumerate(rec["frames"]):
        wm, gm = net(torch.from_numpy(np.ascontiguousarray(aux[i]))[None].cuda())
        img = denoiser.filtering_autograd(wm, gm, torch.from_numpy(img_in[i])[None].cuda())
        m = metrics.compute(img, torch.from_numpy(gt[i])[None].cuda())[0]
        assert frame["name"] == names[i]
        assert abs(m.psnr - frame["psnr"]) <= 1e-9 and abs(m.ssim - frame["ssim"]) <= 1e-9 and abs(m.smape - frame["smape"]) <= 1e-9
        img[..., 3] = 1
        u8 = (img[0] * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy()
        assert np.array_equal(read_png(str(work / "test" / ("r_%d.png" % i))), u8)


@pytest.mark.gpu
def test_resumed_run_equals_uninterrupted_run(dataset, tmp_path):
    import torch
    run(dataset, tmp_path, "whole", *TRAIN, "--epochs", "4")
    # (two epochs of the SAME command: the schedule 0.1 ** (epoch / (epochs + 1)) makes `--epochs 2` no prefix of `--epochs 4`)
    run(dataset, tmp_path, "parts", *TRAIN, "--epochs", "4", "--stop_after", "2")
    assert not os.path.exists(tmp_path / "parts" / "checkpoint_000003.tar")
    out = run(dataset, tmp_path, "parts", *TRAIN, "--epochs", "4")
    assert "Load checkpoint from" in out and "checkpoint_000002.tar" in out
    a = torch.load(tmp_path / "whole" / "checkpoint_000004.tar", map_location="cpu", weights_only=False)["model"]
    b = torch.load(tmp_path / "parts" / "checkpoint_000004.tar", map_location="cpu", weights_only=False)["model"]
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.gpu
def test_torch_route_runs(dataset, tmp_path):
    out = run(dataset, tmp_path, "t", "--task", "train", "--nx", "2", "--ny", "2", "--batch_size", "4", "--i_save", "1", "--route", "torch",
              "--epochs", "1")
    assert "train/loss" in out and os.path.exists(tmp_path / "t" / "checkpoint_000001.tar")
