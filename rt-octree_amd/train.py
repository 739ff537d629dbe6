"""Trains, tests and compacts a GuidanceNet on a dataset of noisy buffers: `python -m rt_octree_amd.train`.

The reference's trainer (paths relative to the reference's root), restated over this package's pieces:
    denoiser/main.py:64-126      the command line and its defaults; the config file (`key = value` text, configs/blender.txt)
    denoiser/dataset.py:71-105   preprocess (/255, composite over white) and slice_imgs / valid_chunk (tolerance 0.8)
    denoiser/dataset.py:137-300  the blender / tt / llff file layouts
    denoiser/runner.py:11-175    Adam + LambdaLR, the epoch loop, checkpoints, compact, the test loop
    denoiser/utils.py:13-28      the newest checkpoint_<epoch>.tar of the work directory resumes the run

Workflow: render `buf_<name>.bin` with the headless renderer's --write_buffer, `--task train`, `--task compact` (ts_latest.ts),
render with --ts_module.

Deviations (DESIGN.md "Deviations"): the image size comes from each PNG, not from a constant per dataset type; ragged remainder
chunks are dropped; `--route fused` (float32 HIP training kernels, no loss scaler) or `--route torch` (autocast + GradScaler
stepping the optimiser); `--stop_after E` ends a run after epoch E as an interruption would (the learning-rate schedule depends on
--epochs, so a run with fewer --epochs is not the beginning of a longer one); the order of the chunks in epoch e depends on
(--seed, e) alone, so a resumed run repeats an uninterrupted one; psnr / ssim / smape come from the device metrics
(ImageMetrics), LPIPS and wandb are not available.
The chunk, composite and listing functions are plain numpy / os code: the CPU suite tests them."""
import argparse
import copy
import json
import os
import sys

import numpy as np

TOLERANCE = 0.8  # dataset.py:97

# main.py:64-118: name -> (type, default); booleans are store_true flags there
OPTIONS = {
    "task": (str, None), "logs_root": (str, "../logs/"), "exp_name": (str, None), "data_dir": (str, "../data/nerf_synthetic/lego"),
    "dataset_type": (str, "blender"), "spp": (int, 1), "preload": (bool, False), "nx": (int, 1), "ny": (int, 1),
    "use_wandb": (bool, False), "i_print": (int, 1), "i_save": (int, 100), "i_test": (int, 100), "save_image": (bool, False),
    "in_channels": (int, 8), "mid_channels": (int, 8), "num_layers": (int, 8), "num_branches": (int, 3), "kernel_levels": (int, 8),
    "loss_fn": (str, "smape"), "lr": (float, 5e-4), "epochs": (int, 30000), "batch_size": (int, 16),
    "route": (str, None), "seed": (int, 0), "stop_after": (int, 0),
}
# which route a run takes when --route is not given: DESIGN.md 7i holds the measurement this follows
DEFAULT_ROUTE = "fused"


def read_config(text):
    """the reference's config text: `key = value` lines, blank lines and # comments -> {key: str}"""
    out = {}
    for no, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if "=" not in line:
            raise ValueError("config line %d is not `key = value`: %r" % (no, line))
        k, v = line.split("=", 1)
        out[k.strip().lstrip("-")] = v.strip()
    return out


def _to_bool(v):
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("true", "1", "yes"):
        return True
    if str(v).lower() in ("false", "0", "no"):
        return False
    raise ValueError("not a boolean: %r" % (v,))


def parse_args(argv=None):
    """the reference's flags with the reference's defaults; a config file sets defaults that the command line overrides"""
    ap = argparse.ArgumentParser(prog="python -m rt_octree_amd.train", description=__doc__.split("\n")[0])
    ap.add_argument("--config", help="config file path")
    for k, (ty, _d) in OPTIONS.items():
        if ty is bool:
            ap.add_argument("--" + k, action="store_true", default=None)
        elif k == "task":
            ap.add_argument("--task", choices=["train", "test", "compact"], default=None)
        elif k == "route":
            ap.add_argument("--route", choices=["fused", "torch"], default=None)
        else:
            ap.add_argument("--" + k, type=ty, default=None)
    ns = ap.parse_args(argv)
    cfg = {}
    if ns.config:
        with open(ns.config) as f:
            cfg = read_config(f.read())
        unknown = sorted(set(cfg) - set(OPTIONS))
        if unknown:
            ap.error("unknown keys in %s: %s" % (ns.config, ", ".join(unknown)))
    for k, (ty, d) in OPTIONS.items():
        v = getattr(ns, k)
        if v is None and k in cfg:
            v = _to_bool(cfg[k]) if ty is bool else ty(cfg[k])
        if v is None:
            v = d
        setattr(ns, k, v)
    if ns.route is None:
        ns.route = DEFAULT_ROUTE
    if ns.use_wandb and ns.task == "train":  # (main.py:122-123 drops the flag for the other tasks)
        ap.error("--use_wandb: wandb is not available here")
    ns.use_wandb = False
    if ns.task is None or ns.exp_name is None:
        ap.error("--task and --exp_name are required")
    if ns.dataset_type not in ("blender", "tt", "llff"):
        ap.error("Invalid dataset type: %s." % ns.dataset_type)
    ns.work_dir = os.path.join(ns.logs_root, ns.exp_name)
    return ns


# ---------------------------------------------------------------- dataset (numpy / os only)
def composite_white(png, has_alpha):
    """dataset.py:75-84: uint8 [H,W,4] -> float32 [H,W,4 or 3]; with alpha, rgb = rgb * a + 1 * (1 - a) in float32"""
    img = png.astype(np.float32) / 255.0
    if not has_alpha:
        return img[..., :3]
    alpha = img[..., -1:]
    img[..., :3] = img[..., :3] * alpha + 1 * (1 - alpha)
    return img


def valid_chunk(gt_chunk):
    """dataset.py:96-105: a chunk is kept when less than 0.8 of it is empty -- alpha == 0 for an RGBA truth, values == 1 for RGB"""
    if gt_chunk.shape[-1] == 4:
        alpha = gt_chunk[..., -1]
        percentage = np.sum(alpha == 0) / alpha.size
    else:
        rgb = gt_chunk[..., :3]
        percentage = np.sum(rgb == 1) / rgb.size
    return percentage < TOLERANCE


def slice_chunks(nx, ny, aux, img_in, img_gt):
    """dataset.py:88-124: ny x nx chunks of H // ny x W // nx, the valid ones, row by row.  The remainder rows and columns of a
    size that does not divide are dropped (the reference cuts ragged chunks there and then fails to stack them)."""
    H, W = aux.shape[1], aux.shape[2]
    dh, dw = H // ny, W // nx
    if dh < 1 or dw < 1:
        raise ValueError("%d x %d chunks of a %d x %d image" % (ny, nx, H, W))
    out = ([], [], [])
    for h in range(0, dh * ny, dh):
        for w in range(0, dw * nx, dw):
            gt = img_gt[h:h + dh, w:w + dw]
            if not valid_chunk(gt):
                continue
            out[0].append(aux[..., h:h + dh, w:w + dw])
            out[1].append(img_in[h:h + dh, w:w + dw])
            out[2].append(gt)
    return out


def list_frames(data_dir, dataset_type, split, spp):
    """[(name, buffer path, PNG path)] of a split, in the reference's order (dataset.py:137-300)"""
    buf = os.path.join(data_dir, "spp_%d" % spp)
    if dataset_type == "blender":
        with open(os.path.join(data_dir, "transforms_%s.json" % split)) as fp:
            meta = json.load(fp)
        names = [os.path.basename(f["file_path"]) for f in meta["frames"]]
        return [(n, os.path.join(buf, split, "buf_" + n + ".bin"), os.path.join(data_dir, split, n + ".png")) for n in names]
    if dataset_type == "tt":
        files = sorted(os.listdir(os.path.join(data_dir, "rgb")))
        files = [x for x in files if x.startswith("0_" if split == "train" else "1_")]
        img_dir = os.path.join(data_dir, "rgb")
    elif dataset_type == "llff":
        img_dir = os.path.join(data_dir, "images_4")
        files = sorted(os.listdir(img_dir))
        test = set(range(0, len(files), 8))
        files = [f for i, f in enumerate(files) if (i in test) == (split == "test")]
    else:
        raise NotImplementedError("Invalid dataset type: %s." % dataset_type)
    out = []
    for f in files:
        n = f.split(".")[0]
        # (tt reads rgb/<name>.png, llff the listed file itself: dataset.py:218-219, 279-280)
        out.append((n, os.path.join(buf, "buf_" + n + ".bin"), os.path.join(img_dir, n + ".png" if dataset_type == "tt" else f)))
    return out


def png_has_alpha(path):
    """the colour type of the IHDR chunk: 6 = RGBA, 2 = RGB (read_png widens both to four channels)"""
    with open(path, "rb") as f:
        head = f.read(26)
    return len(head) == 26 and head[25] == 6


def load_buffer(path, H, W):
    """a --write_buffer file: float32 [8][H][W]; any other size is an error that names the file"""
    want, have = 8 * H * W * 4, os.path.getsize(path)
    if have != want:
        raise ValueError("%s holds %d bytes, not the 8 x %d x %d x 4 = %d of its %d x %d image" % (path, have, H, W, want, W, H))
    return np.fromfile(path, dtype=np.float32).reshape(8, H, W)


def check_buffers(frames, size_of):
    """every buffer of `frames` against its PNG's size (size_of(png) -> (W, H)), before anything is loaded"""
    for _n, b, p in frames:
        W, H = size_of(p)
        if not os.path.exists(b):
            raise FileNotFoundError("%s is missing (render it with --write_buffer)" % b)
        if os.path.getsize(b) != 8 * H * W * 4:
            load_buffer(b, H, W)  # raises with the file's name


def load_split(args, split):
    """(aux [k][8,h,w], img_in [k][h,w,4], img_gt [k][h,w,3 or 4], names): chunks for "train", whole frames for "test" """
    import ctypes as C

    from ._lib import check, lib
    from .metrics import read_png

    def size_of(p):
        w, h = C.c_int(0), C.c_int(0)
        check(lib().rto_image_read_png(str(p).encode(), C.byref(w), C.byref(h), None, 0))
        return w.value, h.value

    frames = list_frames(args.data_dir, args.dataset_type, split, args.spp)
    if not frames:
        raise ValueError("no %s frames under %s" % (split, args.data_dir))
    check_buffers(frames, size_of)
    aux_l, in_l, gt_l, names = [], [], [], []
    for name, b, p in frames:
        png = read_png(p)
        H, W = png.shape[:2]
        aux = load_buffer(b, H, W)[:args.in_channels]
        gt = composite_white(png, png_has_alpha(p))
        img_in = np.ascontiguousarray(aux[:4].transpose(1, 2, 0))  # dataset.py:79
        if split == "train":
            a, i, g = slice_chunks(args.nx, args.ny, aux, img_in, gt)
        else:
            a, i, g = [aux], [img_in], [gt]
        aux_l += a
        in_l += i
        gt_l += g
        names += [name] * len(a)
    if not aux_l:
        raise ValueError("no valid %s chunk under %s" % (split, args.data_dir))
    return aux_l, in_l, gt_l, names


# ---------------------------------------------------------------- runner
def newest_checkpoint(work_dir):
    """utils.py:13-28"""
    best, path = -1, None
    for f in os.listdir(work_dir) if os.path.isdir(work_dir) else []:
        if f.startswith("checkpoint_"):
            num = int(f.split("_")[1].split(".")[0])
            if num > best:
                best, path = num, os.path.join(work_dir, f)
    return path


def say(s):
    print("===== %s" % s, flush=True)  # base_logger.py:14-18


class Runner:
    def __init__(self, args, device):
        import torch
        self.args, self.device, self.epoch = args, device, 0
        self.torch = torch

    def to_device(self, arrays, rgb4=False):
        torch = self.torch
        ts = []
        for a in arrays:
            t = torch.from_numpy(np.ascontiguousarray(a))
            if rgb4 and t.shape[-1] == 3:  # an RGB truth: the kernels take four components, alpha is not measured
                t = torch.cat([t, torch.ones_like(t[..., :1])], -1)
            ts.append(t)
        out = torch.stack(ts)
        return out.to(self.device) if self.args.preload else out

    def loss(self, out, gt):
        from . import denoiser
        if self.args.route == "fused":
            return denoiser.image_loss(out, gt, self.args.loss_fn)
        if self.args.loss_fn == "smape":  # metrics.py:7-9
            p, t = out[..., :3], gt[..., :3]
            return ((p - t).abs() / (p.abs() + t.abs() + 1e-5)).mean()
        if self.args.loss_fn == "mse":
            return ((out[..., :3] - gt[..., :3]) ** 2).mean()
        return denoiser.image_loss(out, gt, self.args.loss_fn)  # huber, or the refusal of LPIPS

    def train(self, model):
        torch, args = self.torch, self.args
        from . import denoiser
        aux, img_in, img_gt, _ = load_split(args, "train")
        aux, img_in, img_gt = self.to_device(aux), self.to_device(img_in), self.to_device(img_gt, rgb4=True)
        self.test_data = load_split(args, "test")
        say("Dataset loaded: %d training chunks of %d x %d, %d test frames" % (len(aux), aux.shape[3], aux.shape[2], len(self.test_data[0])))
        opt = torch.optim.Adam(model.parameters(), lr=args.lr, betas=(0.9, 0.999), weight_decay=5e-4)  # runner.py:19-22
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.1 ** min(epoch / (args.epochs + 1), 1))
        scaler = torch.amp.GradScaler("cuda") if args.route == "torch" else None
        start = 1
        path = newest_checkpoint(args.work_dir)
        if path is not None:
            say("Load checkpoint from %s" % path)
            ckpt = torch.load(path, map_location=self.device, weights_only=False)
            model.load_state_dict(ckpt["model"])
            opt.load_state_dict(ckpt["optimizer"])
            sched.load_state_dict(ckpt["lr_scheduler"])
            start = ckpt["epoch"]
        else:
            say("No checkpoint found")
        n = len(aux)
        for epoch in range(start, args.epochs + 1):
            self.epoch = epoch
            order = np.random.RandomState([args.seed, epoch]).permutation(n)  # a function of (seed, epoch) alone
            total, batches = 0.0, 0
            for b0 in range(0, n, args.batch_size):
                idx = torch.from_numpy(order[b0:b0 + args.batch_size])
                a, x, g = (t[idx.to(t.device)].to(self.device) for t in (aux, img_in, img_gt))
                opt.zero_grad(set_to_none=True)
                out = denoiser.filtering(model, a, x, requires_grad=True, fused=args.route == "fused")
                loss = self.loss(out, g)
                if scaler is None:
                    loss.backward()
                    opt.step()
                else:
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                total += float(loss.detach())
                batches += 1
            sched.step()
            if epoch % args.i_print == 0:
                say(json.dumps({"epoch": epoch, "train/loss": total / batches, "train/lr": opt.param_groups[0]["lr"]}))
            if epoch % args.i_save == 0:
                self.compact(model, load_ckpt=False, filename="ts_%06d.ts" % epoch)
                path = os.path.join(args.work_dir, "checkpoint_%06d.tar" % epoch)
                torch.save({"epoch": epoch + 1, "model": model.state_dict(), "optimizer": opt.state_dict(),
                            "lr_scheduler": sched.state_dict()}, path)
                say("Save checkpoint at %s" % path)
            if start < epoch < args.epochs and epoch % args.i_test == 0:
                say("Testing at epoch %d..." % epoch)
                self.test(model, load_ckpt=False, save_dirname="test_%06d" % epoch)
            if args.stop_after and epoch >= args.stop_after and epoch < args.epochs:
                say("Stopping after epoch %d of %d (--stop_after)" % (epoch, args.epochs))
                return
        say("Test after training")
        self.test(model, load_ckpt=False)

    def load_latest(self, model):
        path = newest_checkpoint(self.args.work_dir)
        if path is None:
            say("No checkpoint found.")
            return False
        say("Load checkpoint from %s" % path)
        model.load_state_dict(self.torch.load(path, map_location="cpu", weights_only=False)["model"])
        return True

    def compact(self, model, load_ckpt=True, filename="ts_latest.ts"):
        """runner.py:162-175"""
        from . import denoiser
        if load_ckpt and not self.load_latest(model):
            return None
        ts = denoiser.compact_and_compile(copy.deepcopy(model), self.device)  # (a copy: it moves its model to the CPU and sets eval)
        if filename:
            self.torch.jit.save(ts, os.path.join(self.args.work_dir, filename))
        return ts

    def test(self, model, load_ckpt=True, save_dirname="test"):
        """runner.py:112-160: the compacted net through FusedGuidanceNet + the filter; psnr / ssim / smape per frame"""
        torch, args = self.torch, self.args
        from . import denoiser
        from ._lib import check, lib
        from .metrics import ImageMetrics
        if load_ckpt and not self.load_latest(model):
            return None
        data = getattr(self, "test_data", None) or load_split(args, "test")
        save_dir = os.path.join(args.work_dir, save_dirname)
        os.makedirs(save_dir, exist_ok=True)
        ts = self.compact(model, load_ckpt=False, filename="")
        net = denoiser.FusedGuidanceNet(ts, device=self.device.index or 0)
        metrics = ImageMetrics(self.device.index or 0)
        frames, total = [], 0.0
        with torch.no_grad():
            for i, (aux, img_in, gt, name) in enumerate(zip(*data)):
                aux_t = torch.from_numpy(np.ascontiguousarray(aux))[None].to(self.device)
                in_t = torch.from_numpy(img_in)[None].to(self.device)
                gt_t = self.to_device([gt], rgb4=True).to(self.device)
                wm, gm = net(aux_t)
                out = denoiser.filtering_autograd(wm, gm, in_t)
                total += float(self.loss(out, gt_t))
                m = metrics.compute(out, gt_t)[0]
                frames.append({"name": name, "psnr": m.psnr, "ssim": m.ssim, "smape": m.smape})
                if args.save_image:  # runner.py:147-149; the 8-bit conversion of torchvision.utils.save_image
                    out[..., -1:] = 1
                    u8 = (out[0] * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy()
                    check(lib().rto_image_write_png(os.path.join(save_dir, "r_%d.png" % i).encode(), u8.ctypes.data, u8.shape[1], u8.shape[0]))
        mean = {k: float(np.mean([f[k] for f in frames])) for k in ("psnr", "ssim", "smape")}
        log = {"epoch": self.epoch, "test/loss": total / len(frames), **{"test/" + k: v for k, v in mean.items()}}
        say(json.dumps(log))
        with open(os.path.join(save_dir, "metrics.json"), "w") as f:
            json.dump({"epoch": self.epoch, "loss": total / len(frames), "mean": mean, "frames": frames}, f, indent=2)
        return mean


def main(argv=None):
    args = parse_args(argv)
    import torch

    from . import denoiser
    if not torch.cuda.is_available():
        raise SystemExit("CPU-only not supported.")  # main.py:20
    if args.loss_fn in ("lpips_alex", "lpips_vgg"):
        raise SystemExit("loss '%s' needs the LPIPS network weights, which this package does not ship" % args.loss_fn)
    device = torch.device("cuda", 0)
    os.makedirs(args.work_dir, exist_ok=True)
    with open(os.path.join(args.work_dir, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=2)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)  # utils.py:6-11
    model = denoiser.GuidanceNet(args.in_channels, args.mid_channels, args.num_branches, args.num_layers, args.kernel_levels)
    runner = Runner(args, device)
    if args.task == "compact":
        runner.compact(model)
        return 0
    model = model.to(device)
    if args.task == "train":
        runner.train(model)
    else:
        runner.test(model)
    return 0


if __name__ == "__main__":
    sys.exit(main())
