"""Exports a trained GuidanceNet state_dict (default: the committed rt-octree_amd/weights/guidance_synth_lego.pt)
as the TorchScript module volrend_headless loads with --ts_module -- the reference's own artefact
(denoiser/network.py:170-208 compact_and_compile: fold the branches, cast to fp16, jit.trace).
usage: python tools/export_ts.py [weights.pt] [out.ts] [--mid-channels C] [--layers N] [--levels L]
(needs a HIP device: the fp16 module is traced on it; the shape options are those the weights were trained with,
tools/train_guidance.py)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rt_octree_amd import denoiser  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("weights", nargs="?", default=os.path.join(ROOT, "rt-octree_amd", "weights", "guidance_synth_lego.pt"))
    ap.add_argument("out", nargs="?", default="ts_latest.ts")
    ap.add_argument("--mid-channels", type=int, default=32)
    ap.add_argument("--layers", type=int, default=2, choices=[2, 3])
    ap.add_argument("--levels", type=int, default=4, choices=[1, 2, 3, 4, 5, 6])
    args = ap.parse_args()
    wpath, out = args.weights, args.out
    model = denoiser.GuidanceNet(8, args.mid_channels, 5, args.layers, args.levels)
    model.load_state_dict(torch.load(wpath, map_location="cpu"))
    dev = "cuda:0" if torch.cuda.is_available() else None
    ts = denoiser.compact_and_compile(model, device=dev, example_hw=(800, 800))
    ts.save(out)
    print("wrote", out, "(fp16, traced on %s)" % dev if dev else "(fp32, CPU)")


if __name__ == "__main__":
    main()
