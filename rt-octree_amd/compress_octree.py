"""Octree compression: median-cut quantisation of the SH coefficients + savez_compressed -- the counterpart of the reference's
renderer/scripts/compress_octree.py, with the project's own quantiser (include/rto.h "quantiser") in place of svox's CUDA
extension.  The output opens in volrend and in this project's loader (expanded, or rendered from the codebooks with
quant_direct).

    python -m rt_octree_amd.compress_octree x.npz [y.npz ...] [--noquant] [--bits 16] [--out_dir min_alt] [--overwrite]
                                            [--sigma_thresh 2.0] [--retain 1] [--backend hip|cpu]

Per input: skipped when the output exists (without --overwrite) or when the source already holds quant_colors; svox's
bookkeeping keys parent_depth, geom_resize_fact, n_free, n_internal and depth_limit are dropped; --noquant only re-saves with
deflate (no GPU, no library call).  Otherwise sigma is the last channel of `data` and a slot is live when
sigma > sigma_thresh, compared as torch compares a half tensor with a Python float: the threshold is rounded to fp16 (through
float32, to nearest even; beyond 65504 it becomes an infinity) and the two halves are compared -- so --sigma_thresh 2.0004 keeps
what 2.0 keeps.  Written: `sigma` fp16 [cap,N,N,N], 0 in dead slots; `data_retained` fp16 [retain,cap,N,N,N,3], basis functions
0 .. retain-1, zeros in dead slots; for every other basis function k the [m,3] triples (data[c * basis_dim + k])_c of the live
slots go through the quantiser, `quant_map[k - retain]` (uint16 [cap,N,N,N]) takes the ids (0 in dead slots) and
`quant_colors[k - retain]` (fp16 [65536,3]) the palette; `data` is dropped, every other key passes through.  A tree without live
slots needs no quantiser call: its maps and codebooks are zero.

Deviations from the reference script:
  * the five svox keys are dropped only if present (the reference raises KeyError on a file without them);
  * --weighted is refused with a message (the reference's line 89 cannot run: it calls sigma.float(float32));
  * for --bits < 16 the codebook still has 65536 rows, zero beyond 2^bits: both loaders index the codebooks with a stride of
    65536, so the reference's own 2^bits-row file would be misread.
--backend cpu uses the host twin of the quantiser and never touches a GPU; both backends write the same bytes."""
import argparse
import os
import os.path as osp
import sys

import numpy as np

SVOX_KEYS = ("parent_depth", "geom_resize_fact", "n_free", "n_internal", "depth_limit")
CODEBOOK_ROWS = 65536


def live_slots(sigma, sigma_thresh):
    """sigma: float16 array -> bool array, torch's `half_tensor > python_float` (see the module docstring)."""
    with np.errstate(over="ignore"):
        t = np.float32(sigma_thresh).astype(np.float16)
    return sigma > t


def compress_arrays(z, bits=16, retain=1, sigma_thresh=2.0, backend="hip", quantizer=None):
    """z: the dict of a dense tree.npz -> the dict of the quantised file (see the module docstring).  `quantizer`: a
    rt_octree_amd.Quantizer to reuse with backend "hip"."""
    from .quantize import Quantizer, quantize_median_cut_host
    z = dict(z)
    data = np.ascontiguousarray(z["data"], dtype=np.float16)
    if data.ndim != 5 or data.shape[1] != data.shape[2] or data.shape[2] != data.shape[3] or (data.shape[4] - 1) % 3:
        raise ValueError("data must be [capacity,N,N,N,3 * basis_dim + 1], not %s" % (list(data.shape),))
    if not 1 <= bits <= 16:
        raise ValueError("--bits must be in 1 .. 16, not %d" % bits)
    cap, N, D = data.shape[0], data.shape[1], data.shape[4]
    basis_dim = (D - 1) // 3
    if not 0 <= retain < basis_dim:
        raise ValueError("--retain must be in 0 .. %d (the tree has %d basis functions), not %d" % (basis_dim - 1, basis_dim, retain))
    flat = data.reshape(-1, D)
    sigma = flat[:, D - 1].copy()
    snz = live_slots(sigma, sigma_thresh)
    sigma[~snz] = 0
    live = np.ascontiguousarray(flat[snz, :D - 1].reshape(-1, 3, basis_dim))  # [m, 3, basis_dim]
    m, nq = live.shape[0], basis_dim - retain
    quant_colors = np.zeros((nq, CODEBOOK_ROWS, 3), np.float16)
    quant_map = np.zeros((nq, flat.shape[0]), np.uint16)
    if m:
        own, dev = None, None
        if backend == "hip":
            import torch
            own = quantizer if quantizer is not None else Quantizer(0)
            dev = torch.from_numpy(live).to("cuda:%d" % own.device)
        elif backend != "cpu":
            raise ValueError("backend must be 'hip' or 'cpu', not %r" % (backend,))
        try:
            for j in range(nq):
                k = j + retain
                if dev is not None:
                    pal, ids = own.median_cut(dev[:, :, k].contiguous(), bits)
                    pal, ids = pal.cpu().numpy(), ids.cpu().numpy().view(np.uint16)
                else:
                    pal, ids = quantize_median_cut_host(live[:, :, k], bits)
                quant_colors[j, :1 << bits] = pal
                quant_map[j, snz] = ids
        finally:
            if own is not None and quantizer is None:
                own.free()
    z["quant_colors"] = quant_colors
    z["quant_map"] = quant_map.reshape(nq, cap, N, N, N)
    z["sigma"] = sigma.reshape(cap, N, N, N)
    if retain:
        kept = np.zeros((retain, flat.shape[0], 3), np.float16)
        for k in range(retain):
            kept[k, snz] = live[:, :, k]
        z["data_retained"] = kept.reshape(retain, cap, N, N, N, 3)
    del z["data"]
    return z


def compress_file(src, dst, noquant=False, **kw):
    """One file; -> "written", or "already compressed" when the source holds quant_colors (nothing is written then)."""
    with np.load(src) as f:
        if not noquant and "quant_colors" in f.files:
            return "already compressed"
        z = {k: f[k] for k in f.files}
    for k in SVOX_KEYS:
        z.pop(k, None)
    if not noquant:
        z = compress_arrays(z, **kw)
    np.savez_compressed(dst, **z)
    return "written"


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m rt_octree_amd.compress_octree", description=__doc__.split("\n\n")[0])
    parser.add_argument("input", type=str, nargs="+", help="Input npz(s)")
    parser.add_argument("--noquant", action="store_true", help="Disable quantization")
    parser.add_argument("--bits", type=int, default=16, help="Quantization bits (order)")
    parser.add_argument("--out_dir", type=str, default="min_alt", help="Where to write compressed npz")
    parser.add_argument("--overwrite", action="store_true", help="Overwrite existing compressed npz")
    parser.add_argument("--weighted", action="store_true", help="Weighted median cut: refused (the reference's cannot run)")
    parser.add_argument("--sigma_thresh", type=float, default=2.0, help="Kill voxels under this sigma")
    parser.add_argument("--retain", type=int, default=1,
                        help="Do not compress first x SH coeffs, needed for some scenes to keep good quality. For lego use --retain 4")
    parser.add_argument("--backend", choices=("hip", "cpu"), default="hip", help="The quantiser: HIP kernels or the host twin")
    args = parser.parse_args(argv)
    if args.weighted:
        print("compress_octree: --weighted is not supported (the reference script's weighted path cannot run either)", file=sys.stderr)
        return 2
    os.makedirs(args.out_dir, exist_ok=True)
    print("Quantization disabled, only applying deflate" if args.noquant else "Quantization enabled")
    quantizer = None
    try:
        for fname in args.input:
            fname_c = osp.join(args.out_dir, osp.basename(fname))
            print("Compressing", fname, "to", fname_c)
            if not args.overwrite and osp.exists(fname_c):
                print(" > skip")
                continue
            if args.backend == "hip" and not args.noquant and quantizer is None:
                from .quantize import Quantizer
                quantizer = Quantizer(0)
            try:
                status = compress_file(fname, fname_c, noquant=args.noquant, bits=args.bits, retain=args.retain,
                                       sigma_thresh=args.sigma_thresh, backend=args.backend, quantizer=quantizer) \
                    if not args.noquant else compress_file(fname, fname_c, noquant=True)
            except ValueError as e:
                print("compress_octree: %s: %s" % (fname, e), file=sys.stderr)
                return 2
            if status != "written":
                print(" > skip since source already compressed")
                continue
            print(" > Size", osp.getsize(fname) // (1024 * 1024), "MB ->", osp.getsize(fname_c) // (1024 * 1024), "MB")
    finally:
        if quantizer is not None:
            quantizer.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
