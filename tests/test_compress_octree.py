"""python -m rt_octree_amd.compress_octree with the host twin (--backend cpu; no GPU is touched): every array of the written file
against the numpy builder of tests/quantize_ref.py, the reference script's skip / overwrite / --noquant behaviour, the three
stated deviations, and the file through the host loader."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import quantize_ref
import rt_octree_amd as R
from rt_octree_amd import _lib, compress_octree

THRESH = "20.004"  # rounds to the half 20.0 as torch's comparison does; the synthetic sigmas spread over 5 .. 300


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    path = str(d / "tree.npz")
    return path, quantize_ref.write_dense_tree(path)


def _run(capsys, *argv):
    rc = compress_octree.main(list(argv))
    out = capsys.readouterr()
    return rc, out.out, out.err


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _assert_files_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), k


def _probe(path):
    buf = C.create_string_buffer(4096)
    _lib.check(R.lib().rto_tree_probe_npz(os.fsencode(path), buf, 4096))
    return json.loads(buf.value.decode())


def test_written_file_equals_the_model_and_loads(dense, tmp_path, capsys):
    src, z = dense
    out_dir = str(tmp_path / "min_alt")
    args = [src, "--backend", "cpu", "--retain", "2", "--sigma_thresh", THRESH, "--out_dir", out_dir]
    rc, out, _ = _run(capsys, *args)
    dst = os.path.join(out_dir, "tree.npz")
    assert rc == 0 and "Quantization enabled" in out and "Compressing %s to %s" % (src, dst) in out
    assert " > Size %d MB -> %d MB" % (os.path.getsize(src) >> 20, os.path.getsize(dst) >> 20) in out
    got = _load(dst)
    want = quantize_ref.expected_file(z, bits=16, retain=2, sigma_thresh=float(THRESH))
    _assert_files_equal(got, want)
    assert not set(quantize_ref.SVOX_KEYS) & set(got) and "data" not in got
    live = z["data"][..., -1] > np.float16(20.0)
    assert 0 < live.sum() < (z["data"][..., -1] > 0).sum()  # the threshold cuts through the tree's sigmas
    assert np.array_equal(got["sigma"] != 0, live)
    assert got["quant_map"].dtype == np.uint16 and got["quant_map"].shape == (7,) + z["child"].shape
    assert got["quant_colors"].shape == (7, 65536, 3) and got["data_retained"].shape == (2,) + z["child"].shape + (3,)
    assert not got["quant_map"][:, ~live].any() and not got["data_retained"][:, ~live].any()
    # the host loader expands it to what the arrays say
    info = _probe(dst)
    assert info["quantized"] == 1 and info["data_format"] == "SH9" and info["capacity"] == z["child"].shape[0]
    assert info["data_fnv1a64"] == quantize_ref.fnv1a64(quantize_ref.decoded(got).tobytes())
    # a second run skips and leaves the file alone; --overwrite writes it again
    stamp = os.stat(dst).st_mtime_ns
    os.utime(dst, ns=(stamp - 10 ** 10, stamp - 10 ** 10))
    rc, out, _ = _run(capsys, *args)
    assert rc == 0 and " > skip\n" in out and os.stat(dst).st_mtime_ns == stamp - 10 ** 10
    rc, out, _ = _run(capsys, *args, "--overwrite")
    assert rc == 0 and " > Size" in out and os.stat(dst).st_mtime_ns > stamp - 10 ** 10
    _assert_files_equal(_load(dst), want)
    # a source that is already quantised is skipped
    again = str(tmp_path / "again")
    rc, out, _ = _run(capsys, dst, "--backend", "cpu", "--out_dir", again)
    assert rc == 0 and "skip since source already compressed" in out and not os.path.exists(os.path.join(again, "tree.npz"))


def test_noquant_only_deflates(dense, tmp_path, capsys):
    src, z = dense
    out_dir = str(tmp_path / "nq")
    rc, out, _ = _run(capsys, src, "--noquant", "--out_dir", out_dir)
    assert rc == 0 and "Quantization disabled, only applying deflate" in out
    dst = os.path.join(out_dir, "tree.npz")
    got = _load(dst)
    _assert_files_equal(got, {k: v for k, v in z.items() if k not in quantize_ref.SVOX_KEYS})
    assert os.path.getsize(dst) < os.path.getsize(src)


def test_keys_are_dropped_only_if_present(tmp_path, capsys):
    src = str(tmp_path / "plain.npz")
    z = quantize_ref.write_dense_tree(src, depth_limit=3, basis_dim=4, seed=3)
    for k in quantize_ref.SVOX_KEYS:
        del z[k]
    np.savez(src, **z)
    out_dir = str(tmp_path / "o")
    rc, _, _ = _run(capsys, src, "--backend", "cpu", "--out_dir", out_dir, "--sigma_thresh", "0")
    assert rc == 0
    _assert_files_equal(_load(os.path.join(out_dir, "plain.npz")), quantize_ref.expected_file(z, 16, 1, 0.0))


def test_weighted_is_refused(dense, tmp_path, capsys):
    rc, _, err = _run(capsys, dense[0], "--weighted", "--backend", "cpu", "--out_dir", str(tmp_path / "w"))
    assert rc != 0 and "--weighted is not supported" in err and not os.path.exists(str(tmp_path / "w" / "tree.npz"))


def test_fewer_bits_keep_the_codebook_stride(dense, tmp_path, capsys):
    src, z = dense
    out_dir = str(tmp_path / "b8")
    rc, _, _ = _run(capsys, src, "--backend", "cpu", "--bits", "8", "--retain", "7", "--sigma_thresh", THRESH, "--out_dir", out_dir)
    assert rc == 0
    got = _load(os.path.join(out_dir, "tree.npz"))
    assert got["quant_colors"].shape == (2, 65536, 3) and not got["quant_colors"][:, 256:].any() and got["quant_colors"][:, :256].any()
    assert got["quant_map"].max() == 255
    _assert_files_equal(got, quantize_ref.expected_file(z, bits=8, retain=7, sigma_thresh=float(THRESH)))
    info = _probe(os.path.join(out_dir, "tree.npz"))
    assert info["data_fnv1a64"] == quantize_ref.fnv1a64(quantize_ref.decoded(got).tobytes())


def test_a_threshold_above_every_sigma_gives_zero_maps(dense, tmp_path, capsys):
    src, z = dense
    out_dir = str(tmp_path / "dead")
    rc, _, _ = _run(capsys, src, "--backend", "cpu", "--sigma_thresh", "1e9", "--out_dir", out_dir)
    assert rc == 0
    got = _load(os.path.join(out_dir, "tree.npz"))
    for k in ("quant_map", "quant_colors", "sigma", "data_retained"):
        assert not got[k].any(), k
    assert got["quant_map"].shape == (8,) + z["child"].shape
    _assert_files_equal(got, quantize_ref.expected_file(z, 16, 1, 1e9))


def test_the_sigma_comparison_is_torch_half_against_float():
    import torch
    sig = np.array([1.999, 2.0, 2.002, 65504.0, 0.0], np.float16)
    for t in (2.0, 2.0004, 2.0009, 2.001, 1.9996, 1.9994, 65519.0, 65520.0, 1e9, -1e9, 0.0):
        want = (torch.from_numpy(sig) > t).numpy()
        assert np.array_equal(compress_octree.live_slots(sig, t), want), t
