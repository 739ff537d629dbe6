"""The HIP median cut (rto_quantize_median_cut, csrc/quantize_kernels.hip) against the host twin and the numpy model of
tests/quantize_ref.py, ids and palette bit for bit (the definition leaves no freedom, so there is no tolerance), and the
compress_octree command on the device against itself on the host.

Shapes: the host tests' list (all of it runs in one workgroup's LDS from round 0, or after a few grid-wide rounds: m = 65537,
70000); m = 300001 (round 0 spans 147 tiles of one box, the tie rank crosses them; the boxes drop to 1024 rows after 9 grid-wide
rounds); m = 40000 at 16 bits (most final boxes hold 0 or 1 rows); and the sizes at which the code changes path: 1023 / 1024
rows (1024: the largest box one workgroup takes whole), 1025 (one grid-wide round first), 2047 .. 2049 and 4097 (one, two and three
tiles per box, the spare tile of a short box), and few bits on many rows (the rounds end while the boxes are still big)."""
import numpy as np
import pytest

import quantize_ref
import rt_octree_amd as R
from rt_octree_amd import compress_octree, quantize, synth

from helpers import assert_bits_equal, cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def quantizer():
    q = R.Quantizer(0)
    yield q
    q.free()


def _dev(rows):
    import torch
    return torch.from_numpy(np.array(rows, dtype=np.float16, order="C", copy=True)).to("cuda:0")


def _run(q, rows, bits, stream=None):
    pal, ids = q.median_cut(_dev(rows), bits, stream)
    return pal.cpu().numpy(), ids.cpu().numpy().view(np.uint16)


_big = {}


def big_case(name):
    """(rows, bits, palette, ids): the large inputs, expected values from the host twin, which the host tests hold to the model"""
    if name not in _big:
        build, bits = {
            "normal_m300001": (lambda: quantize_ref.normal_rows(300001, 31), 16),
            "four_values_m300001": (lambda: quantize_ref.four_value_rows(300001, 37), 16),
            "normal_m40000": (lambda: quantize_ref.normal_rows(40000, 41), 16),
            "four_values_m300001_bits3": (lambda: quantize_ref.four_value_rows(300001, 43), 3),
            "normal_m300001_bits9": (lambda: quantize_ref.normal_rows(300001, 47), 9),
        }[name]
        rows = build()
        pal, ids = quantize.quantize_median_cut(rows, bits, backend="cpu")
        _big[name] = (rows, bits, pal, ids)
    return _big[name]


@pytest.mark.parametrize("name", sorted(quantize_ref.CASES))
def test_kernels_equal_model_and_host_twin(quantizer, name):
    rows, bits, pal, ids = quantize_ref.case(name)
    got_pal, got_ids = _run(quantizer, rows, bits)
    quantize_ref.assert_same(got_pal, got_ids, pal, ids, name + " vs model")
    host_pal, host_ids = quantize.quantize_median_cut(rows, bits, backend="cpu")
    quantize_ref.assert_same(got_pal, got_ids, host_pal, host_ids, name + " vs host twin")


@pytest.mark.parametrize("name", ["normal_m300001", "four_values_m300001", "normal_m40000", "four_values_m300001_bits3",
                                  "normal_m300001_bits9"])
def test_large_inputs_equal_the_host_twin(quantizer, name):
    rows, bits, pal, ids = big_case(name)
    got_pal, got_ids = _run(quantizer, rows, bits)
    quantize_ref.assert_same(got_pal, got_ids, pal, ids, name)
    if name == "normal_m40000":
        cnt = np.bincount(got_ids, minlength=65536)
        assert cnt.max() == 1 and (cnt == 0).sum() == 65536 - 40000
        assert not got_pal[cnt == 0].view(np.uint16).any()  # an empty box is +0


def test_the_model_agrees_on_one_large_input(quantizer):
    rows, bits, pal, ids = big_case("four_values_m300001")
    want_pal, want_ids = quantize_ref.median_cut(rows, bits)
    quantize_ref.assert_same(pal, ids, want_pal, want_ids, "host twin vs model")
    cnt = np.bincount(ids, minlength=65536)
    assert cnt.min() == 4 and cnt.max() == 5


@pytest.mark.parametrize("m,bits", [(1023, 16), (1024, 16), (1025, 16), (2047, 12), (2048, 12), (2049, 12), (4097, 13), (1025, 1),
                                    (5000, 2)])
@pytest.mark.parametrize("kind", ["normal", "four_values"])
def test_path_thresholds(quantizer, m, bits, kind):
    rows = (quantize_ref.normal_rows if kind == "normal" else quantize_ref.four_value_rows)(m, 1000 + m)
    want_pal, want_ids = quantize_ref.median_cut(rows, bits)
    got_pal, got_ids = _run(quantizer, rows, bits)
    quantize_ref.assert_same(got_pal, got_ids, want_pal, want_ids, "m=%d bits=%d %s" % (m, bits, kind))


def test_one_handle_reuses_its_scratch():
    q = R.Quantizer(0)
    try:
        rows, bits, pal, ids = big_case("normal_m300001")
        first = _run(q, rows, bits)
        quantize_ref.assert_same(first[0], first[1], pal, ids, "first")
        small, sbits, spal, sids = quantize_ref.case("normal_m65")
        got = _run(q, small, sbits)
        quantize_ref.assert_same(got[0], got[1], spal, sids, "m=65 after m=300001")
        again = _run(q, rows, bits)
        quantize_ref.assert_same(again[0], again[1], first[0], first[1], "third call")
    finally:
        q.free()


def test_two_runs_are_bit_identical_and_streams_agree(quantizer):
    import torch
    rows, bits, pal, ids = big_case("four_values_m300001")
    a = _run(quantizer, rows, bits)
    b = _run(quantizer, rows, bits)
    quantize_ref.assert_same(b[0], b[1], a[0], a[1], "second run")
    s = torch.cuda.Stream()
    dev = _dev(rows)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        p, i = quantizer.median_cut(dev, bits, s)
    s.synchronize()
    quantize_ref.assert_same(p.cpu().numpy(), i.cpu().numpy(), pal, ids, "non-default stream")


def test_refusals(quantizer):
    import ctypes as C
    import torch
    L = R.lib()
    rows = quantize_ref.normal_rows(100, 3)
    dev = _dev(rows)
    pal = torch.zeros((65536, 3), dtype=torch.float16, device="cuda:0")
    ids = torch.full((100,), 7, dtype=torch.int16, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(*args):
        rc = L.rto_quantize_median_cut(quantizer._h, None, *args)
        msg = L.rto_last_error().decode()
        assert rc == -1 and msg, (rc, msg)
        return msg

    assert "rows is not memory" in refused(C.c_void_p(rows.ctypes.data), 100, 16, P(pal), P(ids))  # a host pointer, before launch
    host_ids = np.zeros(100, np.uint16)
    assert "ids is not memory" in refused(P(dev), 100, 16, P(pal), C.c_void_p(host_ids.ctypes.data))
    assert "null" in refused(None, 100, 16, P(pal), P(ids))
    assert "m must be" in refused(P(dev), 0, 16, P(pal), P(ids))
    assert "bits must be" in refused(P(dev), 100, 0, P(pal), P(ids))
    assert "bits must be" in refused(P(dev), 100, 17, P(pal), P(ids))
    torch.cuda.synchronize()
    assert (ids == 7).all()  # nothing was enqueued
    for bad in (np.nan, np.inf):
        r = rows.copy()
        r[63, 1] = bad
        assert "NaN" in refused(P(_dev(r)), 100, 16, P(pal), P(ids))
    with pytest.raises(R.RtoError):
        R.quantize_median_cut(r, 16, backend="hip", quantizer=quantizer)
    got = R.quantize_median_cut(rows, 16, backend="hip", quantizer=quantizer)  # the handle is fine afterwards
    want = quantize_ref.median_cut(rows, 16)
    quantize_ref.assert_same(got[0], got[1], want[0], want[1], "after the refusals")


def test_compress_octree_on_the_device_writes_the_host_file_and_renders(tmp_path, capsys):
    src = str(tmp_path / "tree.npz")
    quantize_ref.write_dense_tree(src)
    common = [src, "--retain", "2", "--sigma_thresh", "20.004"]
    assert compress_octree.main(common + ["--backend", "cpu", "--out_dir", str(tmp_path / "cpu")]) == 0
    assert compress_octree.main(common + ["--backend", "hip", "--out_dir", str(tmp_path / "hip")]) == 0
    capsys.readouterr()
    with np.load(str(tmp_path / "cpu" / "tree.npz")) as a, np.load(str(tmp_path / "hip" / "tree.npz")) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    path = str(tmp_path / "hip" / "tree.npz")
    W = H = 64
    _, cam = cameras(W, H, synth.orbit_poses(8)[1])
    opt = R.RenderOptions(spp=4, denoise=False)
    images = []
    for direct in (False, True):
        tree = R.N3Tree(path, quant_direct=direct)
        ctx = R.RenderContext(W, H)
        R.launch_renderer_batch(tree, [cam], opt, ctx, rng_jumps=[3])
        images.append((ctx.download_aux(), ctx.download_image()))
    assert_bits_equal(images[0][0], images[1][0], "aux")
    assert_bits_equal(images[0][1], images[1][1], "image")
    assert images[0][1][..., :3].std() > 0.01  # something was drawn
