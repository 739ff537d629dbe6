"""Image metrics on the device (rto_metrics_*, csrc/metrics_kernels.hip) against the numpy model of tests/metrics_ref.py.

Tolerances (fixed; not fitted to the kernel): ssim absolute 1e-9, mse and smape relative 1e-10, psnr absolute 1e-9 dB.  A sum of
N <= 3 x 200 x 136 ~ 8e4 double terms carries at most N x 2^-53 ~ 1e-11 relative error; one SSIM value amplifies rounding by at
most ~1/C2 ~ 1e3 times 2^-53 times a few tens of operations ~ 1e-11; the order sensitivity of the separable sums measured on
the CPU is <= 3e-13.  That leaves two orders of magnitude, seven below what an indexing or halo mistake produces.  The shapes
are the smallest that reach every edge of the 32 x 16 tiling: one tile, a tile whose SSIM part is empty (W or H - 10 ends
before it), partial tiles, several tiles both ways."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import metrics_ref
import rt_octree_amd as R

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


@pytest.fixture(scope="module")
def met():
    return R.ImageMetrics(0)


def _pair(n, H, W, seed, noise=0.05):
    rs = np.random.RandomState(seed)
    pred = rs.uniform(-0.1, 1.1, (n, H, W, 4)).astype(np.float32)
    truth = np.clip(pred + noise * rs.standard_normal((n, H, W, 4)).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return pred, truth


def _bits(m):
    return tuple(struct.pack("<d", float(v)) for v in m)


def _check(met, pred, truth, over_background=None, where=""):
    got = met.compute(_t(pred), _t(truth), over_background=over_background)
    want = metrics_ref.batch_metrics(pred, truth, over_background)
    assert len(got) == len(want) == len(pred)
    for i, (g, w) in enumerate(zip(got, want)):
        metrics_ref.assert_close(g, w, "%s frame %d" % (where, i))
    return got


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(11, 11), (11, 40), (45, 11), (27, 43), (48, 64), (53, 37), (200, 136)])
def test_against_the_model(met, hw, n):
    pred, truth = _pair(n, hw[0], hw[1], seed=hw[0] * 1000 + hw[1] + n)
    got = _check(met, pred, truth, where="%dx%d" % hw)
    assert all(0.0 < g.ssim < 1.0 and g.mse > 0 and math.isfinite(g.psnr) for g in got)


@pytest.mark.parametrize("hw", [(27, 43), (53, 80)])
def test_near_flat_and_constant_images(met, hw):
    """the cancellation case: var = E[x^2] - mu^2 on flat regions against C2 = 9e-4"""
    H, W = hw
    rs = np.random.RandomState(5)
    a = (0.7 + 1e-3 * rs.standard_normal((2, H, W, 4))).astype(np.float32)
    b = (0.7 + 1e-3 * rs.standard_normal((2, H, W, 4))).astype(np.float32)
    _check(met, a, b, where="near-flat")
    c0 = np.full((1, H, W, 4), 0.7, np.float32)
    c1 = np.full((1, H, W, 4), 0.25, np.float32)
    _check(met, c0, c1, where="constant")
    _check(met, c0, a[:1], where="constant vs near-flat")


@pytest.mark.parametrize("kind", ["float", "u8", "float_vs_same_u8_values"])
def test_identical_inputs_are_exact(met, kind):
    rs = np.random.RandomState(9)
    n, H, W = 2, 53, 100  # 4 x 4 tiles, partial ones on both edges
    if kind == "float":
        a = rs.uniform(-0.1, 1.1, (n, H, W, 4)).astype(np.float32)
        b = a.copy()
    else:
        a = rs.randint(0, 256, (n, H, W, 4)).astype(np.uint8)
        b = a.copy() if kind == "u8" else a.astype(np.float32) / np.float32(255.0)
    for g in met.compute(_t(a), _t(b)):
        assert g.ssim == 1.0 and g.mse == 0.0 and g.smape == 0.0 and g.psnr == math.inf, g


@pytest.mark.parametrize("case", ["u8_truth_bg1", "u8_truth_bg025", "u8_pred", "u8_both", "u8_both_bg", "float_truth_bg"])
def test_formats_and_background(met, case):
    rs = np.random.RandomState(13)
    n, H, W = 2, 27, 43
    pred_f, truth_f = _pair(n, H, W, seed=11)
    pred_u = rs.randint(0, 256, (n, H, W, 4)).astype(np.uint8)
    truth_u = np.clip(pred_u.astype(int) + rs.randint(-20, 21, pred_u.shape), 0, 255).astype(np.uint8)
    truth_u[..., 3] = rs.randint(0, 256, (n, H, W))
    truth_fa = truth_f.copy()
    truth_fa[..., 3] = rs.uniform(0, 1, (n, H, W)).astype(np.float32)
    pred, truth, bg = {
        "u8_truth_bg1": (pred_f, truth_u, 1.0), "u8_truth_bg025": (pred_f, truth_u, 0.25), "u8_pred": (pred_u, truth_f, None),
        "u8_both": (pred_u, truth_u, None), "u8_both_bg": (pred_u, truth_u, 0.25), "float_truth_bg": (pred_f, truth_fa, 0.5),
    }[case]
    got = _check(met, pred, truth, over_background=bg, where=case)
    if bg is not None:  # the composite matters: without it the values differ
        plain = met.compute(_t(pred), _t(truth))
        assert all(abs(p.mse - g.mse) > 1e-6 for p, g in zip(plain, got))


def test_batch_and_run_invariance(met):
    import torch
    pred, truth = _pair(5, 45, 70, seed=21)
    tp, tt = _t(pred), _t(truth)
    five = met.compute(tp, tt)
    again = met.compute(tp, tt)
    assert [_bits(m) for m in five] == [_bits(m) for m in again]
    for k in range(5):
        lone = met.compute(tp[k:k + 1].contiguous(), tt[k:k + 1].contiguous())[0]
        assert _bits(lone) == _bits(five[k]), k
    out = torch.full((5, 4), -1.0, dtype=torch.float64, device="cuda:0")
    ret = met.compute_async(tp, tt, out=out)
    torch.cuda.synchronize()
    assert ret is out
    host = out.cpu().numpy()
    assert [_bits(row) for row in host] == [_bits(m) for m in five]
    # the order is mse, psnr, smape, ssim
    assert abs(host[0, 1] + 10.0 * math.log10(host[0, 0])) < 1e-9 and 0.0 < host[0, 3] < 1.0


@pytest.mark.parametrize("hw", [(5, 7), (10, 64), (64, 10)])
def test_small_images_have_no_ssim(met, hw):
    pred, truth = _pair(2, hw[0], hw[1], seed=hw[0])
    got = _check(met, pred, truth, where="small %dx%d" % hw)
    assert all(math.isnan(g.ssim) and g.mse > 0 for g in got)


@pytest.mark.parametrize("where", [("pred", float("nan")), ("truth", float("inf")), ("pred", -float("inf"))])
def test_a_non_finite_pixel_spoils_its_frame_only(met, where):
    side, value = where
    pred, truth = _pair(3, 45, 70, seed=31)
    (pred if side == "pred" else truth)[1, 20, 33, 1] = value
    tp, tt = _t(pred), _t(truth)
    got = met.compute(tp, tt)
    assert all(math.isnan(v) for v in got[1]), got[1]
    for k in (0, 2):
        lone = met.compute(tp[k:k + 1].contiguous(), tt[k:k + 1].contiguous())[0]
        assert _bits(lone) == _bits(got[k]) and all(math.isfinite(v) for v in lone)
    metrics_ref.assert_close(got[1], metrics_ref.frame_metrics(pred[1], truth[1]), "the model agrees")
    # a non-finite alpha is not measured ...
    pred[1, 20, 33, 1] = truth[1, 20, 33, 1] = 0.5
    truth[1, 3, 3, 3] = float("nan")
    assert all(math.isfinite(v) for v in met.compute(_t(pred), _t(truth))[1])
    # ... unless the composite reads it
    assert all(math.isnan(v) for v in met.compute(_t(pred), _t(truth), over_background=1.0)[1])


def test_refusals_leave_the_handle_usable():
    import torch
    L = R.lib()
    h = C.c_void_p(0)
    assert L.rto_metrics_create(0, C.byref(h)) == 0
    assert L.rto_metrics_create(0, None) == -1 and L.rto_metrics_create(1 << 20, C.byref(C.c_void_p(0))) == -1
    pred, truth = _pair(2, 27, 43, seed=41)
    tp, tt = _t(pred), _t(truth)
    tu = _t((truth * 255).astype(np.uint8))
    out = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    host = np.zeros((2, 4), np.float64)
    hp = C.c_void_p(host.ctypes.data)
    P = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc, word):
        msg = L.rto_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def a(m=h, pred=P(tp), pf=0, truth=P(tt), tf=0, n=2, H=27, W=43, flags=0, bg=1.0, out=P(out)):
        return L.rto_metrics_compute_async(m, None, pred, pf, truth, tf, n, H, W, flags, C.c_float(bg), out)

    def s(m=h, pred=P(tp), pf=0, truth=P(tt), tf=0, n=2, H=27, W=43, flags=0, bg=1.0, out=hp):
        return L.rto_metrics_compute(m, None, pred, pf, truth, tf, n, H, W, flags, C.c_float(bg), out)

    for f in (a, s):
        refused(f(m=None), "null argument")
        refused(f(pred=None), "null argument")
        refused(f(truth=None), "null argument")
        refused(f(out=None), "null argument")
        refused(f(n=0), "at least 1")
        refused(f(H=0), "at least 1")
        refused(f(W=-3), "at least 1")
        refused(f(pf=2), "unknown image format 2")
        refused(f(tf=-1), "unknown image format -1")
        refused(f(flags=2), "unknown flag bits")
        refused(f(flags=1, bg=float("nan")), "background is not finite")
        refused(f(flags=1, bg=float("inf")), "background is not finite")
        refused(f(pred=C.c_void_p(host.ctypes.data)), "pred is not memory of the handle's device")
        refused(f(truth=C.c_void_p(host.ctypes.data)), "truth is not memory of the handle's device")
        refused(f(n=1 << 20, H=64, W=64), "index arithmetic")
        refused(f(pred=C.c_void_p(tp.data_ptr() + 4)), "not aligned")
    refused(a(out=hp), "device_out is not memory of the handle's device")
    assert out.abs().sum().item() == 0 and not host.any()  # nothing was enqueued, nothing written
    assert a(bg=float("nan")) == 0  # (the background is not read without the flag)
    # a following valid call on the same handle is correct
    assert s(truth=P(tu), tf=1, flags=1, bg=0.25) == 0
    want = metrics_ref.batch_metrics(pred, (truth * 255).astype(np.uint8), 0.25)
    for i in range(2):
        metrics_ref.assert_close(R.FrameMetrics(*host[i]), want[i], "after the refusals, frame %d" % i)
    L.rto_metrics_free(h)
    L.rto_metrics_free(None)
    # the Python layer's own refusals
    m = R.ImageMetrics(0)
    with pytest.raises(R.RtoError):
        m.compute(tp, tt[:1].contiguous())
    with pytest.raises(R.RtoError):
        m.compute(tp.double(), tt)
    with pytest.raises(R.RtoError):
        m.compute(tp[:, :, ::2], tt[:, :, ::2])


def test_context_route():
    """RenderContext.metrics measures the selected slots' image, or noisy image, in place: the same bits as ImageMetrics on the
    context's views"""
    import torch
    from rt_octree_amd import synth
    W, H, spp = 64, 48, 6
    tree = synth.make_tree(depth_limit=5, basis_dim=9, seed=7)
    dt = R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    fx = synth.blender_focal(W)
    cams = []
    for i in range(2):
        c = R.Camera(W, H, fx, fx)
        c.set_c2w(synth.orbit_poses(4)[i])
        cams.append(c)
    ctx = R.RenderContext(W, H, frames=2)
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=spp, denoise=True), ctx)
    _, noisy_v, image_v = ctx.batch_views()
    noisy, image = torch.as_tensor(noisy_v, device="cuda:0"), torch.as_tensor(image_v, device="cuda:0")
    image.copy_(noisy * 0.5 + 0.125)  # (no denoiser ran: give the image slots a content of their own)
    torch.cuda.synchronize()
    host = noisy.cpu().numpy()
    assert host[..., :3].std() > 0.02, "the frames show nothing"
    rs = np.random.RandomState(3)
    truth = np.clip(host + 0.05 * rs.standard_normal(host.shape), 0.0, 1.0)
    truth[..., 3] = rs.uniform(0.5, 1.0, truth.shape[:3])
    truth = _t((truth * 255).astype(np.uint8))
    met = R.ImageMetrics(0)
    ctx.select_frame(0)
    for is_noisy, view in ((False, image), (True, noisy)):
        got = ctx.metrics(truth, n=2, noisy=is_noisy, over_background=1.0)
        want = met.compute(view, truth, over_background=1.0)
        assert [_bits(g) for g in got] == [_bits(w) for w in want] and all(math.isfinite(v) for g in got for v in g)
    assert _bits(ctx.metrics(truth, n=2)[0]) != _bits(ctx.metrics(truth, n=2, noisy=True)[0])
    ctx.select_frame(1)
    one = ctx.metrics(truth[1:], noisy=True, over_background=1.0)
    assert _bits(one[0]) == _bits(met.compute(noisy[1:], truth[1:], over_background=1.0)[0])
    with pytest.raises(R.RtoError):
        ctx.metrics(truth, n=2)  # two frames from slot 1 of a context of two
    metrics_ref.assert_close(one[0], metrics_ref.frame_metrics(noisy[1].cpu().numpy(), truth[1].cpu().numpy(), 1.0), "context frame 1")
