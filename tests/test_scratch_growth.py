"""A handle's scratch buffers (DeviceBuf, csrc/rto_abi_common.h) grow in mid-life: each handle type works on a small shape, a
larger one that regrows every scratch it owns, and the small one again; every result equals, bit for bit, that of a fresh handle
which saw only that shape."""
import numpy as np
import pytest

import rt_octree_amd as R
from rt_octree_amd import metrics, synth

torch = pytest.importorskip("torch")
from rt_octree_amd import denoiser  # noqa: E402

import guidance_train_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s, output %d" % (what, i)


def _grow_and_compare(shapes, fresh, run):
    """run(handle, shape) -> arrays, on one handle through `shapes` and on a fresh() handle per shape"""
    shared = fresh()
    got = [run(shared, s) for s in shapes]
    for s, g in zip(shapes, got):
        _same_bits(g, run(fresh(), s), "%s on the handle that saw %s" % (s, shapes))


def test_image_metrics_scratch_grows():
    def run(m, shape):  # (11: the smallest side that has an SSIM window)
        rs = np.random.RandomState(shape[2])
        pred, truth = (torch.from_numpy(rs.rand(*shape, 4).astype(np.float32)).cuda() for _ in range(2))
        return [np.array(m.compute(pred, truth), np.float64)]

    _grow_and_compare([(1, 11, 11), (3, 27, 43), (1, 11, 11)], metrics.ImageMetrics, run)


def test_training_scratch_grows():
    """net 8 -> 8 -> 8, 4 levels; 2 x 20 x 36 crosses the 32 x 16 convolution tile and the 32 x 4 gradient tile in both axes: dz, the
    gradient partial sums and the loss partial sums all grow"""
    layers = [(w.cuda(), b.cuda()) for w, b in G.make_net(8, 4, 2)]

    def fresh():  # (the package keeps one training handle per device: dropping it makes the next call create one)
        denoiser._TrainHandle._by_device.clear()

    def run(_handle, shape):
        n, H, W = shape
        params = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in layers]
        rs = np.random.RandomState(H)
        up = [torch.from_numpy(rs.randn(n, 4, H, W).astype(np.float32)).cuda() for _ in range(2)]
        wm, gm = denoiser.guidance_autograd(G.make_aux(n, H, W).cuda(), params, 4)
        ((wm * up[0]).sum() + (gm * up[1]).sum()).backward()
        pred = torch.from_numpy(rs.rand(n, H, W, 4).astype(np.float32)).cuda().requires_grad_(True)
        loss = denoiser.image_loss(pred, torch.from_numpy(rs.rand(n, H, W, 4).astype(np.float32)).cuda())
        loss.backward()
        out = [wm, gm, loss, pred.grad] + [t.grad for wb in params for t in wb]
        return [t.detach().cpu().numpy() for t in out]

    try:
        _grow_and_compare([(1, 8, 8), (2, 20, 36), (1, 8, 8)], fresh, run)
    finally:
        fresh()


def _reference_net(seed=0):
    torch.manual_seed(seed)
    compact = denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, 32, 5, 2, 4)).eval()
    return lambda: denoiser.FusedGuidanceNet(compact)


def test_packed_scratch_grows():
    def run(net, shape):
        n, H, W = shape
        rs = np.random.RandomState(W)
        rgba = rs.rand(n, 4, H, W).astype(np.float32)
        aux = torch.from_numpy(np.concatenate([rgba, rgba * rgba], 1)).cuda()
        img = torch.from_numpy(rs.rand(n, H, W, 4).astype(np.float32)).cuda()
        out = torch.full_like(img, -7.0)
        net.forward_packed(aux)
        net.filter_packed(img, out)
        return [out.cpu().numpy()]

    _grow_and_compare([(1, 16, 16), (2, 24, 40), (1, 16, 16)], _reference_net(), run)


def test_planes_scratch_of_rto_denoise_grows(small_tree_sh9):
    """rto_denoise(EXACT) is the only caller of the planes scratch: two render contexts on one net, one frame of 16 x 16, then two
    frames of 40 x 24 (the contexts keep their rendered frames: every net denoises the same inputs)"""
    t = small_tree_sh9
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    ctxs = {}
    for W, H, n in ((16, 16, 1), (40, 24, 2)):
        fx = synth.blender_focal(W)
        cams = []
        for pose in synth.orbit_poses(n):
            cams.append(R.Camera(W, H, fx, fx))
            cams[-1].set_c2w(pose)
        ctx = R.RenderContext(W, H, frames=n)
        ctx.rng_seed()
        R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=4, denoise=True), ctx)
        ctxs[(n, H, W)] = ctx

    def run(net, shape):
        ctx = ctxs[shape]
        images = torch.as_tensor(ctx.batch_views()[2], device="cuda:0")
        images.fill_(-7.0)
        ctx.select_frame(0)
        net.denoise(ctx, shape[0], R.FILTER_EXACT)
        torch.cuda.synchronize()
        return [images.cpu().numpy()]

    try:
        _grow_and_compare([(1, 16, 16), (2, 24, 40), (1, 16, 16)], _reference_net(3), run)
    finally:
        for ctx in ctxs.values():
            ctx.free()
        dt.free()
