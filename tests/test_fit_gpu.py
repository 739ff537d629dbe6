"""The tree fit on the device (rto_tree_fit_grad / rto_fit_sgd_step, csrc/fit_kernels.hip): the kernels' grad, stats and image
words equal the host twin's -- which tests/test_fit_host.py pins to the numpy restatement and the float64 model -- over every
walk (two-level image, one-level image, child[]), a re-laid file, NDC, every format, chunked and mixed-size camera lists, splits,
masked pixels; ten SGD steps give the host's loss words and params bits; a call between two renders disturbs neither; the
tool's two backends write the same bytes."""
import os

import numpy as np
import pytest

import rt_octree_amd as R
from helpers import FRAME_ANISO, rcam, reframe, reframe_pose, rgba_tree
from rt_octree_amd import optimize_octree, synth
from rt_octree_amd._lib import check, lib

pytestmark = pytest.mark.gpu
W, H = 23, 19
LR10 = 2.0  # tests/test_fit_host.py chose it


def _upload(tree, **kw):
    return R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra, **kw)


def _cams3(w=W, h=H):
    return [rcam(w, h, p) for p in synth.orbit_poses(4)[:3]]


def _targets(cams, seed=1):
    """smooth images with noise, one masked pixel in the second"""
    rng = np.random.default_rng(seed)
    out = []
    for c in cams:
        yy, xx = np.mgrid[0:c.height, 0:c.width]
        base = np.stack([0.5 + 0.4 * np.sin(xx / 5.0), 0.5 + 0.4 * np.cos(yy / 7.0), (xx + yy) / float(c.height + c.width)], -1)
        out.append(np.clip(base + rng.uniform(-0.1, 0.1, base.shape), 0, 1).astype(np.float32))
    if len(out) > 1:
        out[1][3, 4, 1] = np.nan
    return out


def _perturbed_params(tree):
    """float32 params that differ from the uploaded halves (the field is what params says)"""
    p = tree.data.astype(np.float32)
    p[..., :-1] *= np.float32(0.75)
    p[..., -1] *= np.float32(0.9)
    return p


def _host(tree, params, cams, targets, ndc=None, **optkw):
    grad = np.zeros(params.shape, np.int64)
    stats = np.zeros(2, np.int64)
    images = [np.zeros((c.height, c.width, 3), np.float32) for c in cams]
    R.fit_grad_host(tree.child, tree.data, params, tree.scale, tree.offset, tree.data_format, cams, targets, R.RenderOptions(**optkw),
                    ndc=ndc, threads=8, grad=grad, stats=stats, images=images)
    return images, grad, stats


def _dev(dt, params, cams, targets, grad=None, stats=None, want_grad=True, **optkw):
    import torch
    dev = torch.device("cuda", dt.device)
    p = torch.from_numpy(params).to(dev)
    tg = None if targets is None else [torch.from_numpy(t).to(dev) for t in targets]
    grad = (torch.zeros(params.shape, dtype=torch.int64, device=dev) if grad is None else grad) if want_grad else None
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if stats is None else stats
    images = [torch.zeros((c.height, c.width, 3), dtype=torch.float32, device=dev) for c in cams]
    R.fit_grad(dt, p, cams, tg, R.RenderOptions(**optkw), grad=grad, stats=stats if tg is not None else None, images=images)
    return images, grad, stats


def _same(dev, host, what, floor=500):
    di, dg, ds = dev
    hi, hg, hs = host
    for f, (a, b) in enumerate(zip(di, hi)):
        bad = np.flatnonzero(a.cpu().numpy().view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
        assert bad.size == 0, "%s: image %d: %d of %d words differ; first at %d" % (what, f, bad.size, b.size, bad[0])
    got = dg.cpu().numpy()
    bad = np.flatnonzero(got.reshape(-1) != hg.reshape(-1))
    assert bad.size == 0, "%s: %d of %d grad words differ; first at %d: %d vs %d" % (
        what, bad.size, hg.size, bad[0], got.reshape(-1)[bad[0]], hg.reshape(-1)[bad[0]])
    assert np.array_equal(ds.cpu().numpy(), hs), "%s: stats %s vs %s" % (what, ds.cpu().numpy(), hs)
    assert np.count_nonzero(hg) > floor, what + ": nothing was marched"


def _check(dt, tree, cams, what, ndc=None, floor=500, **optkw):
    params, targets = _perturbed_params(tree), _targets(cams)
    dev = _dev(dt, params, cams, targets, **optkw)
    _same(dev, _host(tree, params, cams, targets, ndc=ndc, **optkw), what, floor)
    return dev


@pytest.fixture(scope="module")
def tree5():
    return synth.make_tree(5, 9, seed=7)


def test_depth_6_default_upload_splits_chunks_mixed_sizes_masks_and_no_camera():
    import torch
    tree = synth.make_tree(6, 9, seed=7)
    dt = _upload(tree)
    assert dt.wide_nodes > 0
    bytes_before = dt.device_bytes
    cams = [rcam(47, 41, p) for p in synth.orbit_poses(4)[:3]]  # 3 x 3 workgroups, partial tiles
    params, targets = _perturbed_params(tree), _targets(cams)
    whole = _dev(dt, params, cams, targets)
    host = _host(tree, params, cams, targets)
    _same(whole, host, "depth 6, two-level image")
    assert host[2][1] == 3 * 47 * 41 - 1 and not whole[0][1][3, 4].any(), "the masked pixel"
    _check(dt, tree, cams, "stop_thresh 0, background 0.25", stop_thresh=0.0, background_brightness=0.25)
    dt._refresh()
    assert dt.device_bytes == bytes_before, "the call brought child[] / data[] back"
    # a split of one call into two, accumulating
    _, g, s = _dev(dt, params, cams[:1], targets[:1])
    _, g, s = _dev(dt, params, cams[1:], targets[1:], grad=g, stats=s)
    assert torch.equal(g, whole[1]) and torch.equal(s, whole[2])
    # n = 0 launches nothing and leaves grad and stats alone
    keep_g, keep_s = g.clone(), s.clone()
    _dev(dt, params, [], [], grad=g, stats=s)
    assert torch.equal(g, keep_g) and torch.equal(s, keep_s)
    # forward only: the same images with grad == NULL, and without targets (the masked pixel is rendered then)
    fi, fg, fs = _dev(dt, params, cams, targets, want_grad=False)
    assert fg is None and torch.equal(fs, whole[2]) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(fi, whole[0]))
    ri, _, _ = _dev(dt, params, cams, None, want_grad=False)
    hi = R.HostTreeFit(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, threads=8)
    hi.params[...] = params
    for a, b in zip(ri, hi.render(cams)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    # 33 cameras of 17 x 13 in one call: one more than a launch takes, partial tiles
    poses = synth.orbit_poses(33)
    _check(dt, tree, [rcam(17, 13, p) for p in poses], "33 cameras")
    # mixed sizes in one call (runs of one size become launches)
    mixed = [rcam(17, 13, poses[0]), rcam(17, 13, poses[5]), rcam(31, 9, poses[9]), rcam(17, 13, poses[13]), rcam(16, 16, poses[20])]
    _check(dt, tree, mixed, "mixed sizes")


def test_device_refusals(tree5, tmp_path):
    import torch
    dt = _upload(tree5)
    cams = _cams3()[:2]
    params = torch.from_numpy(_perturbed_params(tree5)).cuda()
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    tg = [torch.from_numpy(t).cuda() for t in _targets(cams)]

    def refused(code, text, **kw):
        args = dict(tree=dt, params=params, cams=cams, targets=tg, grad=grad, stats=stats)
        args.update(kw)
        with pytest.raises(R.RtoError) as e:
            R.fit_grad(args.pop("tree"), args.pop("params"), args.pop("cams"), args.pop("targets"), args.pop("options", None), **args)
        assert e.value.code == code and text in e.value.msg and e.value.msg.startswith("rto_tree_fit_grad: "), e.value.msg

    bad = rcam(W, H, synth.orbit_poses(4)[0])
    bad.fx = 0.0
    refused(-1, "camera 1: width, height (<= 1048560), fx or fy is out of range", cams=[cams[0], bad])
    refused(-1, "rot_dirs is not read", options=R.RenderOptions(rot_dirs=[0.1, 0.0, 0.0]))
    refused(-1, "basis_minmax is not read", options=R.RenderOptions(basis_minmax=[1, 24]))
    refused(-1, "null targets with grad or stats set", targets=None)
    flat = params.view(-1)
    inside = flat[1024:1024 + W * H * 3].view(H, W, 3)
    refused(-1, "camera 1: params overlaps the target", targets=[tg[0], inside])
    refused(-1, "camera 0: params overlaps the image", images=[inside, None])
    # memory that is not the device's: the raw entry with a host pointer
    import ctypes as C
    from rt_octree_amd._lib import CCamera
    arr = (CCamera * 2)(*[c.to_c() for c in cams])
    co = R.RenderOptions().to_c()
    host_plane = np.zeros((H, W, 3), np.float32)
    ptrs = (C.c_void_p * 2)(tg[0].data_ptr(), host_plane.ctypes.data)
    rc = lib().rto_tree_fit_grad(dt._h, C.c_void_p(params.data_ptr()), arr, ptrs, None, 2, C.byref(co), C.c_void_p(grad.data_ptr()),
                                 C.c_void_p(stats.data_ptr()), None)
    assert rc == -1 and "camera 1: target is not memory of the tree's device" in lib().rto_last_error().decode()
    host_params = np.zeros(tuple(params.shape), np.float32)
    rc = lib().rto_tree_fit_grad(dt._h, C.c_void_p(host_params.ctypes.data), arr, ptrs, None, 2, C.byref(co), None, None, None)
    assert rc == -1 and "params is not memory of the tree's device" in lib().rto_last_error().decode()
    torch.cuda.synchronize()
    assert not grad.any() and not stats.any(), "a refused call wrote"
    # trees the fit does not take
    dc = _upload(tree5, compact_records=True)
    refused(-3, "RTO_TREE_COMPACT_RECORDS", tree=dc)
    path = str(tmp_path / "quant.npz")
    tree5.save_quant_npz(path, n_retain=1)
    refused(-3, "RTO_TREE_QUANT_DIRECT", tree=R.N3Tree(path, quant_direct=True))
    sg = synth.with_lobes(synth.make_tree(4, 4, seed=7), "SG")
    dsg = _upload(sg)
    with pytest.raises(R.RtoError) as e:
        R.fit_grad(dsg, torch.zeros((sg.capacity, 2, 2, 2, sg.data.shape[-1]), device="cuda"), cams, tg, grad=None, stats=stats)
    assert e.value.code == -3 and "the fit takes RGBA and SH trees" in e.value.msg
    # the step's refusals
    with pytest.raises(R.RtoError):
        R.sgd_step(params, grad[:1], 1.0)
    assert lib().rto_fit_sgd_step(None, C.c_void_p(grad.data_ptr()), 4, 1.0, None) == -1
    assert lib().rto_fit_sgd_step(C.c_void_p(host_params.ctypes.data), C.c_void_p(grad.data_ptr()), 4, 1.0, None) == -1
    assert "params and grad must be memory of one device" in lib().rto_last_error().decode()


@pytest.mark.parametrize("depth", [7, 8])
def test_wide_node_pairs_below_the_top_grid(depth):
    """basis_dim 4 at depth 7 and 8: one and two wide-node pairs below the top grid (tests/test_query.py _variants)"""
    tree = synth.make_tree(depth, 4, seed=7)
    dt = _upload(tree)
    assert dt.wide_nodes > 0 and dt.max_depth == depth
    _check(dt, tree, _cams3(), "depth %d" % depth)


def test_one_level_image(tree5):
    os.environ["RTO_NO_WIDE"] = "1"
    try:
        dt = _upload(tree5)
    finally:
        del os.environ["RTO_NO_WIDE"]
    assert dt.wide_nodes == 0
    _check(dt, tree5, _cams3(), "one-level image")


@pytest.mark.parametrize("name", ["keep_reference", "shuffled", "reframed", "n4"])
def test_storage_forms_and_tree_shapes(name, tree5):
    from test_query import _n4_tree
    cams = _cams3()
    floor = 500
    if name == "keep_reference":
        tree, kw = tree5, {"keep_reference": True}
    elif name == "shuffled":  # params and grad are numbered like the arrays the tree was uploaded from (node_old)
        tree, kw = synth.shuffle_nodes(tree5, seed=3), {}
    elif name == "reframed":
        tree, kw = reframe(tree5, *FRAME_ANISO), {}
        cams = [rcam(W, H, reframe_pose(p, tree5, tree)) for p in synth.orbit_poses(4)[:3]]
    else:  # no traversal image: child[] with the float descent
        tree, kw, floor = _n4_tree(), {}, 100
    _check(_upload(tree, **kw), tree, cams, name, floor=floor)


@pytest.mark.parametrize("fmt", ["RGBA", "SH1", "SH4", "SH9", "SH16", "SH25"])
def test_every_format_at_depth_5(fmt, tree5):
    tree = rgba_tree(tree5) if fmt == "RGBA" else (tree5 if fmt == "SH9" else synth.make_tree(5, int(fmt[2:]), seed=7))
    _check(_upload(tree), tree, _cams3(), fmt)


def test_ndc_with_a_cropped_render_bbox(tree5):
    dt = _upload(tree5)
    _check(dt, tree5, _cams3(), "render_bbox crop", render_bbox=[0.2, 0.1, 0.3, 0.8, 0.9, 0.7])
    ndc = (64.0, 48.0, 50.0)
    dt.set_ndc(*ndc)
    poses = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2), (0.0, -0.1, 0.4))]
    _check(dt, tree5, [rcam(W, H, p, fx=50.0) for p in poses], "NDC, cropped", ndc=ndc, render_bbox=[0.1, 0.1, 0.0, 0.9, 0.9, 1.0])


def test_ten_sgd_steps_give_the_hosts_loss_words_and_params_bits(tree5):
    import torch
    cams = _cams3()
    ref = R.HostTreeFit(tree5.child, tree5.data, tree5.scale, tree5.offset, tree5.data_format, threads=8)
    targets = ref.render(cams)
    hf = R.HostTreeFit(tree5.child, tree5.data, tree5.scale, tree5.offset, tree5.data_format, threads=8)
    df = R.TreeFit(_upload(tree5), tree5.data)
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), hf.params.view(np.uint32))
    hf.params[..., :-1] *= np.float32(0.5)
    hf.params[..., -1] *= np.float32(0.8)
    df.params.copy_(torch.from_numpy(hf.params))
    tg_dev = [torch.from_numpy(t).cuda() for t in targets]
    words_h, words_d = [], []
    for _ in range(10):
        hf.accumulate(cams, targets)
        df.accumulate(cams, tg_dev)
        words_h.append(int(hf.stats[0]))
        words_d.append(int(df.stats.cpu()[0]))
        assert hf.loss() == df.loss()
        hf.step(LR10)
        df.step(LR10)
        assert not df.grad.any()
    assert words_d == words_h and all(b < a for a, b in zip(words_d, words_d[1:])), (words_d, words_h)
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), hf.params.view(np.uint32))
    assert np.array_equal(df.data_half().view(np.uint16), hf.data_half().view(np.uint16))
    for a, b in zip(df.render(cams), hf.render(cams)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert df.evaluate(cams, tg_dev) == hf.evaluate(cams, targets)


def test_the_step_on_unaligned_and_odd_counts():
    """the 16-byte form needs both arrays 16-byte aligned; views that are not take the single accesses, a count that is no
    multiple of 4 ends in them: the same bits as the host step either way"""
    import torch
    rng = np.random.default_rng(4)
    n = 4 * 256 * 3 + 7
    p = rng.normal(0, 1, n + 4).astype(np.float32)
    g = rng.integers(-2 ** 40, 2 ** 40, n + 4).astype(np.int64)
    g[::7] = 0
    for off, count in ((0, n), (1, n), (0, 5), (2, 4 * 256)):
        hp, hg = p[off:off + count].copy(), g[off:off + count].copy()
        R.sgd_step_host(hp, hg, 0.37)
        tp, tgq = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
        R.sgd_step(tp[off:off + count], tgq[off:off + count], 0.37)
        want_p, want_g = p.copy(), g.copy()
        want_p[off:off + count], want_g[off:off + count] = hp, 0
        assert np.array_equal(tp.cpu().numpy().view(np.uint32), want_p.view(np.uint32)), (off, count)
        assert np.array_equal(tgq.cpu().numpy(), want_g), (off, count)


def test_a_call_between_two_renders_changes_neither_the_frames_nor_the_rng(tree5):
    dt = _upload(tree5)
    cam = rcam(47, 47, synth.orbit_poses(4)[1])
    opt = R.RenderOptions(spp=6, denoise=False)
    cams = _cams3()
    params, targets = _perturbed_params(tree5), _targets(cams)

    def two_frames(between):
        ctx = R.RenderContext(cam.width, cam.height)
        ctx.rng_seed()
        R.launch_renderer(dt, cam, opt, ctx)
        a = ctx.download_aux()
        if between:
            _dev(dt, params, cams, targets)
        ctx.rng_advance()
        R.launch_renderer(dt, cam, opt, ctx)
        return a, ctx.download_aux(), ctx.rng_get()

    a0, b0, r0 = two_frames(False)
    a1, b1, r1 = two_frames(True)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))
    assert tuple(r0) == tuple(r1)
    assert not np.array_equal(a0.view(np.uint32), b0.view(np.uint32))


def test_optimize_octree_backends_write_the_same_bytes(tmp_path, tree5):
    cams = _cams3()
    images = R.HostTreeFit(tree5.child, tree5.data, tree5.scale, tree5.offset, tree5.data_format, threads=8).render(cams)
    os.makedirs(tmp_path / "test")
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), synth.orbit_poses(4)[:3])
    for i, im in enumerate(images):
        u8 = np.concatenate([np.clip(np.rint(im * 255), 0, 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
        u8[:2, :, 3] = 0  # some transparent rows: composited over the background
        u8 = np.ascontiguousarray(u8)
        check(lib().rto_image_write_png(str(tmp_path / "test" / ("r_%d.png" % i)).encode(), u8.ctypes.data, W, H))
    src = tree5.save_npz(str(tmp_path / "tree.npz"))
    with np.load(src) as f:
        z = {k: f[k] for k in f.files}
    d = tree5.data.astype(np.float32)
    d[..., :-1] *= 0.5
    z["data"] = d.astype(np.float16)
    pert = str(tmp_path / "pert.npz")
    np.savez_compressed(pert, **z)
    outs = {}
    for backend in ("hip", "cpu"):
        out_dir = tmp_path / backend
        assert optimize_octree.main([pert, "--poses", js, "--epochs", "2", "--batch_imgs", "2", "--lr", "4000", "--val_poses", js,
                                     "--backend", backend, "--out_dir", str(out_dir)]) == 0
        outs[backend] = (out_dir / "pert.npz").read_bytes()
    assert outs["hip"] == outs["cpu"], "the optimised files differ"
    with np.load(tmp_path / "hip" / "pert.npz") as f:
        assert f["data"].dtype == np.float16 and f["data"].shape == tree5.data.shape and np.array_equal(f["child"], tree5.child)
        assert np.count_nonzero(f["data"].view(np.uint16) != z["data"].view(np.uint16)) > 1000
