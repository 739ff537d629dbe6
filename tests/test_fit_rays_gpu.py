"""The tree fit on rays the caller supplies, on the device (rto_tree_fit_grad_rays, csrc/fit_rays_kernels.hip).  Bit for bit: the
kernel's out, grad and stats words equal the host twin's (which tests/test_fit_rays_host.py pins to the numpy restatement) over
every walk, a re-laid file, NDC with a crop and every format; on the rays of cameras they equal the device's fit_grad on the
cameras in raster order, permuted and in splits; buffers 4 bytes off a 16-byte boundary, a second stream, a call between two
renders; free, degenerate and masked rays; ten SGD steps on shuffled batches; the refusals; the tool's two backends."""
import ctypes as C
import os

import numpy as np
import pytest

import rt_octree_amd as R
import test_fit_rays_host as TH
from helpers import rcam, rgba_tree
from rt_octree_amd import synth
from rt_octree_amd._lib import lib

pytestmark = pytest.mark.gpu
W, H = TH.W, TH.H
SENTINEL = TH.SENTINEL


def _upload(tree, **kw):
    return R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra, **kw)


def _dev(dt, params, o, d, tg, grad=None, stats=None, want_grad=True, out=None, stream=None, **optkw):
    """one rto_tree_fit_grad_rays call on numpy inputs -> (out, grad, stats) as torch tensors; out starts as SENTINEL"""
    import torch
    dev = torch.device("cuda", dt.device)
    p = torch.from_numpy(np.ascontiguousarray(params)).to(dev)
    grad = (torch.zeros(params.shape, dtype=torch.int64, device=dev) if grad is None else grad) if want_grad else None
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if stats is None else stats
    out = torch.full((o.shape[0], 3), float(SENTINEL), dtype=torch.float32, device=dev) if out is None else out
    R.fit_grad_rays(dt, p, np.ascontiguousarray(o), np.ascontiguousarray(d), None if tg is None else np.ascontiguousarray(tg),
                    R.RenderOptions(**optkw), grad=grad, stats=stats if tg is not None else None, out=out, stream=stream)
    return out, grad, stats


def _np(triple):
    return tuple(None if a is None else a.cpu().numpy() for a in triple)


def _same(dev, host, what, floor=500):
    TH.same(_np(dev), host, what)
    assert host[1] is None or np.count_nonzero(host[1]) > floor, what + ": nothing was marched"


def _check(dt, tree, o, d, what, ndc=None, floor=500, **optkw):
    params = TH.perturbed_params(tree)
    hf = TH.host_fit(tree, ndc=ndc, **optkw)
    tg = TH.noisy(hf.render_rays(o, d))
    tg[min(400, len(tg) - 1), 1] = np.nan  # one masked ray
    dev = _dev(dt, params, o, d, tg, **optkw)
    _same(dev, TH.call_rays(tree, params, o, d, tg, ndc=ndc, **optkw), what, floor)
    return dev


@pytest.fixture(scope="module")
def tree5():
    return synth.make_tree(5, 9, seed=7)


@pytest.fixture(scope="module")
def rays3():
    return TH.rays_of(TH.cams3())


# ------------------------------------------------------------------ 1. device == twin
def test_two_level_image(tree5, rays3):
    dt = _upload(tree5)
    assert dt.wide_nodes > 0
    _check(dt, tree5, *rays3, "two-level image")
    _check(dt, tree5, *rays3, "stop_thresh 0, background 0.25", stop_thresh=0.0, background_brightness=0.25)


def test_one_level_image(tree5, rays3):
    os.environ["RTO_NO_WIDE"] = "1"
    try:
        dt = _upload(tree5)
    finally:
        del os.environ["RTO_NO_WIDE"]
    assert dt.wide_nodes == 0
    _check(dt, tree5, *rays3, "one-level image")


def test_child_walk_on_an_n4_tree(rays3):
    from test_query import _n4_tree
    tree = _n4_tree()
    o, d = TH.rays_of([rcam(W, H, p) for p in synth.orbit_poses(4)[:3]])
    _check(_upload(tree), tree, o, d, "child[]", floor=100)


def test_depth_6_with_wide_nodes():
    tree = synth.make_tree(6, 9, seed=7)
    dt = _upload(tree)
    assert dt.wide_nodes > 0 and dt.max_depth == 6
    o, d = TH.rays_of([rcam(47, 41, p) for p in synth.orbit_poses(4)[:2]])
    _check(dt, tree, o, d, "depth 6")


def test_a_relaid_file_node_old(tree5, rays3):
    tree = synth.shuffle_nodes(tree5, seed=3)  # params and grad are numbered like the arrays the tree was uploaded from
    _check(_upload(tree), tree, *rays3, "shuffled")


def test_ndc_with_a_cropped_render_bbox(tree5):
    dt = _upload(tree5)
    ndc = (64.0, 48.0, 50.0)
    dt.set_ndc(*ndc)
    poses = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2), (0.0, -0.1, 0.4))]
    o, d = TH.rays_of([rcam(W, H, p, fx=50.0) for p in poses])
    _check(dt, tree5, o, d, "NDC, cropped", ndc=ndc, render_bbox=[0.1, 0.1, 0.0, 0.9, 0.9, 1.0])


@pytest.mark.parametrize("fmt", TH.FORMATS)
def test_every_format(fmt, tree5, rays3):
    tree = rgba_tree(tree5) if fmt == "RGBA" else (tree5 if fmt == "SH9" else synth.make_tree(5, int(fmt[2:]), seed=7))
    _check(_upload(tree), tree, *rays3, fmt)


# ------------------------------------------------------------------ 2. camera rays == the device's camera entry
@pytest.fixture(scope="module")
def cam_case(tree5, rays3):
    """(the device tree, params, origins, dirs, targets, the device's fit_grad on the three cameras as numpy (out, grad, stats))"""
    import torch
    dt = _upload(tree5)
    cams = TH.cams3()
    o, d = rays3
    params = TH.perturbed_params(tree5)
    tg = TH.noisy(TH.host_fit(tree5).render_rays(o, d))
    tg[W * H + 3 * W + 4, 1] = np.nan
    p = torch.from_numpy(params).cuda()
    planes = [torch.from_numpy(x).cuda() for x in np.ascontiguousarray(tg.reshape(3, H, W, 3))]
    images = [torch.full((H, W, 3), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in cams]
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    R.fit_grad(dt, p, cams, planes, R.RenderOptions(), grad=grad, stats=stats, images=images)
    want = (torch.cat([i.reshape(-1, 3) for i in images]).cpu().numpy(), grad.cpu().numpy(), stats.cpu().numpy())
    assert want[2][1] == o.shape[0] - 1 and np.count_nonzero(want[1]) > 1000
    return dt, params, o, d, tg, want


def test_camera_rays_give_the_camera_entrys_bytes(cam_case):
    import torch
    dt, params, o, d, tg, want = cam_case
    n = o.shape[0]
    assert n % 64 != 0 and n % 256 != 0  # one call whose ray count is no multiple of the workgroup's
    TH.same(_np(_dev(dt, params, o, d, tg)), want, "raster order")
    perm = np.random.default_rng(5).permutation(n)
    po, pg, ps = _np(_dev(dt, params, o[perm], d[perm], tg[perm]))
    back = np.empty_like(po)
    back[perm] = po
    TH.same((back, pg, ps), want, "permuted")
    # splits, accumulating: n = 0, 1, 63, 64, 65, 255, 256, 257 and the rest
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((n, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    at = 0
    for k in (0, 1, 63, 64, 65, 255, 256, 257, n - 961):
        _dev(dt, params, o[at:at + k], d[at:at + k], tg[at:at + k], grad=grad, stats=stats, out=out[at:at + k])
        at += k
    assert at == n
    TH.same(_np((out, grad, stats)), want, "splits")
    # forward only, and without targets
    fo, fg, fs = _dev(dt, params, o, d, tg, want_grad=False)
    assert fg is None
    TH.same(_np((fo, None, fs)), (want[0], None, want[2]), "grad == NULL")
    no = _dev(dt, params, o, d, None, want_grad=False)[0].cpu().numpy()
    m = ~np.isnan(tg).any(1)
    assert np.array_equal(no[m].view(np.uint32), want[0][m].view(np.uint32)) and (no[~m] != SENTINEL).all()


def test_buffers_4_bytes_off_a_16_byte_boundary_and_a_second_stream(cam_case):
    import torch
    dt, params, o, d, tg, want = cam_case
    n = o.shape[0]

    def off4(a):
        """the rows of `a` in a buffer that starts 4 bytes after a 16-byte boundary"""
        buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
        shift = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4
        view = buf[shift:shift + a.size].view(a.shape)
        assert view.data_ptr() % 16 == 4
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return view

    p = torch.from_numpy(params).cuda()
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = off4(np.full((n, 3), SENTINEL, np.float32))
    R.fit_grad_rays(dt, p, off4(o), off4(d), off4(tg), grad=grad, stats=stats, out=out)
    TH.same(_np((out, grad, stats)), want, "offset buffers")
    # a second stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _dev(dt, params, o, d, tg, stream=side)
    side.synchronize()
    TH.same(_np(got), want, "second stream")
    # the classes
    df = R.TreeFit(dt, np.zeros(params.shape, np.float16))
    df.params.copy_(p)
    df.accumulate_rays(o, d, tg)
    assert np.array_equal(df.grad.cpu().numpy(), want[1]) and np.array_equal(df.stats.cpu().numpy(), want[2])
    loss = df.loss()
    assert loss[1] == n - 1 and df.evaluate_rays(o, d, tg) == loss
    m = ~np.isnan(tg).any(1)
    assert np.array_equal(df.render_rays(o, d).cpu().numpy()[m].view(np.uint32), want[0][m].view(np.uint32))


def test_a_call_between_two_renders_changes_neither_the_frames_nor_the_rng(cam_case):
    dt, params, o, d, tg, want = cam_case
    cam = rcam(47, 47, synth.orbit_poses(4)[1])
    opt = R.RenderOptions(spp=6, denoise=False)

    def two_frames(between):
        ctx = R.RenderContext(cam.width, cam.height)
        ctx.rng_seed()
        R.launch_renderer(dt, cam, opt, ctx)
        a = ctx.download_aux()
        if between:
            TH.same(_np(_dev(dt, params, o, d, tg)), want, "between two renders")
        ctx.rng_advance()
        R.launch_renderer(dt, cam, opt, ctx)
        return a, ctx.download_aux(), ctx.rng_get()

    a0, b0, r0 = two_frames(False)
    a1, b1, r1 = two_frames(True)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))
    assert tuple(r0) == tuple(r1)
    assert not np.array_equal(a0.view(np.uint32), b0.view(np.uint32))


# ------------------------------------------------------------------ 3. free, degenerate and masked rays
def test_free_rays():
    tree = synth.make_tree(4, 4, seed=7)
    dt = _upload(tree)
    o, d, _ = TH.free_rays(tree)
    params = TH.perturbed_params(tree)
    tg = TH.noisy(TH.host_fit(tree).render_rays(o, d), seed=2)
    host = TH.call_rays(tree, params, o, d, tg)
    _same(_dev(dt, params, o, d, tg), host, "free rays")
    for s in (4.0, 0.125):
        _same(_dev(dt, params, o, d * np.float32(s), tg), host, "dirs x %g" % s)


def test_degenerate_and_masked_rays(tree5):
    dt = _upload(tree5)
    o, d, tg, bad = TH.degenerate_rays(tree5)
    params = TH.perturbed_params(tree5)
    dev = _dev(dt, params, o, d, tg, background_brightness=0.25)
    _same(dev, TH.call_rays(tree5, params, o, d, tg, background_brightness=0.25), "degenerate", floor=50)
    out, grad, stats = _np(dev)
    assert (out[bad] == np.float32(0.25)).all() and stats[1] == 63 and (out[9] == SENTINEL).all()
    keep = np.setdiff1d(np.arange(64), bad)
    _, g2, s2 = _np(_dev(dt, params, o[keep], d[keep], tg[keep], background_brightness=0.25))
    assert np.array_equal(g2, grad) and s2[1] == 60


# ------------------------------------------------------------------ 4. ten SGD steps
def test_ten_sgd_steps_give_the_hosts_loss_words_and_params_bits():
    import torch
    t, o, d, tg, batches = TH.sgd_rays()
    words_h, hf = TH.ten_steps_host(t, o, d, tg, batches)
    df = R.TreeFit(_upload(t), t.data)
    df.params.copy_(torch.from_numpy(TH.start_params(t)))
    od, dd, td = (torch.from_numpy(a).cuda() for a in (o, d, tg))
    words_d = []
    for epoch in batches:
        for idx in epoch:
            i = torch.from_numpy(idx).cuda()
            df.accumulate_rays(od[i], dd[i], td[i])
            df.step(TH.LR10)
        words_d.append(int(df.stats.cpu()[0]))
        assert df.loss()[1] == 5 * TH.BATCH
    assert words_d == words_h and words_d[1] < words_d[0], (words_d, words_h)
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), hf.params.view(np.uint32))


# ------------------------------------------------------------------ 5. refusals
def test_device_refusals(tree5, rays3, tmp_path):
    import torch
    dt = _upload(tree5)
    o, d = (torch.from_numpy(a[:64].copy()).cuda() for a in rays3)
    params = torch.from_numpy(TH.perturbed_params(tree5)).cuda()
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    tg = torch.full((64, 3), 0.5, device="cuda")
    out = torch.zeros((64, 3), device="cuda")
    co = R.RenderOptions().to_c()
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731

    def raw(tree=dt._h, params=params, origins=o, dirs=d, targets=tg, out=out, n=64, opt=co, grad=grad, stats=stats):
        return lib().rto_tree_fit_grad_rays(tree, ptr(params), ptr(origins), ptr(dirs), ptr(targets), ptr(out), n,
                                            C.byref(opt) if opt is not None else None, ptr(grad), ptr(stats), None)

    def refused(text, code=-1, **kw):
        rc = raw(**kw)
        msg = lib().rto_last_error().decode()
        assert rc == code and text in msg and msg.startswith("rto_tree_fit_grad_rays: "), (rc, msg, text)

    refused("null tree", tree=None)
    refused("null params", params=None)
    refused("null options", opt=None)
    refused("null origins with n > 0", origins=None)
    refused("null dirs with n > 0", dirs=None)
    refused("n must be >= 0", n=-1)
    refused("null targets with grad or stats set", targets=None)
    refused("dirs must be 4-byte aligned", dirs=d.data_ptr() + 2)
    refused("out must be 4-byte aligned", out=out.data_ptr() + 1)
    refused("grad must be 8-byte aligned", grad=grad.data_ptr() + 4)
    refused("stats must be 8-byte aligned", stats=stats.data_ptr() + 4)
    refused("params overlaps targets", targets=params.data_ptr() + 1024)
    refused("grad overlaps out", out=grad.data_ptr() + 64)
    refused("out overlaps origins", out=o)
    refused("rot_dirs is not read", opt=R.RenderOptions(rot_dirs=[0.1, 0.0, 0.0]).to_c())
    refused("basis_minmax is not read", opt=R.RenderOptions(basis_minmax=[1, 24]).to_c())
    # memory of the wrong kind: host pointers
    host_rays = np.ones((64, 3), np.float32)
    host_params = np.zeros(tuple(params.shape), np.float32)
    refused("dirs is not memory of the tree's device", dirs=host_rays.ctypes.data)
    refused("targets is not memory of the tree's device", targets=host_rays.ctypes.data)
    refused("out is not memory of the tree's device", out=host_rays.ctypes.data)
    refused("params is not memory of the tree's device", params=host_params.ctypes.data, grad=None, stats=None, targets=None)
    torch.cuda.synchronize()
    assert not grad.any() and not stats.any() and not out.any(), "a refused call wrote"
    assert raw(origins=None, dirs=None, targets=None, out=None, n=0, grad=None, stats=None) == 0  # n == 0 launches nothing
    assert raw(origins=None, dirs=None, out=None, n=0) == 0
    # trees the fit does not take
    refused("RTO_TREE_COMPACT_RECORDS", code=-3, tree=_upload(tree5, compact_records=True)._h)
    path = str(tmp_path / "quant.npz")
    tree5.save_quant_npz(path, n_retain=1)
    refused("RTO_TREE_QUANT_DIRECT", code=-3, tree=R.N3Tree(path, quant_direct=True)._h)
    # the Python wrapper's own checks: volrend._ray_tensor's
    with pytest.raises(R.RtoError):
        R.fit_grad_rays(dt, params, o, d[:3])
    with pytest.raises(R.RtoError):
        R.fit_grad_rays(dt, params, o, d.double())
    with pytest.raises(R.RtoError):
        R.fit_grad_rays(dt, params, o.cpu(), d)
    with pytest.raises(TypeError):
        R.fit_grad_rays(dt, params, o, d, out=np.zeros((64, 3), np.float32))


# ------------------------------------------------------------------ 6. the tool
def test_optimize_octree_backends_write_the_same_bytes_with_batch_rays(tmp_path, tree5):
    js, pert = TH.write_dataset(tmp_path, tree5)
    flags = ("--batch_rays", str(TH.BATCH), "--seed", "1")
    hip = TH.run_tool(tmp_path, "hip", pert, js, "hip", *flags)
    assert hip == TH.run_tool(tmp_path, "cpu", pert, js, "cpu", *flags), "the optimised files differ"
    with np.load(tmp_path / "hip" / "pert.npz") as f, np.load(pert) as z:
        assert np.count_nonzero(f["data"].view(np.uint16) != z["data"].view(np.uint16)) > 1000
