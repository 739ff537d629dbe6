"""The sparse step of the tree fit on the device (rto_tree_fit_grad_rays_touched, rto_fit_touched_list, rto_fit_step_sparse;
csrc/fit_sparse_kernels.hip).  Bit for bit: out, grad, stats, the bitmap, the list, the count, params, m and v equal the host
twins' (which tests/test_fit_sparse_host.py pins to the numpy restatement) over every walk, a depth-6 tree with wide nodes, a
re-laid file, NDC with a crop and every format, in splits, on a second stream and in buffers 4 bytes off a 16-byte boundary; the
marking entry's grad equals the device's old entry; the list on synthetic bitmaps; count == 0; the SGD identity against the
device's rto_fit_sgd_step; ten RMSProp and Adam steps; a step between two renders; the refusals; the tool's two backends."""
import ctypes as C
import os

import numpy as np
import pytest

import fit_sparse_ref as SR
import rt_octree_amd as R
import test_fit_rays_gpu as TG
import test_fit_rays_host as TH
import test_fit_sparse_host as TS
from helpers import rcam, rgba_tree
from rt_octree_amd import optimize_octree, synth
from rt_octree_amd._lib import CFitOptim, lib

pytestmark = pytest.mark.gpu
W, H = TH.W, TH.H
SENTINEL = TH.SENTINEL


def _dev(dt, tree, params, o, d, tg, grad=None, stats=None, out=None, touched=None, stream=None, **optkw):
    """one rto_tree_fit_grad_rays_touched call on numpy inputs -> (out, grad, stats, touched) as torch tensors"""
    import torch
    dev = torch.device("cuda", dt.device)
    p = torch.from_numpy(np.ascontiguousarray(params)).to(dev)
    grad = torch.zeros(params.shape, dtype=torch.int64, device=dev) if grad is None else grad
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if stats is None else stats
    out = torch.full((o.shape[0], 3), float(SENTINEL), dtype=torch.float32, device=dev) if out is None else out
    touched = torch.zeros(R.touched_words(TS.n_slots(tree)), dtype=torch.int32, device=dev) if touched is None else touched
    R.fit_grad_rays(dt, p, np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tg), R.RenderOptions(**optkw), grad=grad,
                    stats=stats, out=out, stream=stream, touched=touched)
    return out, grad, stats, touched


def _np(quad):
    o, g, s, t = (a.cpu().numpy() for a in quad)
    return o, g, s, t.view(np.uint32)


def _same(dev, host, what):
    TH.same(dev[:3], host[:3], what)
    assert np.array_equal(dev[3], host[3]), "%s: %d bitmap words differ" % (what, np.count_nonzero(dev[3] != host[3]))


def _check(dt, tree, o, d, what, ndc=None, floor=500, **optkw):
    params = TH.perturbed_params(tree)
    tg = TH.noisy(TH.host_fit(tree, ndc=ndc, **optkw).render_rays(o, d))
    tg[min(400, len(tg) - 1), 1] = np.nan  # one masked ray
    dev = _np(_dev(dt, tree, params, o, d, tg, **optkw))
    host = TS.call_touched(tree, params, o, d, tg, ndc=ndc, **optkw)
    _same(dev, host, what)
    assert SR.bits_of(host[3], TS.n_slots(tree)).sum() >= floor, what + ": too few leaves were reached"
    # the marking entry's out, grad and stats are the old entry's on the device
    TH.same(TG._np(TG._dev(dt, params, o, d, tg, **optkw)), dev[:3], what + " against the old entry")
    return dev


@pytest.fixture(scope="module")
def tree5():
    return synth.make_tree(5, 9, seed=7)


@pytest.fixture(scope="module")
def rays3():
    return TH.rays_of(TH.cams3())


# ------------------------------------------------------------------ 1. the marking kernel == the twin
def test_two_level_image(tree5, rays3):
    dt = TG._upload(tree5)
    assert dt.wide_nodes > 0
    _check(dt, tree5, *rays3, "two-level image")
    _check(dt, tree5, *rays3, "stop_thresh 0, background 0.25", stop_thresh=0.0, background_brightness=0.25)


def test_one_level_image(tree5, rays3):
    os.environ["RTO_NO_WIDE"] = "1"
    try:
        dt = TG._upload(tree5)
    finally:
        del os.environ["RTO_NO_WIDE"]
    assert dt.wide_nodes == 0
    _check(dt, tree5, *rays3, "one-level image")


def test_child_walk_on_an_n4_tree():
    from test_query import _n4_tree
    tree = _n4_tree()
    o, d = TH.rays_of([rcam(W, H, p) for p in synth.orbit_poses(4)[:3]])
    _check(TG._upload(tree), tree, o, d, "child[]", floor=100)


def test_depth_6_with_wide_nodes():
    tree = synth.make_tree(6, 9, seed=7)
    dt = TG._upload(tree)
    assert dt.wide_nodes > 0 and dt.max_depth == 6
    o, d = TH.rays_of([rcam(47, 41, p) for p in synth.orbit_poses(4)[:2]])
    _check(dt, tree, o, d, "depth 6")


def test_a_relaid_file_node_old(tree5, rays3):
    tree = synth.shuffle_nodes(tree5, seed=3)
    _check(TG._upload(tree), tree, *rays3, "shuffled")


def test_ndc_with_a_cropped_render_bbox(tree5):
    dt = TG._upload(tree5)
    ndc = (64.0, 48.0, 50.0)
    dt.set_ndc(*ndc)
    poses = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2), (0.0, -0.1, 0.4))]
    o, d = TH.rays_of([rcam(W, H, p, fx=18.0) for p in poses])
    _check(dt, tree5, o, d, "NDC, cropped", ndc=ndc, render_bbox=[0.1, 0.1, 0.0, 0.9, 0.9, 1.0], floor=300)


@pytest.mark.parametrize("fmt", TH.FORMATS)
def test_every_format(fmt, tree5, rays3):
    tree = rgba_tree(tree5) if fmt == "RGBA" else (tree5 if fmt == "SH9" else synth.make_tree(5, int(fmt[2:]), seed=7))
    _check(TG._upload(tree), tree, *rays3, fmt)


# ------------------------------------------------------------------ 2. splits, a second stream, offset buffers
@pytest.fixture(scope="module")
def cam_case(tree5, rays3):
    """(the device tree, the tree, params, origins, dirs, targets, the host twin's (out, grad, stats, touched))"""
    o, d = rays3
    params = TH.perturbed_params(tree5)
    tg = TH.noisy(TH.host_fit(tree5).render_rays(o, d))
    tg[W * H + 3 * W + 4, 1] = np.nan
    want = TS.call_touched(tree5, params, o, d, tg)
    TS.check_marks(tree5, params, want[1], want[3])
    return TG._upload(tree5), tree5, params, o, d, tg, want


def test_splits_accumulate_into_the_bitmap(cam_case):
    import torch
    dt, tree, params, o, d, tg, want = cam_case
    n = o.shape[0]
    assert n % 64 != 0
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((n, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    touched = torch.zeros(want[3].size, dtype=torch.int32, device="cuda")
    at = 0
    for k in (0, 1, 63, 64, 65, 257, n - 450):
        _dev(dt, tree, params, o[at:at + k], d[at:at + k], tg[at:at + k], grad=grad, stats=stats, out=out[at:at + k], touched=touched)
        at += k
    assert at == n
    _same(_np((out, grad, stats, touched)), want, "splits")
    perm = np.random.default_rng(5).permutation(n)
    po, pg, ps, pt = _np(_dev(dt, tree, params, o[perm], d[perm], tg[perm]))
    back = np.empty_like(po)
    back[perm] = po
    _same((back, pg, ps, pt), want, "permuted")


def _off4(a, dtype=None):
    """the elements of the numpy array `a` in a device buffer that starts 4 bytes after a 16-byte boundary"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros(a.size + 9, dtype=src.dtype, device="cuda")
    shift = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4
    view = buf[shift:shift + a.size].view(a.shape)
    assert view.data_ptr() % 16 == 4
    view.copy_(src)
    return view


def test_buffers_4_bytes_off_a_16_byte_boundary_and_a_second_stream(cam_case):
    import torch
    dt, tree, params, o, d, tg, want = cam_case
    n, slots = o.shape[0], TS.n_slots(tree)
    p = _off4(params)
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = _off4(np.full((n, 3), SENTINEL, np.float32))
    touched = _off4(np.zeros(want[3].size, np.int32))
    R.fit_grad_rays(dt, p, _off4(o), _off4(d), _off4(tg), grad=grad, stats=stats, out=out, touched=touched)
    _same(_np((out, grad, stats, touched)), want, "offset buffers")
    # the list and the three steps on offset buffers against the twins on the same values
    want_list = SR.list_of(want[3], slots)
    for kind in ("sgd", "rmsprop", "adam"):
        t2 = _off4(want[3].view(np.int32))
        lst = _off4(np.full(slots, -1, np.int32))
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(R.fit.touched_scratch_bytes(slots) + 8, dtype=torch.uint8, device="cuda")[4:4 + R.fit.touched_scratch_bytes(slots)]
        R.touched_list(t2, slots, lst, count, scratch, clear=True)
        assert int(count.cpu()[0]) == want_list.size and not t2.any()
        assert np.array_equal(lst.cpu().numpy().view(np.uint32)[:want_list.size], want_list)
        rng = np.random.default_rng(3)
        m0 = (rng.normal(size=params.shape) * 1e-3).astype(np.float32)
        v0 = (rng.uniform(size=params.shape) * 1e-6).astype(np.float32)
        optim = R.fit_optim(kind, 0.01, TS.GRAD_SCALE, t=3)
        hp, hg, hm, hv = params.copy(), want[1].copy(), m0.copy(), v0.copy()
        R.step_sparse_host(hp, hg, want_list, np.array([want_list.size], np.uint64), optim, m=hm, v=hv)
        dp, dg, dm, dv = _off4(params), torch.from_numpy(want[1].copy()).cuda(), _off4(m0), _off4(v0)
        R.step_sparse(dp, dg, lst, count, optim, m=dm if kind == "adam" else None, v=dv if kind != "sgd" else None)
        assert np.array_equal(dp.cpu().numpy().view(np.uint32), hp.view(np.uint32)), kind
        assert not dg.any() and not hg.any()
        if kind == "adam":
            assert np.array_equal(dm.cpu().numpy().view(np.uint32), hm.view(np.uint32))
        if kind != "sgd":
            assert np.array_equal(dv.cpu().numpy().view(np.uint32), hv.view(np.uint32))
            assert np.count_nonzero(hv != v0) > 1000
    # a second stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _dev(dt, tree, params, o, d, tg, stream=side)
        lst = torch.full((slots,), -1, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(R.fit.touched_scratch_bytes(slots), dtype=torch.uint8, device="cuda")
        pp = torch.from_numpy(params).cuda()
        R.touched_list(got[3], slots, lst, count, scratch, clear=False, stream=side)
        R.step_sparse(pp, got[1], lst, count, R.fit_optim("sgd", TH.LR10), stream=side)
    side.synchronize()
    assert np.array_equal(got[3].cpu().numpy().view(np.uint32), want[3]) and not got[1].any()
    hp, hg = params.copy(), want[1].copy()
    R.sgd_step_host(hp, hg, TH.LR10)
    assert np.array_equal(pp.cpu().numpy().view(np.uint32), hp.view(np.uint32)), "second stream"


# ------------------------------------------------------------------ 3. the list
def device_list(words, clear, cap):
    import torch
    t = torch.from_numpy(words.view(np.int32).copy()).cuda()
    lst = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(R.fit.touched_scratch_bytes(TS.LIST_SLOTS), dtype=torch.uint8, device="cuda")
    R.touched_list(t, TS.LIST_SLOTS, lst, count, scratch, clear=clear)
    return lst.cpu().numpy().view(np.uint32), int(count.cpu()[0]), t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", ["all clear", "all set", "last valid slot", "only bits beyond slots", "random"])
def test_list_on_synthetic_bitmaps(name):
    assert R.fit.touched_block_words() == TS.BLOCK_WORDS
    TS.check_list(device_list, name, TS.list_patterns()[name])


def test_list_of_small_and_empty_bitmaps_and_count_zero():
    import torch
    for slots in (0, 1, 31, 32, 33):
        words = np.full(R.touched_words(slots), 0xFFFFFFFF, np.uint32)
        t = torch.from_numpy(words.view(np.int32).copy()).cuda() if slots else torch.zeros(0, dtype=torch.int32, device="cuda")
        lst = torch.full((40,), -1, dtype=torch.int32, device="cuda")
        count = torch.full((1,), 99, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(R.fit.touched_scratch_bytes(slots), dtype=torch.uint8, device="cuda")
        R.touched_list(t, slots, lst, count, scratch, clear=True)
        assert int(count.cpu()[0]) == slots and not t.any()
        assert np.array_equal(lst.cpu().numpy()[:slots], np.arange(slots)) and (lst.cpu().numpy()[slots:] == -1).all()
    # count == 0: the step does nothing
    p = torch.ones((5, 2, 2, 2, 4), dtype=torch.float32, device="cuda")
    g = torch.full((5, 2, 2, 2, 4), 1 << 36, dtype=torch.int64, device="cuda")
    v = torch.zeros_like(p)
    R.step_sparse(p, g, torch.zeros(40, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                  R.fit_optim("rmsprop", 0.5), v=v)
    assert (p == 1).all() and (g == 1 << 36).all() and not v.any()
    # an entry >= slots is skipped; a count beyond the capacity is cut
    R.step_sparse(p, g, torch.tensor([40, 3, -1], dtype=torch.int32, device="cuda"), torch.tensor([9], dtype=torch.int64, device="cuda"),
                  R.fit_optim("sgd", 0.5))
    want = np.ones((40, 4), np.float32)
    want[3] = 0.5
    assert np.array_equal(p.cpu().numpy().reshape(40, 4), want) and np.count_nonzero(g.cpu().numpy()) == 39 * 4


# ------------------------------------------------------------------ 4. the SGD identity, ten steps
def test_sparse_sgd_step_leaves_the_dense_device_steps_bytes(cam_case):
    import torch
    dt, tree, params, o, d, tg, want = cam_case
    a = R.TreeFit(dt, tree.data)
    b = R.TreeFit(dt, tree.data, sparse=True)
    for f in (a, b):
        f.params.copy_(torch.from_numpy(params))
        f.accumulate_rays(o, d, tg)
    assert np.array_equal(b.grad.cpu().numpy(), a.grad.cpu().numpy()) and np.array_equal(b.touched.cpu().numpy().view(np.uint32), want[3])
    a.step(TH.LR10)
    b.step(TH.LR10)
    assert np.array_equal(a.params.cpu().numpy().view(np.uint32), b.params.cpu().numpy().view(np.uint32))
    assert not a.grad.any() and not b.grad.any() and not b.touched.any() and b.t == 1
    assert int(b.count.cpu()[0]) == SR.bits_of(want[3], TS.n_slots(tree)).sum()
    assert np.count_nonzero(b.params.cpu().numpy() != params) > 1000
    # accumulate(cams, targets) of a sparse fit goes through the cameras' rays: the camera entry's bytes
    planes = [torch.from_numpy(x).cuda() for x in np.ascontiguousarray(tg.reshape(3, H, W, 3))]
    a.accumulate(TH.cams3(), planes)
    b.accumulate(TH.cams3(), planes)
    assert np.array_equal(b.grad.cpu().numpy(), a.grad.cpu().numpy()) and np.array_equal(b.stats.cpu().numpy(), a.stats.cpu().numpy())


@pytest.mark.parametrize("kind,lr", [("rmsprop", TS.LR_RMSPROP), ("adam", TS.LR_ADAM)])
def test_ten_steps_give_the_hosts_loss_words_params_and_moments(kind, lr):
    import torch
    t, o, d, tg, batches = TH.sgd_rays()
    words_h, hf, _ = TS.ten_steps_sparse_host(kind, lr, t, o, d, tg, batches)
    df = R.TreeFit(TG._upload(t), t.data, optimizer=kind)
    df.params.copy_(torch.from_numpy(TH.start_params(t)))
    od, dd, td = (torch.from_numpy(a).cuda() for a in (o, d, tg))
    words_d = []
    for epoch in batches:
        for idx in epoch:
            i = torch.from_numpy(idx).cuda()
            df.accumulate_rays(od[i], dd[i], td[i])
            df.step(lr, grad_scale=TS.GRAD_SCALE)
        words_d.append(int(df.stats.cpu()[0]))
        assert df.loss()[1] == 5 * TH.BATCH
    assert words_d == words_h and words_d[1] < words_d[0], (words_d, words_h)
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), hf.params.view(np.uint32))
    assert np.array_equal(df.v.cpu().numpy().view(np.uint32), hf.v.view(np.uint32))
    if kind == "adam":
        assert np.array_equal(df.m.cpu().numpy().view(np.uint32), hf.m.view(np.uint32))
    assert not df.grad.any() and not df.touched.any() and df.t == 10


def test_a_step_between_two_renders_changes_neither_the_frames_nor_the_rng(cam_case):
    import torch
    dt, tree, params, o, d, tg, want = cam_case
    cam = rcam(47, 47, synth.orbit_poses(4)[1])
    opt = R.RenderOptions(spp=6, denoise=False)

    def two_frames(between):
        ctx = R.RenderContext(cam.width, cam.height)
        ctx.rng_seed()
        R.launch_renderer(dt, cam, opt, ctx)
        a = ctx.download_aux()
        if between:
            f = R.TreeFit(dt, tree.data, optimizer="adam")
            f.params.copy_(torch.from_numpy(params))
            f.accumulate_rays(o, d, tg)
            assert np.array_equal(f.touched.cpu().numpy().view(np.uint32), want[3])
            f.step(0.01, grad_scale=TS.GRAD_SCALE)
            assert f.v.any()
        ctx.rng_advance()
        R.launch_renderer(dt, cam, opt, ctx)
        return a, ctx.download_aux(), ctx.rng_get()

    a0, b0, r0 = two_frames(False)
    a1, b1, r1 = two_frames(True)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))
    assert tuple(r0) == tuple(r1)


# ------------------------------------------------------------------ 5. refusals
def test_device_refusals(tree5, rays3):
    import torch
    dt = TG._upload(tree5)
    slots = TS.n_slots(tree5)
    o, d = (torch.from_numpy(a[:64].copy()).cuda() for a in rays3)
    params = torch.from_numpy(TH.perturbed_params(tree5)).cuda()
    grad = torch.zeros(params.shape, dtype=torch.int64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    tg = torch.full((64, 3), 0.5, device="cuda")
    out = torch.zeros((64, 3), device="cuda")
    touched = torch.zeros(R.touched_words(slots) + 1, dtype=torch.int32, device="cuda")
    co = R.RenderOptions().to_c()
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    host_words = np.zeros(R.touched_words(slots), np.uint32)

    def refused(call, prefix, text, **kw):
        rc = call(**kw)
        msg = lib().rto_last_error().decode()
        assert rc == -1 and text in msg and msg.startswith(prefix), (rc, msg, text)

    def raw(tree=dt._h, params=params, origins=o, dirs=d, targets=tg, out=out, n=64, grad=grad, stats=stats, touched=touched):
        return lib().rto_tree_fit_grad_rays_touched(tree, ptr(params), ptr(origins), ptr(dirs), ptr(targets), ptr(out), n, C.byref(co),
                                                    ptr(grad), ptr(stats), ptr(touched), None)

    w = "rto_tree_fit_grad_rays_touched: "
    refused(raw, w, "null tree", tree=None)
    refused(raw, w, "null grad: a forward-only call uses the entry without the bitmap", grad=None)
    refused(raw, w, "null touched", touched=None)
    refused(raw, w, "touched must be 4-byte aligned", touched=touched.data_ptr() + 2)
    refused(raw, w, "touched overlaps params", touched=params.data_ptr() + 64)
    refused(raw, w, "touched overlaps grad", touched=grad.data_ptr())
    refused(raw, w, "touched overlaps stats", touched=stats.data_ptr() + 8)
    refused(raw, w, "touched overlaps origins", touched=o.data_ptr())
    refused(raw, w, "touched overlaps dirs", touched=d.data_ptr() + 4)
    refused(raw, w, "touched overlaps targets", touched=tg.data_ptr())
    refused(raw, w, "touched overlaps out", touched=out.data_ptr() + 8)
    refused(raw, w, "touched is not memory of the tree's device", touched=host_words.ctypes.data)
    refused(raw, w, "null targets with grad or stats set", targets=None)
    refused(raw, w, "grad must be 8-byte aligned", grad=grad.data_ptr() + 4)
    torch.cuda.synchronize()
    assert not grad.any() and not stats.any() and not out.any() and not touched.any(), "a refused call wrote"
    assert raw(origins=None, dirs=None, out=None, n=0) == 0  # n == 0 launches nothing

    lst = torch.zeros(16, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    nbytes = R.fit.touched_scratch_bytes(slots)
    scratch = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    host16 = np.zeros(16, np.uint64)

    def raw_list(touched=touched, slots=slots, list_=lst, cap=16, count=count, scratch=scratch, scratch_bytes=nbytes):
        return lib().rto_fit_touched_list(ptr(touched), slots, 0, ptr(list_), cap, ptr(count), ptr(scratch), scratch_bytes, None)

    w = "rto_fit_touched_list: "
    refused(raw_list, w, "null touched", touched=None)
    refused(raw_list, w, "null count", count=None)
    refused(raw_list, w, "null scratch", scratch=None)
    refused(raw_list, w, "slots must be in [0, 2^31)", slots=2 ** 31)
    refused(raw_list, w, "list_capacity must be >= 0", cap=-1)
    refused(raw_list, w, "null list with list_capacity > 0", list_=None)
    refused(raw_list, w, "scratch_bytes is below rto_fit_touched_scratch_bytes(slots)", scratch_bytes=nbytes - 1)
    refused(raw_list, w, "scratch must be 4-byte aligned", scratch=scratch.data_ptr() + 2)
    refused(raw_list, w, "list must be 4-byte aligned", list_=lst.data_ptr() + 2)
    refused(raw_list, w, "count must be 8-byte aligned", count=count.data_ptr() + 4)
    for key in ("touched", "list_", "count", "scratch"):
        refused(raw_list, w, "must be memory of one device", **{key: host16.ctypes.data})
    assert raw_list() == 0

    m, v = torch.zeros_like(params), torch.zeros_like(params)
    D = int(params.shape[-1])
    host_p = np.zeros(tuple(params.shape), np.float32)

    def raw_step(params=params, grad=grad, m=m, v=v, slots=slots, row=D, list_=lst, count=count, cap=16, kind=2, opt=True):
        o_ = CFitOptim(kind, 0.1, 1.0, 0.9, 0.999, 1e-8, 0.1, 0.001)
        return lib().rto_fit_step_sparse(ptr(params), ptr(grad), ptr(m), ptr(v), slots, row, ptr(list_), ptr(count), cap,
                                         C.byref(o_) if opt else None, None)

    w = "rto_fit_step_sparse: "
    for name, key in (("params", "params"), ("grad", "grad"), ("list", "list_"), ("count", "count")):
        refused(raw_step, w, "null " + name, **{key: None})
    refused(raw_step, w, "null options", opt=False)
    refused(raw_step, w, "row must be >= 1", row=0)
    refused(raw_step, w, "unknown kind 7", kind=7)
    refused(raw_step, w, "null m: RTO_FIT_ADAM keeps a first moment", m=None)
    refused(raw_step, w, "null v: RTO_FIT_RMSPROP and RTO_FIT_ADAM keep a second moment", v=None, kind=1)
    refused(raw_step, w, "params must be 4-byte aligned", params=params.data_ptr() + 2)
    refused(raw_step, w, "grad must be 8-byte aligned", grad=grad.data_ptr() + 4)
    refused(raw_step, w, "v must be 4-byte aligned", v=v.data_ptr() + 1)
    for key in ("params", "m", "v"):
        refused(raw_step, w, "must be memory of one device", **{key: host_p.ctypes.data})
    refused(raw_step, w, "must be memory of one device", list_=host16.ctypes.data)
    assert raw_step(m=host_p.ctypes.data, v=host_p.ctypes.data, kind=0) == 0  # (m and v are not read by SGD)
    torch.cuda.synchronize()
    assert not m.any() and not v.any() and not grad.any()
    with pytest.raises(R.RtoError):
        R.fit_grad_rays(dt, params, o, d, tg, grad=grad, touched=touched[:3])
    with pytest.raises(R.RtoError):
        R.TreeFit(dt, tree5.data, optimizer="lion")


# ------------------------------------------------------------------ 6. the tool
def test_optimize_octree_backends_write_the_same_bytes_with_adam(tmp_path, tree5):
    js, pert = TH.write_dataset(tmp_path, tree5)
    out = {}
    for backend in ("hip", "cpu"):
        d = tmp_path / backend
        assert optimize_octree.main([pert, "--poses", js, "--epochs", "2", "--val_poses", js, "--backend", backend, "--out_dir", str(d),
                                     "--optimizer", "adam", "--lr", "0.01", "--batch_rays", str(TH.BATCH), "--seed", "1"]) == 0
        out[backend] = (d / "pert.npz").read_bytes()
    assert out["hip"] == out["cpu"], "the optimised files differ"
    with np.load(tmp_path / "hip" / "pert.npz") as f, np.load(pert) as z:
        assert np.count_nonzero(f["data"].view(np.uint16) != z["data"].view(np.uint16)) > 1000
