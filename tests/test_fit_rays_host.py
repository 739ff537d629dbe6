"""The tree fit on rays the caller supplies, on the host (include/rto.h "tree fit", rto_fit_grad_rays_host; no GPU).  Every
comparison is bit for bit: the host twin against the numpy restatement of the set-up (tests/fit_rays_ref.py); the twin on the
rays of cameras against fit_grad_host on the cameras, in any order, split and thread count; free, degenerate and masked rays;
forward only; the refusals by their texts; ten SGD steps on shuffled 257-ray batches; optimize_octree --batch_rays."""
import ctypes as C
import os

import numpy as np
import pytest

import fit_rays_ref as RR
import fit_ref as FR
import orc
import rt_octree_amd as R
from helpers import FRAME_ANISO, rcam, reframe, reframe_pose, rgba_tree
from rt_octree_amd import optimize_octree, synth
from rt_octree_amd._lib import check, lib

E_INVALID = -1
W, H = 23, 19  # odd on purpose (tests/test_fit_host.py)
FORMATS = ["RGBA", "SH1", "SH4", "SH9", "SH16", "SH25"]
LR10 = 2.0  # tests/test_fit_host.py chose it
BATCH = 257
FREE_SEED = 11  # chosen so that at least a quarter of the free rays carry a gradient (asserted below)
SENTINEL = np.float32(-7.0)


def make5(fmt):
    """synth.make_tree(5, .) of a format"""
    if fmt == "RGBA":
        return rgba_tree(synth.make_tree(5, 9, seed=7))
    return synth.make_tree(5, int(fmt[2:]), seed=7)


def poses3():
    return synth.orbit_poses(4)[:3]


def cams3():
    return [rcam(W, H, p) for p in poses3()]


def rays_of(cams):
    """volrend.camera_rays of the cameras, one after the other -> (origins, dirs) float32 [n,3]"""
    pairs = [R.camera_rays(c) for c in cams]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def host_fit(t, ndc=None, threads=8, **optkw):
    return R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, options=R.RenderOptions(**optkw), ndc=ndc, threads=threads)


def noisy(colours, seed=1):
    rng = np.random.default_rng(seed)
    return np.clip(colours * 0.8 + rng.uniform(0, 0.2, colours.shape), 0, 1).astype(np.float32)


def perturbed_params(t):
    p = t.data.astype(np.float32)
    p[..., :-1] *= np.float32(0.75)
    p[..., -1] *= np.float32(0.9)
    return p


def call_rays(t, params, o, d, tg, ndc=None, threads=8, want_grad=True, want_stats=True, grad=None, stats=None, out=None, **optkw):
    """one rto_fit_grad_rays_host call -> (out, grad, stats); out starts as SENTINEL"""
    grad = (np.zeros(params.shape, np.int64) if grad is None else grad) if want_grad else None
    stats = np.zeros(2, np.int64) if stats is None else stats
    out = np.full((o.shape[0], 3), SENTINEL, np.float32) if out is None else out
    R.fit_grad_rays_host(t.child, t.data, params, t.scale, t.offset, t.data_format, o, d, tg, R.RenderOptions(**optkw), ndc=ndc,
                         threads=threads, grad=grad, stats=stats if (tg is not None and want_stats) else None, out=out)
    return out, grad, stats


def restated(t, params, o, d, tg, ndc=None, **optkw):
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)
    bg = optkw.pop("background_brightness", 1.0)
    return RR.restate(ht, params, o, d, tg, ndc=ndc, bg=bg, out=np.full((o.shape[0], 3), SENTINEL, np.float32), **optkw)


def same(a, b, what=""):
    (ao, ag, as_), (bo, bg, bs) = a, b
    assert np.array_equal(ao.view(np.uint32), bo.view(np.uint32)), "%s: %d out words differ" % (what, np.count_nonzero(ao.view(np.uint32) != bo.view(np.uint32)))
    assert (ag is None and bg is None) or np.array_equal(ag, bg), "%s: %d grad words differ" % (what, np.count_nonzero(ag != bg))
    assert np.array_equal(as_, bs), "%s: stats %s vs %s" % (what, as_, bs)


# ------------------------------------------------------------------ 1. the twin == the restatement, on the rays of cameras
@pytest.mark.parametrize("fmt", FORMATS)
def test_twin_equals_the_restatement_in_every_format(fmt):
    t = make5(fmt)
    o, d = rays_of(cams3())
    params = perturbed_params(t)
    tg = noisy(host_fit(t).render_rays(o, d))
    tg[400, 1] = np.nan  # one masked ray
    got = call_rays(t, params, o, d, tg)
    same(got, restated(t, params, o, d, tg), fmt)
    assert got[2][1] == o.shape[0] - 1 and np.count_nonzero(got[1]) > 1000 and (got[0][400] == SENTINEL).all()
    assert not got[1][t.child != 0].any(), "an internal slot carries a gradient"


@pytest.mark.parametrize("name", ["ndc", "reframed", "bbox_crop", "camera_inside"])
def test_variants_equal_the_restatement(name):
    t = synth.make_tree(5, 9, seed=7)
    ndc, kw = None, {}
    if name == "ndc":
        ndc = (64.0, 48.0, 50.0)
        pose = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2))]
        cams = [rcam(W, H, p, fx=50.0) for p in pose]
    elif name == "reframed":
        t0, t = t, reframe(t, *FRAME_ANISO)
        cams = [rcam(W, H, reframe_pose(p, t0, t)) for p in poses3()[:2]]
    elif name == "bbox_crop":
        cams, kw = cams3()[:2], {"render_bbox": [0.2, 0.1, 0.3, 0.8, 0.9, 0.7], "stop_thresh": 0.0, "background_brightness": 0.25}
    else:
        cams = [rcam(W, H, synth.look_at_c2w((-1.2, -1.2, 1.2)))]
    o, d = rays_of(cams)
    params = perturbed_params(t)
    tg = noisy(host_fit(t, ndc=ndc, **kw).render_rays(o, d))
    got = call_rays(t, params, o, d, tg, ndc=ndc, **kw)
    same(got, restated(t, params, o, d, tg, ndc=ndc, **kw), name)
    assert np.count_nonzero(got[1]) > 500, "the variant marches nothing"
    # and the camera entry gives these bytes
    images = [np.zeros((H, W, 3), np.float32) for _ in cams]
    grad, stats = np.zeros(params.shape, np.int64), np.zeros(2, np.int64)
    R.fit_grad_host(t.child, t.data, params, t.scale, t.offset, t.data_format, cams, list(tg.reshape(len(cams), H, W, 3)),
                    R.RenderOptions(**kw), ndc=ndc, threads=8, grad=grad, stats=stats, images=images)
    same(got, (np.concatenate([i.reshape(-1, 3) for i in images]), grad, stats), name + " against the cameras")


# ------------------------------------------------------------------ 2. camera rays == the camera entry, in any order and split
@pytest.fixture(scope="module")
def cam_case():
    """(tree, params, cameras, origins, dirs, targets [n,3], the camera entry's (out, grad, stats)) -- computed once, read only"""
    t = make5("SH9")
    cams = cams3()
    o, d = rays_of(cams)
    params = perturbed_params(t)
    tg = noisy(host_fit(t).render_rays(o, d))
    tg[W * H + 3 * W + 4, 1] = np.nan  # pixel (4, 3) of the second camera
    images = [np.full((H, W, 3), SENTINEL, np.float32) for _ in cams]
    grad, stats = np.zeros(params.shape, np.int64), np.zeros(2, np.int64)
    R.fit_grad_host(t.child, t.data, params, t.scale, t.offset, t.data_format, cams, list(tg.reshape(3, H, W, 3)), R.RenderOptions(),
                    threads=8, grad=grad, stats=stats, images=images)
    want = (np.concatenate([i.reshape(-1, 3) for i in images]), grad, stats)
    for a in (params, o, d, tg) + want:
        a.setflags(write=False)
    return t, params, cams, o, d, tg, want


def test_camera_rays_give_the_camera_entrys_bytes(cam_case):
    t, params, cams, o, d, tg, want = cam_case
    n = o.shape[0]
    assert want[2][1] == n - 1 and np.count_nonzero(want[1]) > 1000
    same(call_rays(t, params, o, d, tg), want, "as given")
    for threads in (1, 3, 8):
        same(call_rays(t, params, o, d, tg, threads=threads), want, "threads %d" % threads)
    perm = np.random.default_rng(5).permutation(n)
    po, pg, ps = call_rays(t, params, o[perm], d[perm], tg[perm], threads=3)
    back = np.empty_like(po)
    back[perm] = po
    same((back, pg, ps), want, "permuted")
    # split into calls of 1, 63, 64, 65 rays and the rest, accumulating
    grad, stats, out = np.zeros(params.shape, np.int64), np.zeros(2, np.int64), np.full((n, 3), SENTINEL, np.float32)
    at = 0
    for k in (1, 63, 64, 65, n - 193):
        s = slice(at, at + k)
        call_rays(t, params, o[s], d[s], tg[s], grad=grad, stats=stats, out=out[s], threads=3)
        at += k
    assert at == n
    same((out, grad, stats), want, "split")
    # no ray: nothing changes
    g0, s0 = grad.copy(), stats.copy()
    call_rays(t, params, o[:0], d[:0], tg[:0], grad=g0, stats=s0)
    assert np.array_equal(g0, grad) and np.array_equal(s0, stats)


def test_forward_only_and_without_targets(cam_case):
    t, params, cams, o, d, tg, want = cam_case
    fo, fg, fs = call_rays(t, params, o, d, tg, want_grad=False)
    assert fg is None
    same((fo, None, fs), (want[0], None, want[2]), "grad == NULL")
    no, _, _ = call_rays(t, params, o, d, None, want_grad=False)
    m = ~np.isnan(tg).any(1)
    assert np.array_equal(no[m].view(np.uint32), want[0][m].view(np.uint32)) and (no[~m] != SENTINEL).all(), "targets == NULL"
    # out == NULL: the same grad and stats
    grad, stats = np.zeros(params.shape, np.int64), np.zeros(2, np.int64)
    R.fit_grad_rays_host(t.child, t.data, params, t.scale, t.offset, t.data_format, o, d, tg, threads=8, grad=grad, stats=stats)
    assert np.array_equal(grad, want[1]) and np.array_equal(stats, want[2])
    # the classes
    hf = host_fit(t)
    hf.params[...] = params
    hf.accumulate_rays(o, d, tg)
    assert np.array_equal(hf.grad, want[1]) and np.array_equal(hf.stats, want[2])
    loss = hf.loss()
    assert loss == (float(int(want[2][0])) / FR.FIX, int(want[2][1])) and hf.evaluate_rays(o, d, tg) == loss
    assert np.array_equal(hf.render_rays(o, d)[m].view(np.uint32), want[0][m].view(np.uint32))


# ------------------------------------------------------------------ 3. free rays
def free_rays(t, n=2000, seed=FREE_SEED):
    """n seeded rays through the box of `t` in world space: from outside towards a point inside, a fifth from origins inside
    the box, a fifth parallel to an axis (two zero components); a third each of length 1, 1e-3 and 1e3"""
    rng = np.random.default_rng(seed)
    sc, of = t.scale.astype(np.float64), t.offset.astype(np.float64)
    to_world = lambda p: (p - of) / sc  # noqa: E731
    aim = rng.uniform(0.2, 0.8, (n, 3))
    u = rng.normal(size=(n, 3))
    org = 0.5 + 1.6 * u / np.linalg.norm(u, axis=1, keepdims=True)  # tree units
    kind = rng.integers(0, 5, n)
    inside = kind == 0
    org[inside] = rng.uniform(0.05, 0.95, (int(inside.sum()), 3))
    dirs = to_world(aim) - to_world(org)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    axis = np.flatnonzero(kind == 1)
    ax = rng.integers(0, 3, axis.size)
    sign = rng.choice([-1.0, 1.0], axis.size)
    org[axis] = aim[axis]
    org[axis, ax] = 0.5 - sign * 1.3
    dirs[axis] = 0.0
    dirs[axis, ax] = sign
    length = np.array([1.0, 1e-3, 1e3])[rng.integers(0, 3, n)]
    return to_world(org).astype(np.float32), (dirs * length[:, None]).astype(np.float32), kind


def test_free_rays():
    t = synth.make_tree(4, 4, seed=7)
    o, d, kind = free_rays(t)
    assert (kind == 0).sum() > 200 and ((d == 0).sum(1) == 2).sum() > 200
    params = perturbed_params(t)
    tg = noisy(host_fit(t).render_rays(o, d), seed=2)
    got = call_rays(t, params, o, d, tg)
    same(got, restated(t, params, o, d, tg), "free rays")
    # scaling a direction by a power of two changes no bit
    for s in (4.0, 0.125):
        same(call_rays(t, params, o, d * np.float32(s), tg), got, "dirs x %g" % s)
    # at least a quarter of the rays carry a gradient: the test does not pass on rays that all miss
    carrying = 0
    g1 = np.zeros(params.shape, np.int64)
    for i in range(o.shape[0]):
        R.fit_grad_rays_host(t.child, t.data, params, t.scale, t.offset, t.data_format, o[i:i + 1], d[i:i + 1], tg[i:i + 1], grad=g1)
        if g1.any():
            carrying += 1
            g1[...] = 0
    print("free rays with a gradient: %d of %d" % (carrying, o.shape[0]))
    assert 4 * carrying >= o.shape[0]


# ------------------------------------------------------------------ 4. degenerate and masked rays
def degenerate_rays(t):
    """(origins, dirs, targets, bad): 64 rays of a camera's middle rows with a zero direction, a NaN direction and an infinite
    origin among them (rows `bad`), and one NaN target (row 9)"""
    o, d = rays_of(cams3()[:1])
    at = (H // 2) * W
    o, d = o[at:at + 64].copy(), d[at:at + 64].copy()
    d[3] = 0.0
    d[17, 1] = np.nan
    o[40, 2] = np.inf
    tg = np.full((64, 3), 0.5, np.float32)
    tg[9, 0] = np.nan
    return o, d, tg, [3, 17, 40]


def test_degenerate_and_masked_rays():
    t = make5("SH9")
    o, d, tg, bad = degenerate_rays(t)
    params = perturbed_params(t)
    got = call_rays(t, params, o, d, tg, background_brightness=0.25)
    same(got, restated(t, params, o, d, tg, background_brightness=0.25), "degenerate")
    out, grad, stats = got
    assert (out[bad] == np.float32(0.25)).all(), "a ray that is not marched gives bg"
    assert stats[1] == 63 and (out[9] == SENTINEL).all(), "a NaN target is not counted and its out keeps its bytes"
    # the degenerate rays add no gradient: without them the same grad, and their loss is that of out = bg
    keep = np.setdiff1d(np.arange(64), bad)
    _, g2, s2 = call_rays(t, params, o[keep], d[keep], tg[keep], background_brightness=0.25)
    assert np.array_equal(g2, grad) and s2[1] == 60 and np.count_nonzero(grad) > 50
    r = np.float32(0.25) - np.float32(0.5)
    assert stats[0] - s2[0] == 3 * int(FR.to_fixed((r * r + r * r) + r * r))


# ------------------------------------------------------------------ 5. refusals
def test_refusal_texts():
    t = synth.make_tree(4, 4, seed=7)
    params = t.data.astype(np.float32)
    grad, stats = np.zeros(params.shape, np.int64), np.zeros(2, np.int64)
    n = 8
    buf = np.zeros((4, n + 1, 3), np.float32)  # origins, dirs, targets, out with room for a misaligned view
    buf[1] = 1.0
    pp, gp, sp = params.ctypes.data, grad.ctypes.data, stats.ctypes.data
    op, dp, tp, up = (buf[k].ctypes.data for k in range(4))
    sc = (C.c_float * 3)(*[float(v) for v in t.scale])
    of = (C.c_float * 3)(*[float(v) for v in t.offset])
    data = t.data.view(np.uint16)

    def raw(params=pp, origins=op, dirs=dp, targets=tp, out=up, n=n, opt=R.RenderOptions(), grad=gp, stats=sp, use_opt=True, child=t.child):
        co = opt.to_c()
        return lib().rto_fit_grad_rays_host(C.c_void_p(child.ctypes.data) if child is not None else None, C.c_void_p(data.ctypes.data), params,
                                            t.child.shape[0], 2, data.shape[-1], t.data_format.encode(), sc, of, None, origins, dirs, targets,
                                            out, n, C.byref(co) if use_opt else None, 0, grad, stats)

    def refused(text, **kw):
        rc = raw(**kw)
        msg = lib().rto_last_error().decode()
        assert rc == E_INVALID and text in msg and msg.startswith("rto_fit_grad_rays_host: "), (rc, msg, text)

    assert raw() == 0
    grad[...] = 0
    stats[...] = 0
    buf[3] = 0
    refused("null argument", child=None)
    refused("null params", params=None)
    refused("null options", use_opt=False)
    refused("null origins with n > 0", origins=None)
    refused("null dirs with n > 0", dirs=None)
    assert raw(origins=None, dirs=None, targets=None, out=None, n=0, grad=None, stats=None) == 0
    refused("n must be >= 0", n=-1)
    refused("params must be 4-byte aligned", params=pp + 2)
    for name, key, p in (("origins", "origins", op), ("dirs", "dirs", dp), ("targets", "targets", tp), ("out", "out", up)):
        refused(name + " must be 4-byte aligned", **{key: p + 1})
    refused("grad must be 8-byte aligned", grad=gp + 4)
    refused("stats must be 8-byte aligned", stats=sp + 4)
    refused("null targets with grad or stats set", targets=None)
    refused("null targets with grad or stats set", targets=None, grad=None)
    refused("params overlaps origins", origins=pp + 64)
    refused("params overlaps dirs", dirs=pp + 4 * (params.size - 1))
    refused("params overlaps targets", targets=pp)
    refused("params overlaps out", out=pp + 128)
    refused("grad overlaps origins", origins=gp + 8 * (grad.size - 1))
    refused("grad overlaps dirs", dirs=gp)
    refused("grad overlaps targets", targets=gp + 16)
    refused("grad overlaps out", out=gp + 8)
    refused("out overlaps origins", out=op + 12)
    refused("out overlaps dirs", out=dp)
    refused("out overlaps targets", out=tp + 12 * (n - 1))
    refused("rot_dirs is not read", opt=R.RenderOptions(rot_dirs=[0.0, 0.1, 0.0]))
    refused("basis_minmax is not read", opt=R.RenderOptions(basis_minmax=[0, 3]))
    assert not grad.any() and not stats.any() and not buf[3].any(), "a refused call wrote"
    # the Python wrapper's own checks (volrend._ray_tensor's rules on the host)
    o, d = buf[0][:n], buf[1][:n]
    args = (t.child, t.data, params, t.scale, t.offset, t.data_format)
    with pytest.raises(R.RtoError):
        R.fit_grad_rays_host(*args, o, d[:3])
    with pytest.raises(R.RtoError):
        R.fit_grad_rays_host(*args, o.astype(np.float64), d)
    with pytest.raises(R.RtoError):
        R.fit_grad_rays_host(*args, o, d, out=np.zeros((n, 4), np.float32))
    with pytest.raises(TypeError):
        R.fit_grad_rays_host(*args, o.tolist(), d)


# ------------------------------------------------------------------ 6. ten SGD steps on shuffled batches
def sgd_rays():
    """the tree, the ray table (origins, dirs, targets of three cameras: the unperturbed field's colours) and the ten batches:
    two epochs of five batches of 257 rays, each epoch's permutation drawn as optimize_octree draws it (seed 3)"""
    t = make5("SH9")
    o, d = rays_of(cams3())
    tg = host_fit(t).render_rays(o, d)
    batches = []
    for epoch in range(2):
        perm = np.random.Generator(np.random.PCG64(3 + epoch)).permutation(o.shape[0])
        batches.append([perm[b:b + BATCH] for b in range(0, 5 * BATCH, BATCH)])
    return t, o, d, tg, batches


def start_params(t):
    p = t.data.astype(np.float32)
    p[..., :-1] *= np.float32(0.5)
    p[..., -1] *= np.float32(0.8)
    return p


def ten_steps_host(t, o, d, tg, batches):
    """-> (the summed loss word of each epoch, the HostTreeFit after the ten steps)"""
    hf = host_fit(t)
    hf.params[...] = start_params(t)
    words = []
    for epoch in batches:
        for idx in epoch:
            hf.accumulate_rays(o[idx], d[idx], tg[idx])
            hf.step(LR10)
            assert not hf.grad.any()
        words.append(int(hf.stats[0]))
        assert hf.loss()[1] == 5 * BATCH
    return words, hf


def test_ten_sgd_steps_on_shuffled_batches_lower_the_loss():
    t, o, d, tg, batches = sgd_rays()
    words, hf = ten_steps_host(t, o, d, tg, batches)
    # the same sequence from the restatement: both loss words and the final params
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    p = start_params(t)
    want = []
    for epoch in batches:
        stats = np.zeros(2, np.int64)
        for idx in epoch:
            _, g, stats = RR.restate(ht, p, o[idx], d[idx], tg[idx], stats=stats)
            p = FR.sgd_step(p, g, LR10)
        want.append(int(stats[0]))
    print([round(w / FR.FIX, 4) for w in words])
    assert words == want and np.array_equal(hf.params.view(np.uint32), p.view(np.uint32))
    assert words[1] < words[0]


# ------------------------------------------------------------------ 7. the tool
def write_dataset(tmp_path, tree):
    """three 23 x 19 training images of `tree` and a perturbed tree file -> (the pose json, the tree file)"""
    cams = cams3()
    images = host_fit(tree).render(cams)
    os.makedirs(tmp_path / "test")
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), poses3())
    for i, im in enumerate(images):
        u8 = np.concatenate([np.clip(np.rint(im * 255), 0, 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
        u8[:2, :, 3] = 0  # some transparent rows: composited over the background
        u8 = np.ascontiguousarray(u8)
        check(lib().rto_image_write_png(str(tmp_path / "test" / ("r_%d.png" % i)).encode(), u8.ctypes.data, W, H))
    src = tree.save_npz(str(tmp_path / "tree.npz"))
    with np.load(src) as f:
        z = {k: f[k] for k in f.files}
    dd = tree.data.astype(np.float32)
    dd[..., :-1] *= 0.5
    z["data"] = dd.astype(np.float16)
    pert = str(tmp_path / "pert.npz")
    np.savez_compressed(pert, **z)
    return js, pert


def run_tool(tmp_path, name, pert, js, backend, *flags):
    out_dir = tmp_path / name
    assert optimize_octree.main([pert, "--poses", js, "--epochs", "2", "--lr", "4000", "--val_poses", js, "--backend", backend,
                                 "--out_dir", str(out_dir)] + list(flags)) == 0
    return (out_dir / "pert.npz").read_bytes()


def test_optimize_octree_batch_rays_on_the_cpu(tmp_path):
    tree = make5("SH9")
    js, pert = write_dataset(tmp_path, tree)
    run = lambda name, *flags: run_tool(tmp_path, name, pert, js, "cpu", *flags)  # noqa: E731
    plain = run("plain", "--batch_imgs", "2")
    assert run("zero", "--batch_imgs", "2", "--batch_rays", "0") == plain, "--batch_rays 0 is not the run without the flag"
    # one batch of all rays == one batch of all images: the order of the rays cannot change a bit
    assert run("all_rays", "--batch_imgs", "3", "--batch_rays", str(3 * W * H + 5)) == run("all_imgs", "--batch_imgs", "3")
    a = run("seed_a", "--batch_rays", str(BATCH), "--seed", "1")
    assert run("seed_a2", "--batch_rays", str(BATCH), "--seed", "1") == a, "two runs with one seed differ"
    assert run("seed_b", "--batch_rays", str(BATCH), "--seed", "2") != a, "another seed writes the same bytes"
    assert a != plain
    with np.load(tmp_path / "seed_a" / "pert.npz") as f:
        assert f["data"].dtype == np.float16 and f["data"].shape == tree.data.shape and np.array_equal(f["child"], tree.child)
    assert optimize_octree.main([pert, "--poses", js, "--batch_rays", "-1", "--out_dir", str(tmp_path / "bad")]) == 2
