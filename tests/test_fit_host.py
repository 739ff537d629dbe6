"""The tree fit on the host (include/rto.h "tree fit"; no GPU): the host twin's grad, stats and images against the numpy
restatement bit for bit and against the float64 model of the suite, its invariances (threads, splits, masked pixels, forward
only), the float64 model's own gradient against central differences, ten SGD steps, the support, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as FR
import orc
import rt_octree_amd as R
from helpers import FRAME_ANISO, rcam, reframe, reframe_pose, rgba_tree
from rt_octree_amd import synth
from rt_octree_amd._lib import CCamera, lib

E_INVALID, E_UNSUPPORTED, E_FORMAT = -1, -3, -6
W, H = 23, 19  # odd on purpose (at an even size a pixel column lies in a cell boundary of the tree)
FORMATS = ["RGBA", "SH1", "SH4", "SH9", "SH16", "SH25"]
# max |g32 - g64| / max |g64| of the twin against Model64, measured on this suite's trees (stop_thresh 0, three 23 x 19
# cameras), and the bound: twice that.  The twin is bit-reproducible; the margin covers the float64 model's libm.
GRAD_REL_MEASURED = {"RGBA": 1.44e-4, "SH1": 3.25e-5, "SH4": 5.14e-5, "SH9": 8.06e-5, "SH16": 9.02e-5, "SH25": 2.15e-5}
LR10 = 2.0  # the ten-step sequence: chosen on the CPU among 0.5, 2, 8, 32 (all decrease strictly; 2 leaves 50 % of the loss)


def make(fmt):
    """the suite's tree of a format: depth 5 for RGBA and SH9, depth 4 for the others"""
    if fmt == "RGBA":
        return rgba_tree(synth.make_tree(5, 9, seed=7))
    B = int(fmt[2:])
    return synth.make_tree(5 if B == 9 else 4, B, seed=7)


def poses3():
    return synth.orbit_poses(4)[:3]


def cams3(w=W, h=H):
    return [rcam(w, h, p) for p in poses3()]


def host_fit(t, ndc=None, threads=8, **optkw):
    return R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, options=R.RenderOptions(**optkw), ndc=ndc, threads=threads)


def noisy_targets(images, seed=1):
    rng = np.random.default_rng(seed)
    return [np.clip(i * 0.8 + rng.uniform(0, 0.2, i.shape), 0, 1).astype(np.float32) for i in images]


def call(t, params, cams, targets, ndc=None, threads=8, want_grad=True, want_images=True, grad=None, stats=None, **optkw):
    """one rto_fit_grad_host call -> (images, grad, stats)"""
    grad = (np.zeros(params.shape, np.int64) if grad is None else grad) if want_grad else None
    stats = np.zeros(2, np.int64) if stats is None else stats
    images = [np.zeros((c.height, c.width, 3), np.float32) for c in cams] if want_images else None
    R.fit_grad_host(t.child, t.data, params, t.scale, t.offset, t.data_format, cams, targets, R.RenderOptions(**optkw), ndc=ndc,
                    threads=threads, grad=grad, stats=stats if targets is not None else None, images=images)
    return images, grad, stats


def same_images(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def case():
    """per format: (tree, cameras, params, targets, (images, grad, stats) of the twin) -- computed once, never written"""
    memo = {}

    def get(fmt):
        if fmt not in memo:
            t = make(fmt)
            cams = cams3()
            hf = host_fit(t)
            targets = noisy_targets(hf.render(cams))
            targets[1][3, 4, 1] = np.nan  # one masked pixel
            got = call(t, hf.params, cams, targets)
            for a in (hf.params, got[1], got[2]) + tuple(targets) + tuple(got[0]):
                a.setflags(write=False)
            memo[fmt] = (t, cams, hf.params, targets, got)
        return memo[fmt]

    return get


# ------------------------------------------------------------------ 1. the numpy restatement, word for word
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_equals_the_numpy_restatement(case, fmt):
    t, cams, params, targets, (images, grad, stats) = case(fmt)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    ri, rg, rs = FR.restate(ht, params, cams, targets)
    assert same_images(images, ri), "images"
    assert np.array_equal(grad, rg), "%d grad words differ" % np.count_nonzero(grad != rg)
    assert np.array_equal(stats, rs), (stats, rs)
    assert stats[1] == 3 * W * H - 1 and stats[0] > 0 and np.count_nonzero(grad) > 1000
    assert not grad[t.child != 0].any(), "an internal slot carries a gradient"
    # the fixed-point sums stay far from a wrap: |q| <= 2^52 per contribution, 2^63 per word
    print(fmt, "max |grad word| 2^%.1f, loss word 2^%.1f" % (np.log2(np.abs(grad).max()), np.log2(stats[0])))
    assert np.abs(grad).max() < 2 ** 44 and stats[0] < 2 ** 50


@pytest.mark.parametrize("name", ["ndc", "reframed", "bbox_crop_stop_0", "camera_inside"])
def test_variants_equal_the_numpy_restatement(name):
    t = synth.make_tree(5, 9, seed=7)
    ndc, kw = None, {}
    if name == "ndc":
        ndc = (64.0, 48.0, 50.0)
        pose = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2))]
        cams = [rcam(W, H, p, fx=50.0) for p in pose]
    elif name == "reframed":
        t0, t = t, reframe(t, *FRAME_ANISO)
        cams = [rcam(W, H, reframe_pose(p, t0, t)) for p in poses3()[:2]]
    elif name == "bbox_crop_stop_0":
        cams, kw = cams3()[:2], {"render_bbox": [0.2, 0.1, 0.3, 0.8, 0.9, 0.7], "stop_thresh": 0.0, "background_brightness": 0.25}
    else:
        cams = [rcam(W, H, synth.look_at_c2w((-1.2, -1.2, 1.2)))]
    hf = host_fit(t, ndc=ndc, **kw)
    targets = noisy_targets(hf.render(cams))
    images, grad, stats = call(t, hf.params, cams, targets, ndc=ndc, **kw)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)
    rkw = {k: v for k, v in kw.items() if k != "background_brightness"}
    ri, rg, rs = FR.restate(ht, hf.params, cams, targets, ndc=ndc, bg=kw.get("background_brightness", 1.0), **rkw)
    assert same_images(images, ri) and np.array_equal(grad, rg) and np.array_equal(stats, rs)
    assert np.count_nonzero(grad) > 500, "the variant marches nothing"


# ------------------------------------------------------------------ 2. invariances
def test_threads_splits_masks_and_forward_only(case):
    t, cams, params, targets, (images, grad, stats) = case("SH9")
    for threads in (1, 3):
        i2, g2, s2 = call(t, params, cams, targets, threads=threads)
        assert same_images(images, i2) and np.array_equal(grad, g2) and np.array_equal(stats, s2), threads
    # the cameras split over two calls, accumulating
    i_a, g, s = call(t, params, cams[:1], targets[:1])
    i_b, g, s = call(t, params, cams[1:], targets[1:], grad=g, stats=s)
    assert same_images(images, i_a + i_b) and np.array_equal(grad, g) and np.array_equal(stats, s)
    # no camera: nothing changes
    _, g0, s0 = call(t, params, [], [], grad=g.copy(), stats=s.copy())
    assert np.array_equal(g0, g) and np.array_equal(s0, s)
    # forward only: grad == NULL gives the same images and stats; without targets the same images again
    i3, g3, s3 = call(t, params, cams, targets, want_grad=False)
    assert g3 is None and same_images(images, i3) and np.array_equal(stats, s3)
    i4, _, _ = call(t, params, cams, None, want_grad=False)
    assert all(np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32)) for a, b, m in
               zip(i4, images, [~np.isnan(x).any(-1) for x in targets]))
    # the masked pixel: not written, not counted; masking another pixel removes that pixel's share and nothing else
    assert not images[1][3, 4].any() and i4[1][3, 4].any()
    more = [x.copy() for x in targets]
    more[0][5, 6, 2] = np.nan
    i5, g5, s5 = call(t, params, cams, more)
    one = rcam(W, H, poses3()[0])
    solo_t = np.full((H, W, 3), np.nan, np.float32)
    solo_t[5, 6] = targets[0][5, 6]
    _, g_px, s_px = call(t, params, [one], [solo_t])
    assert s_px[1] == 1 and np.array_equal(g5 + g_px, grad) and np.array_equal(s5 + s_px, stats)
    i5[0][5, 6] = images[0][5, 6]
    assert same_images(i5, images)


# ------------------------------------------------------------------ 3. the float64 model
@pytest.fixture(scope="module")
def model_case():
    memo = {}

    def get(fmt):
        if fmt not in memo:
            t = make(fmt)
            cams = cams3()
            model = FR.Model64(t, poses3(), W, H, cams[0].fx, cams[0].fx)
            memo[fmt] = (t, cams, model)
        return memo[fmt]

    return get


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_twin_against_the_float64_model(case, model_case, fmt):
    """stop_thresh = 0 (the model composites every segment).  Image: max |delta| < 1e-3, the bound of the leaf-weights test
    against the same model.  Gradient: max |g32 - g64| / max |g64| over all parameters within twice GRAD_REL_MEASURED."""
    t, cams, model = model_case(fmt)
    _, _, params, targets, _ = case(fmt)
    targets = [np.nan_to_num(x, nan=0.5) for x in targets]
    images, grad, _ = call(t, params, cams, targets, stop_thresh=0.0)
    img64, g64 = model.grad(params, np.stack(targets))
    d_img = np.abs(np.stack(images) - img64).max()
    g32 = grad.astype(np.float64) / FR.FIX
    rel = np.abs(g32 - g64).max() / np.abs(g64).max()
    print("%s: image max |delta| %.3g; gradient rel %.3g (measured %.3g), max |g64| %.3g" % (fmt, d_img, rel, GRAD_REL_MEASURED[fmt],
                                                                                             np.abs(g64).max()))
    assert d_img < 1e-3
    assert rel <= 2 * GRAD_REL_MEASURED[fmt]


def test_the_float64_model_agrees_with_central_differences(model_case):
    """Pure float64: 40 random parameters with a gradient, h = 1e-4.  The truncation term is h^2 / 6 |f'''|; with |f'''| <= 6 max |g|
    (a sigmoid's derivatives are below its first, a density's scale with the segment lengths < 1) the bound is h^2 max |g| =
    1e-8 max |g|; round-off, eps * loss / h ~ 1e-11, lies below it.  Measured: 1.7e-11 against max |g| = 0.036."""
    import torch
    t, cams, model = model_case("SH9")
    p0 = t.data.astype(np.float64)
    p0[..., :-1] *= 0.5
    p0[..., -1] *= 0.8
    targets = torch.sigmoid(torch.linspace(-2, 2, 3 * H * W * 3, dtype=torch.float64)).reshape(3, H, W, 3).numpy()
    _, g = model.grad(p0, targets)
    flat = g.reshape(-1)
    pick = np.random.default_rng(3).choice(np.flatnonzero(flat), 40, replace=False)
    h, worst = 1e-4, 0.0
    with torch.no_grad():
        for i in pick:
            vals = []
            for s in (1.0, -1.0):
                p = p0.reshape(-1).copy()
                p[i] += s * h
                vals.append(float(model.loss(model.values_of(p.reshape(p0.shape)), targets)))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - flat[i]))
    print("central differences: worst %.3g, max |g| %.3g" % (worst, np.abs(flat).max()))
    assert worst <= h * h * np.abs(flat).max()


# ------------------------------------------------------------------ 4. ten SGD steps
def perturbed(hf):
    hf.params[..., :-1] *= np.float32(0.5)
    hf.params[..., -1] *= np.float32(0.8)
    return hf


def ten_steps_host(t, cams, targets):
    """-> (the ten stats[0] words, the HostTreeFit after them)"""
    hf = perturbed(host_fit(t))
    words = []
    for _ in range(10):
        hf.accumulate(cams, targets)
        words.append(int(hf.stats[0]))
        assert hf.loss()[1] == 3 * W * H
        before, g = hf.params.copy(), hf.grad.copy()
        hf.step(LR10)
        assert np.array_equal(hf.params.view(np.uint32), FR.sgd_step(before, g, LR10).view(np.uint32)) and not hf.grad.any()
    return words, hf


def test_ten_sgd_steps_decrease_the_loss_strictly():
    t = make("SH9")
    cams = cams3()
    targets = host_fit(t).render(cams)
    words, hf = ten_steps_host(t, cams, targets)
    print([round(w / FR.FIX, 4) for w in words])
    assert all(b < a for a, b in zip(words, words[1:])), words
    assert words[-1] < 0.6 * words[0]
    half = hf.data_half()
    assert half.dtype == np.float16 and np.array_equal(half.view(np.uint16), hf.params.astype(np.float16).view(np.uint16))


def test_a_leaf_that_fails_either_density_test_never_moves():
    t = make("SH9")
    cams = cams3()
    sig = t.data[..., -1].astype(np.float32)
    leaves = np.argwhere((t.child == 0) & (sig > 1.0))
    rng = np.random.default_rng(2)
    pick = leaves[rng.choice(len(leaves), 400, replace=False)]
    a, b = tuple(pick[:200].T), tuple(pick[200:].T)
    data = t.data.copy()
    data[..., -1][a] = np.float16(0.005)  # the uploaded half fails; params keeps the large density
    t2 = synth.SynthTree(t.child, data, t.scale, t.offset, t.data_format, t.depth_limit, {})
    hf = host_fit(t2)
    hf.params[..., -1][a] = sig[a]
    hf.params[..., -1][b] = np.float32(0.005)  # params fails; the uploaded half is large
    hf.params[..., -1][tuple(pick[200:250].T)] = np.nan
    start = hf.params.copy()
    targets = [np.full((H, W, 3), 0.5, np.float32) for _ in cams]
    for _ in range(3):
        hf.accumulate(cams, targets)
        assert not hf.grad[a].any() and not hf.grad[b].any()
        hf.step(LR10)
    moved = (hf.params.view(np.uint32) != start.view(np.uint32)).any(-1)
    assert not moved[a].any() and not moved[b].any() and np.count_nonzero(moved) > 200  # (the other leaves the rays reach do move)
    # and it is stepped over: the images are those of a field without these leaves
    gone = t.data.copy()
    gone[..., -1][a] = 0
    gone[..., -1][b] = 0
    t3 = synth.SynthTree(t.child, gone, t.scale, t.offset, t.data_format, t.depth_limit, {})
    h2 = host_fit(t2)
    h2.params[...] = start
    assert same_images(h2.render(cams), host_fit(t3).render(cams))


# ------------------------------------------------------------------ 5. refusals
def _raw(t, cams, n, params, targets, grad, stats, images=None, child=None, opt=None, fmt=None, use_opt=True):
    child = t.child if child is None else child
    data = t.data.view(np.uint16)
    sc = (C.c_float * 3)(*[float(v) for v in t.scale])
    of = (C.c_float * 3)(*[float(v) for v in t.offset])
    co = (opt or R.RenderOptions()).to_c()
    arr = (CCamera * max(len(cams), 1))(*[c.to_c() for c in cams])
    ptrs = lambda xs: None if xs is None else (C.c_void_p * max(len(xs), 1))(*xs)  # noqa: E731
    return lib().rto_fit_grad_host(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), params, child.shape[0], child.shape[1],
                                   data.shape[-1], (fmt or t.data_format).encode(), sc, of, None, arr if cams else None, ptrs(targets),
                                   ptrs(images), n, C.byref(co) if use_opt else None, 0, grad, stats)


def test_refusal_texts():
    t = make("SH4")
    cam = rcam(9, 7, poses3()[0])
    params = t.data.astype(np.float32)
    grad = np.zeros(params.shape, np.int64)
    stats = np.zeros(2, np.int64)
    tg = np.zeros((7, 9, 3), np.float32)
    pp, gp, sp, tp = params.ctypes.data, grad.ctypes.data, stats.ctypes.data, tg.ctypes.data

    def refused(rc, code, text):
        msg = lib().rto_last_error().decode()
        assert rc == code and text in msg and msg.startswith("rto_fit_grad_host: "), (rc, msg)

    refused(_raw(t, [cam], 1, None, [tp], gp, sp), E_INVALID, "null params")
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp, use_opt=False), E_INVALID, "null options")
    refused(_raw(t, [cam], 1, pp + 2, [tp], gp, sp), E_INVALID, "params must be 4-byte aligned")
    refused(_raw(t, [cam], 1, pp, [tp], gp + 4, sp), E_INVALID, "grad must be 8-byte aligned")
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp + 4), E_INVALID, "stats must be 8-byte aligned")
    refused(_raw(t, [cam], 1, pp, None, gp, None), E_INVALID, "null targets with grad or stats set")
    refused(_raw(t, [cam], 1, pp, None, None, sp), E_INVALID, "null targets with grad or stats set")
    refused(_raw(t, [cam], -1, pp, [tp], gp, sp), E_INVALID, "n must be >= 0")
    refused(_raw(t, [], 1, pp, [tp], gp, sp), E_INVALID, "null cams with n > 0")
    refused(_raw(t, [cam, cam], 2, pp, [tp, None], gp, sp), E_INVALID, "camera 1: null target")
    refused(_raw(t, [cam, cam], 2, pp, [tp, tp + 2], gp, sp), E_INVALID, "camera 1: target must be 4-byte aligned")
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp, images=[tp + 1]), E_INVALID, "camera 0: image must be 4-byte aligned")
    refused(_raw(t, [cam, cam], 2, pp, [tp, pp + 64], gp, sp), E_INVALID, "camera 1: params overlaps the target")
    refused(_raw(t, [cam], 1, pp, [gp + 8 * (grad.size - 1)], gp, sp), E_INVALID, "camera 0: grad overlaps the target")
    bad = rcam(9, 7, poses3()[0])
    bad.fx = 0.0
    refused(_raw(t, [cam, bad], 2, pp, [tp, tp], gp, sp), E_INVALID, "camera 1: width, height (<= 1048560), fx or fy is out of range")
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp, opt=R.RenderOptions(rot_dirs=[0.0, 0.1, 0.0])), E_INVALID, "rot_dirs is not read")
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp, opt=R.RenderOptions(basis_minmax=[0, 3])), E_INVALID, "basis_minmax is not read")
    for fmt in ("SG4", "ASG4", "SH5", "SH9", "SH", "rgba"):
        refused(_raw(t, [cam], 1, pp, [tp], gp, sp, fmt=fmt), E_UNSUPPORTED, "the fit takes RGBA and SH trees of basis_dim 1, 4, 9, 16 or 25")
    child = t.child.copy()
    child[0, 0, 0, 0] = t.child.shape[0]
    refused(_raw(t, [cam], 1, pp, [tp], gp, sp, child=child), E_FORMAT, "the offset refers outside [1, %d)" % child.shape[0])
    assert not grad.any() and not stats.any(), "a refused call wrote"
    assert lib().rto_fit_sgd_step_host(None, gp, 4, 1.0) == E_INVALID and "null params or grad" in lib().rto_last_error().decode()
    assert lib().rto_fit_sgd_step_host(pp, gp, -1, 1.0) == E_INVALID and "count must be >= 0" in lib().rto_last_error().decode()
    # the Python wrappers' own checks
    with pytest.raises(R.RtoError):
        R.fit_grad_host(t.child, t.data, params.astype(np.float64), t.scale, t.offset, t.data_format, [cam], [tg])
    with pytest.raises(R.RtoError):
        R.fit_grad_host(t.child, t.data, params, t.scale, t.offset, t.data_format, [cam], [tg[:3]], grad=grad)
    with pytest.raises(R.RtoError):
        R.sgd_step_host(params, grad[:1], 1.0)
