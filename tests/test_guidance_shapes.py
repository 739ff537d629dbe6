"""The fused GuidanceNet for every trained shape (rto_guidance_net_create_layers, guidance_general.inc): 8 -> c1 [-> c1] ->
2 * levels with c1 in 1..64, levels in 1..6, two or three layers.  Layout (bit-exact on data that is exact in fp16 / fp32),
rounding points (against the float64 emulation, with torch's own fp16 run of the same net as the yardstick), input modes,
tile skipping and rto_denoise, the reference shape through the new entry, the refusals of the packed / sparse routes, the CLI."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rt_octree_amd as R
from rt_octree_amd import _lib, synth, volrend

torch = pytest.importorskip("torch")
from rt_octree_amd import denoiser  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "rt-octree_amd", "bin", "volrend_headless")
E_INVALID, E_UNSUPPORTED = -1, -3

SHAPES = [(8, 6, 2), (16, 3, 2), (64, 1, 2), (32, 4, 3), (64, 6, 3), (20, 2, 3), (8, 5, 3)]  # (c1, levels, layers)
_ids = ["c%d_l%d_n%d" % s for s in SHAPES]


# ---------------------------------------------------------------- not gpu

def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rto.h")).read()
    L = C.CDLL(R.LIB_PATH)
    for name in ("rto_guidance_net_create_layers", "rto_guidance_net_get_info"):
        assert "int %s(" % name in hdr
        assert name in _lib.SYMBOLS
        getattr(L, name)
    assert "typedef struct rto_guidance_layer" in hdr and "typedef struct rto_guidance_net_info" in hdr


def _layer_structs(specs):
    """specs: [(cin, cout)] -> (ctypes array of rto_guidance_layer, the numpy arrays that back it)"""
    keep, arr = [], (_lib.CGuidanceLayer * len(specs))()
    for l, (cin, cout) in zip(arr, specs):
        w = np.full((max(cout, 1), max(cin, 1), 3, 3), 0.125, np.float32)
        b = np.zeros(max(cout, 1), np.float32)
        keep += [w, b]
        l.weight, l.bias, l.cin, l.cout = w.ctypes.data, b.ctypes.data, cin, cout
    return arr, keep


def test_invalid_stacks_are_refused_without_a_device():
    """every RTO_E_INVALID case of rto_guidance_net_create_layers is decided on the host, before any device is touched"""
    lib = R.lib()
    h = C.c_void_p(0)

    def create(arr, n, levels, out=True):
        return lib.rto_guidance_net_create_layers(arr, n, levels, 0, C.byref(h) if out else None)

    ok, keep = _layer_structs([(8, 16), (16, 6)])
    assert create(None, 2, 3) == E_INVALID
    assert create(ok, 2, 3, out=False) == E_INVALID
    for field in ("weight", "bias"):
        arr, keep2 = _layer_structs([(8, 16), (16, 6)])
        setattr(arr[1], field, None)
        assert create(arr, 2, 3) == E_INVALID, field
    arr, k1 = _layer_structs([(7, 16), (16, 6)])  # the first layer does not read the 8 aux channels
    assert create(arr, 2, 3) == E_INVALID and b"8 aux channels" in lib.rto_last_error()
    arr, k2 = _layer_structs([(8, 16), (12, 6)])  # broken chain
    assert create(arr, 2, 3) == E_INVALID
    arr, k3 = _layer_structs([(8, 16), (16, 16), (12, 6)])
    assert create(arr, 3, 3) == E_INVALID
    arr, k4 = _layer_structs([(8, 16), (16, 6)])  # last cout != 2 * levels
    assert create(arr, 2, 4) == E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        arr, k5 = _layer_structs([(8, 16), (16, 16), (16, 6)])
        k5[2][3, 2, 1, 1] = bad
        assert create(arr, 3, 3) == E_INVALID and b"non-finite" in lib.rto_last_error()
    # (RTO_E_UNSUPPORTED is decided on the host as well)
    arr, k6 = _layer_structs([(8, 16), (16, 16), (16, 16), (16, 6)])
    assert create(arr, 4, 3) == E_UNSUPPORTED
    arr, k7 = _layer_structs([(8, 65), (65, 6)])
    assert create(arr, 2, 3) == E_UNSUPPORTED
    arr, k8 = _layer_structs([(8, 16), (16, 24), (24, 6)])
    assert create(arr, 3, 3) == E_UNSUPPORTED
    arr, k9 = _layer_structs([(8, 16), (16, 14)])
    assert create(arr, 2, 7) == E_UNSUPPORTED
    arr, k10 = _layer_structs([(8, 6)])
    assert create(arr, 1, 3) == E_UNSUPPORTED
    assert not h.value


# ---------------------------------------------------------------- gpu

gpu = pytest.mark.gpu


def _integer_net(c1, levels, layers, seed):
    """weights and biases that keep every product, sum and activation exact in fp16 / fp32 and the activations off the
    clamps: first and last layer randint(-2, 3) / 8, biases randint(-4, 5) / 8, middle layer in {-1, 0, 1} kept with
    probability 6 / (9 cin), a last layer with cin > 8 thinned to about 24 taps per output"""
    g = torch.Generator().manual_seed(seed)
    net = denoiser.GuidanceNetCompact(8, c1, layers, levels).eval()
    with torch.no_grad():
        for i, layer in enumerate(net.layers):
            w = layer.conv.weight
            cin = w.shape[1]
            if 0 < i < layers - 1:
                v = torch.randint(-1, 2, w.shape, generator=g).float()
                v = v * (torch.rand(w.shape, generator=g) < 6.0 / (9 * cin)).float()
            else:
                v = torch.randint(-2, 3, w.shape, generator=g).float() / 8
                if i == layers - 1 and cin > 8:
                    v = v * (torch.rand(w.shape, generator=g) < 24.0 / (9 * cin)).float()
            w.copy_(v)
            layer.conv.bias.copy_(torch.randint(-4, 5, layer.conv.bias.shape, generator=g).float() / 8)
    return net


def _exactness(net, aux):
    """float64 evaluation: (every activation is an fp16 value, smallest share of a layer's values strictly inside (0, 6))"""
    import torch.nn.functional as F
    x = aux.double()
    exact, inside = True, 1.0
    for layer in net.layers:
        x = F.conv2d(x, layer.conv.weight.double(), layer.conv.bias.double(), padding=1).clamp(0.0, 6.0)
        exact = exact and bool(torch.equal(x.half().double(), x))
        inside = min(inside, float(((x > 0) & (x < 6)).double().mean()))
    return exact, inside


_INT_IMAGES = [(1, 24, 40), (2, 5, 7), (1, 9, 161)]


@pytest.fixture(scope="module")
def integer_cases():
    """per shape: the integer net, and per image its input and fp32 reference maps -- computed once"""
    out = {}
    for si, (c1, levels, layers) in enumerate(SHAPES):
        # (seeds chosen on the CPU so that at least 30 % of every layer's float64 values lie strictly inside (0, 6))
        net = _integer_net(c1, levels, layers, 203 if (c1, levels, layers) == (20, 2, 3) else 201)
        g = torch.Generator().manual_seed(7 + si)
        imgs = []
        for shape in _INT_IMAGES:
            aux = torch.randint(0, 3, (shape[0], 8) + shape[1:], generator=g).float() / 4
            with torch.no_grad():
                w_ref, g_ref = net(aux)
            imgs.append((aux, w_ref, g_ref))
        out[(c1, levels, layers)] = (net, imgs)
    return out


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_layout_is_bit_exact_on_integer_data(integer_cases, shape):
    """MFMA fragment maps, k-step packing (tap pairs for 16 channels, two k-steps per tap for 64), channel padding, halo and
    border of every layer, the softmax across lane groups: on data whose every product and sum is exact the kernel equals the
    fp32 network exactly"""
    net, imgs = integer_cases[shape]
    fused = denoiser.FusedGuidanceNet(net)
    assert (fused.c1, fused.levels, fused.num_layers) == shape
    assert fused.packed_route is False
    for aux, w_ref, g_ref in imgs:
        exact, inside = _exactness(net, aux)
        assert exact, "the recipe left an activation that is not an fp16 value"
        assert inside >= 0.25, "saturated data: only %.2f of a layer's values inside (0, 6)" % inside
        w, gm = fused(aux.cuda().contiguous())
        torch.cuda.synchronize()
        assert torch.equal(gm.cpu(), g_ref), tuple(aux.shape)
        assert float((w.cpu() - w_ref).abs().max()) < 2e-6, tuple(aux.shape)  # softmax: fast exp vs torch exp


def _default_net(c1, levels, layers, seed):
    torch.manual_seed(seed)
    return denoiser.GuidanceNetCompact.from_full(denoiser.GuidanceNet(8, c1, 5, layers, levels)).eval()


@gpu
@pytest.mark.parametrize("image", [(1, 48, 64), (2, 33, 47)])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rounding_points_against_the_half_pipeline(shape, image):
    """against the float64 emulation of the reference's fp16 rounding points.  Yardstick: the same net as the reference runs it,
    compact.half() under torch on the GPU -- both differ from the emulation only by the fp32 accumulation order, so the fused
    kernel may be off by at most twice torch's own distance (and never less than the 4e-3 the two-layer test allows)."""
    from test_guidance_fused import _emulate_fp16_network
    c1, levels, layers = shape
    n, H, W = image
    compact = _default_net(c1, levels, layers, 7)
    fused = denoiser.FusedGuidanceNet(compact)
    torch.manual_seed(8)
    aux = torch.rand(n, 8, H, W)
    aux[:, 4:] = aux[:, :4] ** 2
    w_ref, g_ref = _emulate_fp16_network(compact, aux)
    with torch.no_grad():
        w_t, g_t = copy.deepcopy(compact).half().cuda()(aux.cuda())
    w, g = fused(aux.cuda().contiguous())
    torch.cuda.synchronize()
    w, g, w_t, g_t = w.cpu(), g.cpu(), w_t.float().cpu(), g_t.float().cpu()
    dg_t, dw_t = float((g_t - g_ref).abs().max()), float((w_t - w_ref).abs().max())
    dg, dw = float((g - g_ref).abs().max()), float((w - w_ref).abs().max())
    print("shape %s image %s: guidance fused %.3e torch %.3e | weights fused %.3e torch %.3e" % (shape, image, dg, dg_t, dw, dw_t))
    assert dg <= max(2 * dg_t, 4e-3)
    assert dw <= max(2 * dw_t, 4e-3)
    assert np.allclose(w.sum(1).numpy(), 1.0, atol=1e-5)


@gpu
@pytest.mark.parametrize("image", [(2, 37, 53), (1, 17, 350)])
@pytest.mark.parametrize("shape", [(16, 3, 2), (32, 4, 3)], ids=["c16_l3_n2", "c32_l4_n3"])
def test_input_modes_give_the_same_bytes(shape, image):
    n, H, W = image
    fused = denoiser.FusedGuidanceNet(_default_net(*shape, seed=3))
    torch.manual_seed(4)
    aux = torch.rand(n, 8, H, W)
    aux[:, 4:] = aux[:, :4] * aux[:, :4]
    dev_aux = aux.cuda().contiguous()
    w0, g0 = (t.clone() for t in fused(dev_aux))
    poisoned = dev_aux.clone()
    poisoned[:, 4:] = 123.0  # must not be read in the implied mode
    w1, g1 = (t.clone() for t in fused(poisoned, squares_implied=True))
    rgba = dev_aux[:, :4].permute(0, 2, 3, 1).contiguous()  # [n][H][W][4] = planes 0..3 interleaved
    w2, g2 = fused(rgba, rgba=True)
    torch.cuda.synchronize()
    assert torch.equal(w0, w1) and torch.equal(g0, g1)
    assert torch.equal(w0, w2) and torch.equal(g0, g2)


@pytest.fixture(scope="module")
def cull_scene():
    t = synth.make_tree(depth_limit=7, basis_dim=9, shell=2.5)
    dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
    yield dt
    dt.free()


def _net_tiles_skipped_and_computed(marks, n, H, W, halo):
    """from the tile marks: (network tiles 32 x 8 whose input region lies inside the image and in unmarked render tiles, others)"""
    from denoise_synth import net_tiles_skipped_and_computed  # (the predicate lives with the other restated skip decisions)
    ptr, words, _s0, _frames, _bg = marks
    m = torch.as_tensor(volrend._DevArray(ptr, (n, words), None), device="cuda:0").view(torch.int32).cpu().numpy().view(np.uint32)
    return net_tiles_skipped_and_computed(m, H, W, halo)


@gpu
@pytest.mark.parametrize("shape", [(16, 3, 2), (32, 4, 3)], ids=["c16_l3_n2", "c32_l4_n3"])
def test_culling_and_one_call_denoise_are_bit_identical(cull_scene, shape):
    from helpers import assert_bits_equal
    from test_filter_cull import cams_for, images
    dt = cull_scene
    net = denoiser.FusedGuidanceNet(_default_net(*shape, seed=3))
    W, H, n = 200, 152, 3
    cams = cams_for(W, H, n)
    opt = R.RenderOptions(spp=4, denoise=True, background_brightness=0.75)
    ctx = R.RenderContext(W, H, frames=n)
    ctx.rng_seed()
    R.launch_renderer_batch(dt, cams, opt, ctx)
    marks = ctx.tile_marks()
    assert marks is not None and marks[3] == n
    skipped, computed = _net_tiles_skipped_and_computed(marks, n, H, W, net.num_layers)
    assert skipped > 0 and computed > 0, (skipped, computed)
    aux = torch.as_tensor(ctx.batch_views()[0], device="cuda:0")[:n]
    ctx.select_frame(0)
    wm, gm = (t.clone() for t in net(aux, squares_implied=True))
    wm_c, gm_c = (t.clone() for t in net(aux, squares_implied=True, cull=marks))
    torch.cuda.synchronize()
    assert_bits_equal(wm_c.cpu().numpy(), wm.cpu().numpy(), "weight planes, culled network")
    assert_bits_equal(gm_c.cpu().numpy(), gm.cpu().numpy(), "guidance planes, culled network")
    want = {}
    for mode in (R.FILTER_EXACT, R.FILTER_FAST):
        R.filtering(None, wm, gm, ctx.noisy_ptr, ctx.image_ptr, mode=mode)
        torch.cuda.synchronize()
        want[mode] = images(ctx, n)
        torch.as_tensor(ctx.batch_views()[2], device="cuda:0").fill_(-7.0)
        net.filter_planes(wm_c, gm_c, ctx.noisy_ptr, ctx.image_ptr, mode=mode, cull=marks)
        torch.cuda.synchronize()
        assert_bits_equal(images(ctx, n).cpu().numpy(), want[mode].cpu().numpy(), "culled filter, mode %d" % mode)
        torch.as_tensor(ctx.batch_views()[2], device="cuda:0").fill_(-7.0)
        net.denoise(ctx, n, mode)
        torch.cuda.synchronize()
        assert_bits_equal(images(ctx, n).cpu().numpy(), want[mode].cpu().numpy(), "rto_denoise on full outputs, mode %d" % mode)
    # a lean level-1 batch: the network reads the interleaved image
    lean = R.RenderContext(W, H, frames=n)
    lean.set_lean_outputs(1)
    lean.rng_seed()
    R.launch_renderer_batch(dt, cams, opt, lean)
    assert lean.frames_are_lean(0, n)
    for mode in (R.FILTER_EXACT, R.FILTER_FAST):
        torch.as_tensor(lean.batch_views()[2], device="cuda:0").fill_(-7.0)
        lean.select_frame(0)
        net.denoise(lean, n, mode)
        torch.cuda.synchronize()
        assert_bits_equal(images(lean, n).cpu().numpy(), want[mode].cpu().numpy(), "rto_denoise on lean frames, mode %d" % mode)
    # sparse lean frames have no route for a general net
    sparse = R.RenderContext(W, H, frames=n)
    sparse.set_lean_outputs(2)
    sparse.rng_seed()
    R.launch_renderer_batch(dt, cams, opt, sparse)
    sparse.select_frame(0)
    with pytest.raises(R.RtoError) as e:
        net.denoise(sparse, n, R.FILTER_FAST)
    assert e.value.code == E_UNSUPPORTED
    net.denoise(ctx, n, R.FILTER_FAST)  # the handle stays usable
    torch.cuda.synchronize()
    assert_bits_equal(images(ctx, n).cpu().numpy(), want[R.FILTER_FAST].cpu().numpy(), "rto_denoise after the refusal")
    for c in (ctx, lean, sparse):
        c.free()


@gpu
def test_reference_shape_through_the_new_entry():
    """create_layers with 8 -> 32 -> 8 is rto_guidance_net_create's handle: same planes, same packed route"""
    compact = _default_net(32, 4, 2, seed=5)
    new = denoiser.FusedGuidanceNet(compact)  # (through rto_guidance_net_create_layers)
    assert new.packed_route is True and (new.c1, new.levels, new.num_layers) == (32, 4, 2)
    sd = {k: v.detach().float().cpu().contiguous() for k, v in compact.state_dict().items()}
    h = C.c_void_p(0)
    _lib.check(R.lib().rto_guidance_net_create(sd["layers.0.conv.weight"].data_ptr(), sd["layers.0.conv.bias"].data_ptr(),
                                               sd["layers.1.conv.weight"].data_ptr(), sd["layers.1.conv.bias"].data_ptr(), 32, 4, 0, C.byref(h)))
    old = denoiser.FusedGuidanceNet.__new__(denoiser.FusedGuidanceNet)
    old._h, old._out, old.levels, old.device = h, {}, 4, torch.device("cuda", 0)
    info = _lib.CGuidanceNetInfo()
    _lib.check(R.lib().rto_guidance_net_get_info(h, C.byref(info)))
    assert (info.c1, info.levels, info.num_layers, info.halo, info.packed_route) == (32, 4, 2, 2, 1)
    torch.manual_seed(6)
    n, H, W = 2, 37, 53
    aux = torch.rand(n, 8, H, W)
    aux[:, 4:] = aux[:, :4] * aux[:, :4]
    aux = aux.cuda().contiguous()
    noisy = torch.rand(n, H, W, 4, device="cuda:0")
    outs = []
    for net in (old, new):
        w, g = (t.clone() for t in net(aux))
        out = torch.full_like(noisy, -3.0)
        net.forward_packed(aux, squares_implied=True)
        net.filter_packed(noisy, out)
        torch.cuda.synchronize()
        outs.append((w, g, out))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@gpu
def test_packed_and_sparse_routes_are_refused_for_a_general_net():
    compact = _default_net(16, 3, 2, seed=9)
    net = denoiser.FusedGuidanceNet(compact)
    n, H, W = 1, 24, 40
    torch.manual_seed(10)
    aux = torch.rand(n, 8, H, W).cuda().contiguous()
    noisy = torch.rand(n, H, W, 4, device="cuda:0")
    out = torch.empty_like(noisy)
    w0, g0 = (t.clone() for t in net(aux))
    lib, h = R.lib(), net._h
    marks = torch.full(((5 * 3 + 31) // 32 + 1,), -1, dtype=torch.int32, device="cuda:0")
    calls = {
        "forward_packed": lambda: net.forward_packed(aux),
        "filter_packed": lambda: net.filter_packed(noisy, out, shape=(n, H, W)),
        "reserve": lambda: net.reserve(n, H, W),
        "forward_packed_culled": lambda: _lib.check(lib.rto_guidance_net_forward_packed_culled(h, None, aux.data_ptr(), n, H, W, 0, marks.data_ptr(), marks.numel(), 1.0)),
        "filtering_packed_culled": lambda: _lib.check(lib.rto_filtering_packed_culled(h, None, noisy.data_ptr(), out.data_ptr(), n, H, W, marks.data_ptr(), marks.numel(), 1.0)),
        "forward_ex sparse": lambda: _lib.check(lib.rto_guidance_net_forward_ex(h, None, noisy.data_ptr(), n, H, W, w0.data_ptr(), g0.data_ptr(), 2 | 4)),
        "forward_culled sparse": lambda: _lib.check(lib.rto_guidance_net_forward_culled(h, None, noisy.data_ptr(), n, H, W, w0.data_ptr(), g0.data_ptr(), 2 | 4,
                                                                                        marks.data_ptr(), marks.numel(), 1.0)),
    }
    for name, call in calls.items():
        with pytest.raises(R.RtoError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED, name
        assert "16" in e.value.msg and "3" in e.value.msg, (name, e.value.msg)  # the message names the shape
        w1, g1 = net(aux)  # the handle stays usable
        torch.cuda.synchronize()
        assert torch.equal(w1, w0) and torch.equal(g1, g0), name


@gpu
def test_cli_runs_a_three_layer_module_fused(tmp_path):
    from PIL import Image
    tree = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    tp = tree.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(2)
    pp = synth.write_transforms_json(str(tmp_path / "transforms_test.json"), poses)
    torch.manual_seed(0)
    ts = denoiser.compact_and_compile(denoiser.GuidanceNet(8, 16, 3, 3, 3), device="cuda:0", example_hw=(64, 80))
    tsp = str(tmp_path / "ts_latest.ts")
    ts.save(tsp)
    op = synth.write_opt_json(str(tmp_path / "opt.json"))
    base = [BIN, tp, pp, "--options", op, "--ts_module", tsp, "-w", "80", "-h", "64", "--warmup", "1"]
    out_f, out_t = str(tmp_path / "fused"), str(tmp_path / "torch")
    rf = subprocess.run(base + ["-o", out_f], capture_output=True, text=True, timeout=600)
    assert rf.returncode == 0, rf.stderr
    assert "GuidanceNet runs as the fused HIP kernel" in rf.stdout
    rt = subprocess.run(base + ["-o", out_t, "--torch_net"], capture_output=True, text=True, timeout=600)
    assert rt.returncode == 0, rt.stderr
    assert "GuidanceNet runs through libtorch" in rt.stdout
    dt = R.N3Tree(tp)
    ctx = R.RenderContext(80, 64)
    fx = synth.blender_focal(80)
    cam = R.Camera(80, 64, fx, fx)
    opt = R.RenderOptions.from_json(op)
    fused = denoiser.FusedGuidanceNet(torch.jit.load(tsp, map_location="cuda:0"))
    assert (fused.c1, fused.levels, fused.num_layers, fused.packed_route) == (16, 3, 3, False)
    for i in range(2):
        cam.set_c2w(poses[i])
        ctx.rng_seed()
        ctx.rng_advance((1 + i) << 32)
        R.launch_renderer(dt, cam, opt, ctx)
        wm, gm = fused(torch.as_tensor(ctx.aux_view(), device="cuda:0"), squares_implied=True)
        R.filtering(None, wm[0].contiguous(), gm[0].contiguous(), ctx.noisy_ptr, ctx.image_ptr)
        want = ctx.download_rgba8()
        got = np.array(Image.open(os.path.join(out_f, "r_%d.png" % i)))
        assert np.array_equal(got, want), i
        ref = np.array(Image.open(os.path.join(out_t, "r_%d.png" % i)))
        mse = np.mean((got[..., :3].astype(np.float64) / 255 - ref[..., :3].astype(np.float64) / 255) ** 2)
        assert mse == 0 or -10 * np.log10(mse) > 50.0, i
    ctx.free()
    dt.free()
