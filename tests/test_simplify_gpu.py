"""The HIP tree simplifier (rto_tree_simplify, csrc/simplify_kernels.hip) against the numpy model of tests/simplify_ref.py and
the host twin, child / data / node_map / stats bit for bit (the definition leaves no freedom: no tolerance), and what the
simplified tree does downstream on the device: point queries, the batched render against the CPU oracle on that same tree, the
4096-spp mean against the float64 model, and the simplify_octree command on the device against itself on the host.

Shapes: the host tests' list -- D = 4, 5, 13, 28 (a record aligned to 8, 2, 2 and 8 bytes), N = 2 and 4, negative offsets,
garbage nodes, 1 .. 32 levels, 18885 nodes (19 tiles of the scan), 300001 nodes (293 tiles: the scan of the tile counts takes two
chunks of 256), and buffers that are not aligned to 16 bytes (the half-by-half scatter)."""
import ctypes as C

import numpy as np
import pytest

import expected_render as E
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import simplify, simplify_octree, synth
from rt_octree_amd._lib import CSimplifyStats

from helpers import assert_bits_equal, make_pair, oracle_whole_frame, rcam
from test_simplify_host import _write_tree, renumbering_inputs

pytestmark = pytest.mark.gpu

RTO_E_INVALID, RTO_E_FORMAT = -1, -6


@pytest.fixture(scope="module")
def simplifier():
    s = R.Simplifier(0)
    yield s
    s.free()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to("cuda:0")


def _run(s, child, data, kill, stream=None):
    c, d, m, st = s.simplify(_dev(child), _dev(data), kill, stream)
    return c.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy(), st


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_kernels_equal_model_and_host_twin(simplifier, name):
    child, data, kill, want = SR.case(name)
    got = _run(simplifier, child, data, kill)
    SR.assert_same(got, want, name + " vs model")
    SR.assert_same(got, simplify.simplify_tree(child, data, kill, backend="cpu"), name + " vs host twin")


@pytest.mark.parametrize("name", ["sh4_depth6_kill50", "sh9_depth4_kill50", "n4_kill"])
def test_buffers_not_aligned_to_16_bytes(simplifier, name):
    """data and data_out 2 bytes off a 16-byte boundary: the half-by-half scatter"""
    import torch
    child, data, kill, want = SR.case(name)
    cap, N, D = child.shape[0], child.shape[1], data.shape[-1]
    halves = data.size
    src = torch.zeros(halves + 8, dtype=torch.float16, device="cuda:0")
    dst = torch.zeros(halves + 8, dtype=torch.float16, device="cuda:0")
    src[1:1 + halves] = _dev(data).reshape(-1)
    dc, child_out = _dev(child), torch.zeros(child.size, dtype=torch.int32, device="cuda:0")
    node_map = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    out_cap, st = C.c_int64(0), CSimplifyStats()
    thresh = float("nan") if kill is None else kill
    R._lib.check(R.lib().rto_tree_simplify(simplifier._h, None, C.c_void_p(dc.data_ptr()), C.c_void_p(src.data_ptr() + 2), cap, N, D, thresh,
                                           C.c_void_p(child_out.data_ptr()), C.c_void_p(dst.data_ptr() + 2), C.byref(out_cap),
                                           C.c_void_p(node_map.data_ptr()), C.byref(st)))
    k = out_cap.value
    assert k == want[0].shape[0] and st.merged == want[3]["merged"]
    assert np.array_equal(child_out.cpu().numpy()[:k * N ** 3], want[0].reshape(-1))
    assert np.array_equal(dst.cpu().numpy()[1:1 + k * N ** 3 * D].view(np.uint16), want[1].reshape(-1).view(np.uint16))
    assert float(dst[0]) == 0.0 and np.array_equal(node_map.cpu().numpy()[:k], want[2])


def test_two_runs_are_bit_identical_and_streams_agree(simplifier):
    import torch
    child, data, kill, want = SR.case("rgba_depth7_kill50")
    a = _run(simplifier, child, data, kill)
    b = _run(simplifier, child, data, kill)
    SR.assert_same(b, a, "second run")
    s = torch.cuda.Stream()
    dc, dd = _dev(child), _dev(data)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c, d, m, st = simplifier.simplify(dc, dd, kill, s)
    s.synchronize()
    SR.assert_same((c.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy(), st), want, "non-default stream")


def wide_tree():
    """300001 nodes, D = 1: a full octree of seven levels (299593 nodes) with 408 more nodes below its last level -- 293 tiles
    of the scan, so the scan of the tile counts runs in two chunks.  Three leaves in four are empty: a tenth of the leaf nodes
    is uniform"""
    counts = [1, 8, 64, 512, 4096, 32768, 262144, 408]
    cap = sum(counts)
    child = np.zeros((cap, 8), np.int32)
    first = np.cumsum([0] + counts)
    for l in range(len(counts) - 1):
        slots = np.arange(counts[l + 1])
        parent = first[l] + slots // 8
        child[parent, slots % 8] = (first[l + 1] + slots) - parent
    data = (np.random.default_rng(21).random((cap, 8, 1)) < 0.25).astype(np.float16)
    return child.reshape(cap, 2, 2, 2), data.reshape(cap, 2, 2, 2, 1)


def test_one_handle_reuses_its_scratch():
    s = R.Simplifier(0)
    try:
        child, data = wide_tree()
        assert child.shape[0] == 300001
        want = simplify.simplify_tree(child, data, 0.0, backend="cpu")  # (the host tests hold the twin to the model)
        assert want[3]["merged"] > 1000 and want[3]["levels"] == 8
        first = _run(s, child, data, 0.0)
        SR.assert_same(first, want, "300001 nodes")
        small = SR.case("sh4_depth3_kill50")
        SR.assert_same(_run(s, small[0], small[1], small[2]), small[3], "67 nodes after 300001")
        SR.assert_same(_run(s, child, data, 0.0), first, "third call")
    finally:
        s.free()


@pytest.mark.parametrize("kind", SR.MALFORMED + ("too_deep",))
def test_malformed_links_are_refused(simplifier, kind):
    child, data = SR.too_deep() if kind == "too_deep" else SR.malformed(kind)
    with pytest.raises(R.RtoError) as e:
        _run(simplifier, child, data, None)
    assert e.value.code == RTO_E_FORMAT and e.value.msg
    ok = SR.case("sh4_depth3_lossless")  # the handle is fine afterwards
    SR.assert_same(_run(simplifier, ok[0], ok[1], ok[2]), ok[3], "after the refusal")


def test_argument_refusals(simplifier):
    import torch
    child, data, _, want = SR.case("sh4_depth3_lossless")
    cap, D = child.shape[0], data.shape[-1]
    dc, dd = _dev(child), _dev(data)
    co = torch.full((cap * 8,), 7, dtype=torch.int32, device="cuda:0")
    do = torch.zeros(cap * 8 * D, dtype=torch.float16, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    oc = C.c_int64(0)

    def refused(*args):
        rc = R.lib().rto_tree_simplify(*args)
        msg = R.lib().rto_last_error().decode()
        assert rc == RTO_E_INVALID and msg, (rc, msg)
        return msg

    h, nan = simplifier._h, float("nan")
    assert "child is not memory" in refused(h, None, C.c_void_p(child.ctypes.data), P(dd), cap, 2, D, nan, P(co), P(do), C.byref(oc), None, None)
    host_out = np.zeros(cap * 8 * D, np.float16)
    assert "data_out is not memory" in refused(h, None, P(dc), P(dd), cap, 2, D, nan, P(co), C.c_void_p(host_out.ctypes.data), C.byref(oc), None, None)
    host_map = np.zeros(cap, np.int64)
    assert "node_map is not memory" in refused(h, None, P(dc), P(dd), cap, 2, D, nan, P(co), P(do), C.byref(oc), C.c_void_p(host_map.ctypes.data), None)
    assert "null" in refused(None, None, P(dc), P(dd), cap, 2, D, nan, P(co), P(do), C.byref(oc), None, None)
    assert "null" in refused(h, None, P(dc), None, cap, 2, D, nan, P(co), P(do), C.byref(oc), None, None)
    assert "null" in refused(h, None, P(dc), P(dd), cap, 2, D, nan, P(co), P(do), None, None, None)
    assert "cap" in refused(h, None, P(dc), P(dd), 0, 2, D, nan, P(co), P(do), C.byref(oc), None, None)
    assert "2^31" in refused(h, None, P(dc), P(dd), 1 << 28, 2, D, nan, P(co), P(do), C.byref(oc), None, None)
    assert "N must" in refused(h, None, P(dc), P(dd), cap, 1, D, nan, P(co), P(do), C.byref(oc), None, None)
    assert "D must" in refused(h, None, P(dc), P(dd), cap, 2, 0, nan, P(co), P(do), C.byref(oc), None, None)
    assert "overlap" in refused(h, None, P(dc), P(dd), cap, 2, D, nan, P(dc), P(do), C.byref(oc), None, None)
    assert "overlap" in refused(h, None, P(dc), P(dd), cap, 2, D, nan, P(co), C.c_void_p(dd.data_ptr() + 64), C.byref(oc), None, None)
    torch.cuda.synchronize()
    assert (co == 7).all()  # nothing was enqueued
    SR.assert_same(_run(simplifier, child, data, None), want, "after the refusals")


def _unit_tree(child, data, fmt="SH4"):
    """in a world that IS tree space: points with exact binary coordinates stay exactly on cell faces"""
    return R.N3Tree.from_arrays(child, data, np.ones(3, np.float32), np.zeros(3, np.float32), fmt)


@pytest.mark.parametrize("name", ["sh4_depth6_lossless", "sh4_depth6_kill50", "sh4_depth5_shuffled_garbage_kill50"])
def test_queries_return_the_original_bits(simplifier, name):
    child, data, kill, _ = SR.case(name)
    got = _run(simplifier, child, data, kill)
    pts = SR.probe_points(got[3]["levels"] + 3).astype(np.float32)
    a, b = _unit_tree(child, data), _unit_tree(got[0], got[1])
    qa, qb = a.query(pts, values=True, sigma=True, level=True), b.query(pts, values=True, sigma=True, level=True)
    va, vb = qa["values"].cpu().numpy(), qb["values"].cpu().numpy()
    sa, sb = qa["sigma"].cpu().numpy(), qb["sigma"].cpu().numpy()
    live = np.ones(len(pts), bool)
    if kill is not None:
        live = sa.astype(np.float16) > np.float16(kill)  # (sigma is a widened half: the cast back is exact)
    assert live.sum() > 100 and (kill is None or (~live).sum() > 100)
    assert_bits_equal(vb[live], va[live], "values")
    assert_bits_equal(sb[live], sa[live], "sigma")
    assert not vb[~live].view(np.uint32).any() and not sb[~live].view(np.uint32).any()
    la, lb = qa["level"].cpu().numpy(), qb["level"].cpu().numpy()
    assert (lb <= la).all() and (lb < la).any()
    a.free()
    b.free()


@pytest.fixture(scope="module")
def depth6(simplifier):
    """the depth-6 SH9 tree of smoke() and its simplified twins: lossless, and killed at 50"""
    t = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    out = {"tree": t}
    for key, kill in (("lossless", None), ("kill50", 50.0)):
        c, d, _, st = _run(simplifier, t.child, t.data, kill)
        assert st["merged"] > 1000
        out[key] = synth.SynthTree(c, d, t.scale, t.offset, t.data_format, t.depth_limit, {})
    return out


@pytest.mark.parametrize("key", ["lossless", "kill50"])
def test_simplified_tree_renders_like_the_oracle_renders_it(depth6, key):
    t = depth6[key]
    ht, dt = make_pair(t)
    W, H, spp = 96, 64, 4
    cams = [rcam(W, H, synth.orbit_poses(8)[i]) for i in (1, 5)]
    jumps = [3, 11]
    ctx = R.RenderContext(W, H, frames=2)
    R.launch_renderer_batch(dt, cams, R.RenderOptions(spp=spp, denoise=False), ctx, rng_jumps=jumps)
    for f in range(2):
        aux_o, _ = oracle_whole_frame(ht, cams[f], cams[f].fx, spp, jumps[f])
        ctx.select_frame(f)
        aux = ctx.download_aux()
        assert (aux[3] > 0).mean() > 0.05
        assert_bits_equal(aux, aux_o, "%s tree, frame %d" % (key, f))
    dt.free()


def test_the_mean_of_4096_spp_on_the_simplified_tree_matches_the_float64_model(simplifier):
    """the check and the sample count of test_expectation_gpu.test_hip_mean_matches_rendering_equation (batched kernel), with the
    simplified tree on the device and the ORIGINAL tree in the model"""
    from test_expectation import _check_against_model, _thin
    t = _thin(synth.make_tree(depth_limit=6, basis_dim=9, seed=3, shell=1.5), 0.08)
    c, d, _, st = _run(simplifier, t.child, t.data, None)
    assert st["merged"] > 1000
    dt = R.N3Tree.from_arrays(c, d, t.scale, t.offset, t.data_format)
    W = H = 64
    fx = 0.9 * synth.blender_focal(W)
    pose = synth.orbit_poses(7)[3]
    cam = rcam(W, H, pose, fx)
    rot = [0.1, 0.3, -0.2]
    opt = R.RenderOptions(spp=32, denoise=False, background_brightness=0.5, rot_dirs=rot)
    ctx = R.RenderContext(W, H, frames=2)
    acc = np.zeros((4, H, W))
    n_frames = 0
    for launch in range(64):
        ctx.rng_seed(977 + 7919 * launch)
        R.launch_renderer_batch(dt, [cam] * 2, opt, ctx, rng_jumps=[0, 1 + launch])
        for k in range(2):
            ctx.select_frame(k)
            acc += ctx.download_aux()[:4]
            n_frames += 1
    mean, var = E.expected_frame(E.Scene.of(t), pose, W, H, fx, fx, bg=0.5, rot_dirs=rot)
    _check_against_model(acc / n_frames, mean, var, n_frames * 32, "hip batched, simplified tree")
    dt.free()


def test_a_renumbered_tree_renders_the_same_frames(simplifier):
    """T1 shuffled and padded with garbage, simplified without a kill, is T1 shuffled -- and renders T1's frames bit for bit"""
    (sc, sd), (gc, gd) = renumbering_inputs()
    got = _run(simplifier, gc, gd, None)
    assert np.array_equal(got[0], sc) and np.array_equal(got[1].view(np.uint16), sd.view(np.uint16))
    t1 = SR.case("sh4_depth6_kill50")[3]
    ref = SR.synth_tree(6, 4)
    W, H = 96, 64
    cam = rcam(W, H, synth.orbit_poses(8)[2])
    frames = []
    for c, d in ((t1[0], t1[1]), (got[0], got[1])):
        dt = R.N3Tree.from_arrays(c, d, ref.scale, ref.offset, ref.data_format)
        ctx = R.RenderContext(W, H)
        R.launch_renderer_batch(dt, [cam], R.RenderOptions(spp=4, denoise=False), ctx, rng_jumps=[5])
        frames.append((ctx.download_aux(), ctx.download_image()))
        dt.free()
    assert (frames[0][0][3] > 0).mean() > 0.05
    assert_bits_equal(frames[1][0], frames[0][0], "aux")
    assert_bits_equal(frames[1][1], frames[0][1], "image")


def test_simplify_octree_on_the_device_writes_the_host_file_and_renders(tmp_path, capsys):
    src = str(tmp_path / "tree.npz")
    _write_tree(src, depth_limit=6, basis_dim=9)
    common = [src, "--sigma_thresh", "20.004"]
    assert simplify_octree.main(common + ["--backend", "cpu", "--out_dir", str(tmp_path / "cpu")]) == 0
    assert simplify_octree.main(common + ["--backend", "hip", "--out_dir", str(tmp_path / "hip")]) == 0
    capsys.readouterr()
    with open(str(tmp_path / "cpu" / "tree.npz"), "rb") as a, open(str(tmp_path / "hip" / "tree.npz"), "rb") as b:
        assert a.read() == b.read()
    with np.load(src) as f:
        cap_before = f["child"].shape[0]
    path = str(tmp_path / "hip" / "tree.npz")
    tree = R.N3Tree(path)
    with np.load(path) as f:
        assert f["child"].shape[0] < cap_before
        ht, dt = make_pair(synth.SynthTree(f["child"], f["data"], f["invradius3"], f["offset"], str(f["data_format"]), 6, {}))
    W = H = 64
    cam = rcam(W, H, synth.orbit_poses(8)[1])
    frames = []
    for t in (tree, dt):
        ctx = R.RenderContext(W, H)
        R.launch_renderer_batch(t, [cam], R.RenderOptions(spp=4, denoise=False), ctx, rng_jumps=[3])
        frames.append(ctx.download_aux())
    assert_bits_equal(frames[0], frames[1], "file vs arrays")
    aux_o, _ = oracle_whole_frame(ht, cam, cam.fx, 4, 3)
    assert_bits_equal(frames[0], aux_o, "file vs oracle")
    assert frames[0][3].std() > 0.01  # something was drawn
    tree.free()
    dt.free()
