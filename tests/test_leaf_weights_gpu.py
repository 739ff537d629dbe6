"""Per-leaf peak weights on the device (rto_tree_leaf_weights, csrc/leaf_weight_kernels.hip): the kernel's words equal the host
twin's -- which tests/test_leaf_weights_host.py pins to the numpy restatement and the float64 model -- over every walk (two-level
image, one-level image, child[]), every storage form, chunked and mixed-size camera lists; a weight-0 prune renders the same
bits through the HIP renderer; a call between two renders disturbs neither; the tool's two backends write the same bytes."""
import os

import numpy as np
import pytest

import rt_octree_amd as R
from helpers import FRAME_ANISO, rcam, reframe, reframe_pose
from rt_octree_amd import prune_octree, synth

pytestmark = pytest.mark.gpu
W47 = 47


def _upload(tree, **kw):
    return R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra, **kw)


def _host(t, cams, ndc=None, data=None, **optkw):
    return R.leaf_weights_host(t.child, t.data if data is None else data, t.scale, t.offset, cams, R.RenderOptions(**optkw), ndc=ndc,
                               threads=8)


def _cams3(W=W47, H=W47):
    return [rcam(W, H, p) for p in synth.orbit_poses(4)[:3]]


def _same(dev, host, what, floor=20):
    import torch
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.float32 and tuple(dev.shape) == host.shape
    got = dev.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got.reshape(-1) != host.view(np.uint32).reshape(-1))
    assert bad.size == 0, "%s: %d of %d words differ; first at slot %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], dev.cpu().numpy().reshape(-1)[bad[0]], host.reshape(-1)[bad[0]])
    assert np.count_nonzero(host) > floor, what + ": nothing was marched"


def _check(dt, tree, cams, what, ndc=None, data=None, floor=20, **optkw):
    dev = R.leaf_weights(dt, cams, R.RenderOptions(**optkw))
    _same(dev, _host(tree, cams, ndc=ndc, data=data, **optkw), what, floor)
    return dev


@pytest.fixture(scope="module")
def tree5():
    return synth.make_tree(5, 9, seed=7)


def test_depth_6_default_upload_splits_chunks_mixed_sizes_and_no_camera():
    import torch
    tree = synth.make_tree(6, 9, seed=7)
    dt = _upload(tree)
    assert dt.wide_nodes > 0
    bytes_before = dt.device_bytes
    cams = _cams3()
    whole = _check(dt, tree, cams, "depth 6, two-level image")
    _check(dt, tree, cams, "stop_thresh 0", stop_thresh=0.0)
    dt._refresh()
    assert dt.device_bytes == bytes_before, "the call brought child[] / data[] back"
    # a split of one call into two, accumulating
    part = R.leaf_weights(dt, cams[:1])
    both = R.leaf_weights(dt, cams[1:], out=part)
    assert both is part and torch.equal(both.view(torch.int32), whole.view(torch.int32))
    # n = 0 launches nothing and leaves `out` alone
    keep = whole.clone()
    assert R.leaf_weights(dt, [], out=whole) is whole and torch.equal(whole.view(torch.int32), keep.view(torch.int32))
    assert not R.leaf_weights(dt, []).any()
    # 33 cameras of 17 x 13 in one call: one more than a launch takes, partial tiles
    poses = synth.orbit_poses(33)
    c33 = [rcam(17, 13, p) for p in poses]
    _check(dt, tree, c33, "33 cameras")
    # mixed sizes in one call (runs of one size become launches)
    mixed = [rcam(17, 13, poses[0]), rcam(17, 13, poses[5]), rcam(31, 9, poses[9]), rcam(17, 13, poses[13]), rcam(16, 16, poses[20])]
    _check(dt, tree, mixed, "mixed sizes")
    # the wrapper's own checks and the entry's refusals
    with pytest.raises(R.RtoError):
        R.leaf_weights(dt, cams, out=torch.zeros(3, device="cuda"))
    with pytest.raises(R.RtoError):
        R.leaf_weights(dt, cams, out=torch.zeros(tuple(whole.shape)))  # host memory
    bad = rcam(9, 9, poses[0])
    bad.fx = 0.0
    with pytest.raises(R.RtoError) as e:
        R.leaf_weights(dt, [cams[0], bad], out=whole)
    assert e.value.code == -1 and "camera 1" in e.value.msg and torch.equal(whole.view(torch.int32), keep.view(torch.int32))


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


@pytest.mark.parametrize("name", ["keep_reference", "compact_records", "shuffled", "reframed", "n4", "rgba"])
def test_storage_forms_and_tree_shapes(name, tree5):
    from helpers import rgba_tree
    from test_query import _n4_tree
    cams = _cams3()
    if name == "keep_reference":
        tree, kw = tree5, {"keep_reference": True}
    elif name == "compact_records":
        tree, kw = tree5, {"compact_records": True}
    elif name == "shuffled":  # weights are numbered like the arrays the tree was uploaded from
        tree, kw = synth.shuffle_nodes(tree5, seed=3), {}
    elif name == "reframed":
        tree, kw = reframe(tree5, *FRAME_ANISO), {}
        cams = [rcam(W47, W47, reframe_pose(p, tree5, tree)) for p in synth.orbit_poses(4)[:3]]
    elif name == "n4":  # no traversal image: child[] with the float descent
        tree, kw = _n4_tree(), {}
    else:
        tree, kw = rgba_tree(tree5), {}
    _check(_upload(tree, **kw), tree, cams, name)


def test_quantised_direct_file(tmp_path, tree5):
    path = str(tmp_path / "quant.npz")
    decoded = tree5.save_quant_npz(path, n_retain=1)
    dt = R.N3Tree(path, quant_direct=True)
    _check(dt, tree5, _cams3(), "quantised-direct", data=decoded)


def test_ndc_crop_and_a_camera_inside_the_box(tree5):
    dt = _upload(tree5)
    _check(dt, tree5, _cams3(), "render_bbox crop", render_bbox=[0.2, 0.1, 0.3, 0.8, 0.9, 0.7])
    inside = [rcam(W47, W47, synth.look_at_c2w((-1.2, -1.2, 1.2))), rcam(W47, W47, synth.look_at_c2w((1.2, -1.2, 1.3)))]
    _check(dt, tree5, inside + _cams3()[:1], "camera inside the box")
    # (step_size 0: a ray ends at the first cell face its step does not carry it across; few leaves, the same on both sides)
    _check(dt, tree5, _cams3(), "step_size 0", floor=0, step_size=0.0, stop_thresh=0.0)
    ndc = (64.0, 48.0, 50.0)
    dt.set_ndc(*ndc)
    poses = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2), (0.0, -0.1, 0.4))]
    _check(dt, tree5, [rcam(W47, 35, p, fx=50.0) for p in poses], "NDC", ndc=ndc)


# ------------------------------------------------------------------ rendering invariance through the HIP renderer
def _aux(dt, cam, spp, kernel, frame):
    ctx = R.RenderContext(cam.width, cam.height)
    ctx.rng_seed()
    for _ in range(frame):
        ctx.rng_advance()
    ctx.set_kernel(kernel)
    R.launch_renderer(dt, cam, R.RenderOptions(spp=spp, denoise=False), ctx)
    return ctx.download_aux()


def test_a_weight_0_prune_renders_the_same_bits_on_the_device():
    tree = synth.make_tree(6, 9, seed=7)
    cams = _cams3()[:2]
    dt = _upload(tree)
    w = R.leaf_weights(dt, cams, R.RenderOptions(stop_thresh=0.0)).cpu().numpy()
    pruned = R.kill_unseen(tree.child, tree.data, w, 0.0)
    assert np.count_nonzero(pruned[..., -1].view(np.uint16) != tree.data[..., -1].view(np.uint16)) > 500
    dp = R.N3Tree.from_arrays(tree.child, pruned, tree.scale, tree.offset, tree.data_format)
    for spp in (1, 6, 32):
        for kernel in (R.KERNEL_AUTO, R.KERNEL_GENERIC, R.KERNEL_FAST):
            for k, cam in enumerate(cams):
                a, b = _aux(dt, cam, spp, kernel, k), _aux(dp, cam, spp, kernel, k)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (spp, kernel, k)
        frames = []
        for t in (dt, dp):
            bctx = R.RenderContext(W47, W47, frames=2)
            R.launch_renderer_batch(t, cams, R.RenderOptions(spp=spp, denoise=False), bctx, rng_jumps=[3, 1])
            got = []
            for f in range(2):
                bctx.select_frame(f)
                got.append(bctx.download_aux().view(np.uint32))
            frames.append(got)
        assert all(np.array_equal(a, b) for a, b in zip(*frames)), ("batch", spp)


def test_a_call_between_two_renders_changes_neither_the_frames_nor_the_rng(tree5):
    dt = _upload(tree5)
    cam = _cams3()[1]
    opt = R.RenderOptions(spp=6, denoise=False)

    def two_frames(between):
        ctx = R.RenderContext(cam.width, cam.height)
        ctx.rng_seed()
        R.launch_renderer(dt, cam, opt, ctx)
        a = ctx.download_aux()
        if between:
            R.leaf_weights(dt, _cams3())
        ctx.rng_advance()
        R.launch_renderer(dt, cam, opt, ctx)
        return a, ctx.download_aux(), ctx.rng_get()

    a0, b0, r0 = two_frames(False)
    a1, b1, r1 = two_frames(True)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))
    assert tuple(r0) == tuple(r1)
    assert not np.array_equal(a0.view(np.uint32), b0.view(np.uint32))


def test_prune_octree_backends_write_the_same_bytes(tmp_path):
    tree = synth.make_tree(6, 9, seed=7)
    src = tree.save_npz(str(tmp_path / "tree.npz"))
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), synth.orbit_poses(4))
    common = [src, "--poses", js, "-w", str(W47), "-h", str(W47)]
    for merge in ([], ["--no_merge"]):
        tag = "nomerge" if merge else "merge"
        outs = {}
        for backend in ("hip", "cpu"):
            d = tmp_path / (backend + "_" + tag)
            wn = str(tmp_path / ("w_%s_%s.npy" % (backend, tag)))
            assert prune_octree.main(common + merge + ["--backend", backend, "--out_dir", str(d), "--save_weights", wn]) == 0
            outs[backend] = ((d / "tree.npz").read_bytes(), open(wn, "rb").read())
        assert outs["hip"][1] == outs["cpu"][1], "weights differ (%s)" % tag
        assert outs["hip"][0] == outs["cpu"][0], "pruned files differ (%s)" % tag
    with np.load(tmp_path / "hip_merge" / "tree.npz") as z:
        assert z["child"].shape[0] < tree.capacity
