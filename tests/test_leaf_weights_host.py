"""Per-leaf peak weights on the host (include/rto.h "leaf weights"; no GPU): the host twin against the numpy restatement word
for word and against the float64 model of the suite, its invariances, tree and option variants, refusals, kill_unseen, the
prune_octree tool with --backend cpu, and the rendering invariance of a weight-0 prune through the oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import leaf_weights_ref as LR
import orc
import rt_octree_amd as R
from helpers import FRAME_ANISO, assert_bits_equal, rcam, reframe, reframe_pose
from rt_octree_amd import prune_octree, synth
from rt_octree_amd._lib import CCamera, lib

E_INVALID, E_FORMAT = -1, -6
W47 = 47


def _ht(t, ndc=None):
    return orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)


def _host(t, cams, ndc=None, threads=0, out=None, **optkw):
    return R.leaf_weights_host(t.child, t.data, t.scale, t.offset, cams, R.RenderOptions(**optkw), ndc=ndc, threads=threads, out=out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def tree6():
    return synth.make_tree(6, 9, seed=7)


@pytest.fixture(scope="module")
def cams4():
    return [rcam(W47, W47, p) for p in synth.orbit_poses(4)]


@pytest.fixture(scope="module")
def host_default(tree6, cams4):
    w = _host(tree6, cams4)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------ 1. the numpy restatement, word for word
@pytest.mark.parametrize("stop_thresh", [1e-2, 0.0])
def test_host_twin_equals_the_numpy_restatement(tree6, cams4, host_default, stop_thresh):
    got = host_default if stop_thresh else _host(tree6, cams4, stop_thresh=0.0)
    want = LR.restate(_ht(tree6), cams4, stop_thresh=stop_thresh)
    assert got.shape == tree6.child.shape and got.dtype == np.float32
    assert_bits_equal(got, want, "host twin vs numpy restatement, stop_thresh %g" % stop_thresh)
    seen = int(np.count_nonzero(got > 0))
    print("stop_thresh %g: %d leaves seen" % (stop_thresh, seen))
    assert seen > 3000 and float(got.max()) <= 1.0 and float(got.min()) >= 0.0
    assert not (got[tree6.child != 0] != 0).any(), "an internal slot carries a weight"


def test_two_cameras_reach_the_leaves_the_design_note_counts(tree6, cams4):
    """two 47 x 47 cameras reach 3650 of the 13464 dense leaves of the depth-6 tree (stop_thresh 1e-2)"""
    w = _host(tree6, cams4[:2])
    dense = (tree6.child == 0) & (tree6.data[..., -1].astype(np.float32) > np.float32(1e-2))
    assert int(np.count_nonzero(dense)) == 13464 and int(np.count_nonzero(w > 0)) == 3650
    assert not (w[~dense] != 0).any()


# ------------------------------------------------------------------ 2. / 3. the float64 model (odd image sizes)
def test_host_twin_against_the_float64_model(tree6, cams4, host_default):
    """The image size is odd on purpose: at an even size column x = W / 2 of cameras 0 and 2 lies exactly in the tree's plane
    y = 0.5 (cameras 1 and 3: x = 0.5), a cell boundary, where the two precisions pick different neighbours.
    Bound: |delta| <= 1e-3 (six times the maximum measured with a numpy restatement of the definition, 1.7e-4), at most 0.1 % of
    the seen leaves outside it, and the same set of seen leaves."""
    fx = cams4[0].fx
    model = LR.model64(tree6, synth.orbit_poses(4), W47, W47, fx, fx, stop_thresh=1e-2)
    got = host_default.astype(np.float64)
    seen_h, seen_m = got > 0, model > 0
    delta = np.abs(got - model)
    over = int(np.count_nonzero(delta > 1e-3))
    print("seen: host %d, model %d, only one of them %d; max |delta| %.3g; over 1e-3: %d"
          % (seen_h.sum(), seen_m.sum(), np.count_nonzero(seen_h != seen_m), delta.max(), over))
    assert np.array_equal(seen_h, seen_m), "%d leaves are seen by only one statement" % np.count_nonzero(seen_h != seen_m)
    assert over <= 0.001 * np.count_nonzero(seen_h), over


# ------------------------------------------------------------------ 4. accumulation and invariance
def test_threads_splits_and_accumulation(tree6, cams4, host_default):
    assert np.array_equal(_bits(_host(tree6, cams4, threads=4)), _bits(host_default)), "threads = 4"
    assert np.array_equal(_bits(_host(tree6, cams4, threads=1)), _bits(host_default)), "threads = 1"
    part = _host(tree6, cams4[:1])
    first = part.copy()
    both = _host(tree6, cams4[1:], out=part)
    assert both is part and np.array_equal(_bits(both), _bits(host_default)), "cameras split over two calls"
    assert (both >= first).all() and (both > first).any()
    # into an array that is not zero: values only rise, and those already above stay
    base = np.full(tree6.child.shape, 0.25, np.float32)
    acc = _host(tree6, cams4, out=base.copy())
    assert np.array_equal(acc, np.maximum(base, host_default))
    # no camera: nothing changes
    assert np.array_equal(_host(tree6, [], out=base.copy()), base)


# ------------------------------------------------------------------ 5. tree and option variants against the restatement
@pytest.fixture(scope="module")
def tree5():
    return synth.make_tree(5, 9, seed=7)


def _variant(name, tree5):
    """-> (tree, cameras, ndc, option keywords)"""
    poses = synth.orbit_poses(4)
    if name == "ndc":
        pose = synth.look_at_c2w((0.1, 0.05, 0.3), target=(0, 0, -1), up=(0, 1, 0))
        return tree5, [rcam(33, 25, pose, fx=50.0)], (64.0, 48.0, 50.0), {}
    if name == "reframed":
        t = reframe(tree5, *FRAME_ANISO)
        return t, [rcam(33, 29, reframe_pose(p, tree5, t)) for p in poses[:2]], None, {}
    if name == "n4":
        from test_query import _n4_tree
        return _n4_tree(), [rcam(33, 33, p) for p in poses[:2]], None, {}
    if name == "bbox_crop":
        return tree5, [rcam(33, 31, p) for p in poses[:2]], None, {"render_bbox": [0.2, 0.1, 0.3, 0.8, 0.9, 0.7]}
    if name == "camera_inside":
        # tree-space (0.1, 0.1, 0.9): inside the box, in the empty corner above the scene (tmin = 0 for every ray)
        return tree5, [rcam(31, 33, synth.look_at_c2w((-1.2, -1.2, 1.2)))], None, {}
    if name == "step_size_0":
        return tree5, [rcam(33, 33, poses[1])], None, {"step_size": 0.0, "stop_thresh": 0.0}
    if name == "nan_inf_density":
        rng = np.random.default_rng(5)
        data = tree5.data.copy()
        sig = data[..., -1]
        leaves = np.argwhere((tree5.child == 0) & (sig.astype(np.float32) > 0))
        pick = leaves[rng.choice(len(leaves), 600, replace=False)]
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            p = pick[k * 200:(k + 1) * 200]
            sig[p[:, 0], p[:, 1], p[:, 2], p[:, 3]] = v
        t = synth.SynthTree(tree5.child, data, tree5.scale, tree5.offset, tree5.data_format, tree5.depth_limit, {})
        return t, [rcam(33, 33, p) for p in poses[:2]], None, {"stop_thresh": 0.0}
    raise KeyError(name)


@pytest.mark.parametrize("name", ["ndc", "reframed", "n4", "bbox_crop", "camera_inside", "step_size_0", "nan_inf_density"])
def test_variants_equal_the_numpy_restatement(name, tree5):
    t, cams, ndc, kw = _variant(name, tree5)
    got = _host(t, cams, ndc=ndc, **kw)  # (returns: every variant terminates)
    want = LR.restate(_ht(t, ndc), cams, ndc=ndc, **kw)
    assert_bits_equal(got, want, name)
    # (step_size = 0: a ray ends at the first cell face its step does not carry it across -- the point is that it ends)
    assert np.count_nonzero(got > 0) > (0 if name == "step_size_0" else 20), "the variant marches nothing"
    assert float(got.max()) <= 1.0 and float(got.min()) >= 0.0 and not np.isnan(got).any()


def test_a_non_finite_camera_marches_nothing(tree5):
    for i, v in ((9, np.nan), (10, np.inf), (0, np.nan), (4, -np.inf)):
        cam = rcam(17, 13, synth.orbit_poses(4)[0])
        flat = cam.transform.reshape(-1).copy()
        flat[i] = v
        cam.transform = flat.reshape(4, 3)
        got = _host(tree5, [cam])
        assert not got.any(), (i, v)
        assert_bits_equal(got, LR.restate(_ht(tree5), [cam]), "non-finite camera")


# ------------------------------------------------------------------ 6. refusals
def _raw_host(tree, cams, n, weights_ptr, child=None, opt=True):
    child = tree.child if child is None else child
    data = tree.data.view(np.uint16)
    sc = (C.c_float * 3)(*[float(v) for v in tree.scale])
    of = (C.c_float * 3)(*[float(v) for v in tree.offset])
    co = R.RenderOptions().to_c()
    arr = (CCamera * max(len(cams), 1))(*[c.to_c() for c in cams])
    return lib().rto_leaf_weights_host(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), child.shape[0], child.shape[1],
                                       data.shape[-1], sc, of, None, arr if cams else None, n, C.byref(co) if opt else None, 0, weights_ptr)


def test_refusal_texts(tree5):
    cam = rcam(9, 7, synth.orbit_poses(4)[0])
    w = np.zeros(tree5.child.shape, np.float32)
    wp = C.c_void_p(w.ctypes.data)

    def refused(rc, code, text):
        msg = lib().rto_last_error().decode()
        assert rc == code and text in msg and msg.startswith("rto_leaf_weights_host: "), (rc, msg)

    refused(_raw_host(tree5, [cam], -1, wp), E_INVALID, "n must be >= 0")
    refused(_raw_host(tree5, [], 1, wp), E_INVALID, "null cams with n > 0")
    refused(_raw_host(tree5, [cam], 1, None), E_INVALID, "null weights")
    refused(_raw_host(tree5, [cam], 1, C.c_void_p(w.ctypes.data + 2)), E_INVALID, "weights must be 4-byte aligned")
    refused(_raw_host(tree5, [cam], 1, wp, opt=False), E_INVALID, "null argument")
    for field, v in (("width", 0), ("height", 0), ("fx", 0.0), ("fy", float("nan")), ("fx", float("inf"))):
        bad = rcam(9, 7, synth.orbit_poses(4)[0])
        setattr(bad, field, v)
        refused(_raw_host(tree5, [cam, bad], 2, wp), E_INVALID, "camera 1: width, height (<= 1048560), fx or fy is out of range")
    child = tree5.child.copy()
    child[0, 0, 0, 0] = tree5.child.shape[0]  # refers to node `capacity`
    refused(_raw_host(tree5, [cam], 1, wp, child=child), E_FORMAT, "the offset refers outside [1, %d)" % child.shape[0])
    child = tree5.child.copy()
    root = child[0].reshape(-1)
    i = int(np.flatnonzero(root)[0])
    root[(i + 1) % 8] = root[i]  # two slots of the root refer to one node
    refused(_raw_host(tree5, [cam], 1, wp, child=child), E_FORMAT, "is reached twice")
    assert not w.any(), "a refused call wrote weights"
    # the Python wrappers' own checks
    with pytest.raises(R.RtoError):
        R.leaf_weights_host(tree5.child.astype(np.int64), tree5.data, tree5.scale, tree5.offset, [cam])
    with pytest.raises(R.RtoError):
        R.leaf_weights_host(tree5.child, tree5.data, tree5.scale, tree5.offset, [cam], out=np.zeros(3, np.float32))


# ------------------------------------------------------------------ 7. kill_unseen
def test_kill_unseen_on_hand_made_arrays():
    child = np.zeros((2, 2, 2, 2), np.int32)
    child[0, 0, 0, 0] = 1
    rng = np.random.default_rng(0)
    data = rng.normal(0, 1, (2, 2, 2, 2, 4)).astype(np.float16)
    data[..., -1] = np.abs(data[..., -1]) + np.float16(0.5)
    w = np.zeros((2, 2, 2, 2), np.float32)
    w[0, 0, 0, 1] = 0.5      # kept at any threshold <= 0.5
    w[0, 0, 1, 0] = 0.01     # exactly the threshold: kept (the test is <)
    w[0, 0, 1, 1] = 0.00999  # killed at 0.01, kept at 0
    w[1, 0, 0, 0] = 1e-30    # tiny but seen
    before = data.copy()
    out = R.kill_unseen(child, data, w, 0.01)
    assert np.array_equal(data.view(np.uint16), before.view(np.uint16)), "the input was written"
    assert out is not data and out.dtype == np.float16
    kept = np.zeros((2, 2, 2, 2), bool)
    kept[0, 0, 0, 0] = True  # internal slot: untouched whatever its weight
    kept[0, 0, 0, 1] = kept[0, 0, 1, 0] = True
    assert np.array_equal(out[..., :-1].view(np.uint16), before[..., :-1].view(np.uint16)), "coefficients changed"
    assert np.array_equal(out[..., -1].view(np.uint16)[kept], before[..., -1].view(np.uint16)[kept])
    assert (out[..., -1].view(np.uint16)[~kept] == 0).all()
    out0 = R.kill_unseen(child, data, w, 0.0)
    kept0 = kept.copy()
    kept0[0, 0, 1, 1] = kept0[1, 0, 0, 0] = True
    assert np.array_equal(out0[..., -1].view(np.uint16)[kept0], before[..., -1].view(np.uint16)[kept0])
    assert (out0[..., -1].view(np.uint16)[~kept0] == 0).all()
    with pytest.raises(R.RtoError):
        R.kill_unseen(child, data, w[:1], 0.01)
    with pytest.raises(R.RtoError):
        R.kill_unseen(child, data, w, float("nan"))


# ------------------------------------------------------------------ 8. the tool, --backend cpu
def _probe(path):
    buf = C.create_string_buffer(4096)
    assert lib().rto_tree_probe_npz(os.fsencode(str(path)), buf, 4096) == 0, lib().rto_last_error()
    return json.loads(buf.value.decode())


def test_pose_files_are_read_with_the_cli_conventions(tmp_path):
    poses = synth.orbit_poses(5)
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), poses)
    trans, w, h, fx, fy = prune_octree.load_poses("blender", js, 47, 45)
    assert (w, h) == (47, 45) and fx == fy == synth.blender_focal(47) and len(trans) == 5
    for t, p in zip(trans, poses):
        c = R.Camera(47, 45, fx, fy)
        c.set_c2w(p)
        assert np.array_equal(t.view(np.uint32), c.transform.view(np.uint32))
    pose_dir = synth.write_tt_dataset(str(tmp_path / "tt"), poses, fx=1160.0, fy=1170.0)
    trans, w, h, fx, fy = prune_octree.load_poses("tt", pose_dir)
    assert (w, h, fx, fy) == (1920, 1080, 1160.0, 1170.0) and len(trans) == 5
    for t, p in zip(trans, poses):  # (written with %.8f; the loader undoes the OpenCV flip)
        assert np.allclose(t, p[:3, :4].T, atol=2e-8 + 1e-7 * np.abs(p[:3, :4].T)), (t, p)
    assert prune_octree.scaled_size(1920, 1080, 1160.0, 1170.0, 0.025) == (48, 27, 29.0, 29.25)
    assert prune_octree.scaled_size(800, 800, 1111.0, 1111.0, 1.0) == (800, 800, 1111.0, 1111.0)
    with pytest.raises(ValueError, match="llff"):
        prune_octree.load_poses("llff", js)


def test_prune_octree_end_to_end_cpu(tmp_path, tree6, cams4, capsys):
    src = tree6.save_npz(str(tmp_path / "tree.npz"))
    poses = synth.orbit_poses(4)
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), poses)
    common = [src, "--poses", js, "-w", str(W47), "-h", str(W47), "--backend", "cpu"]
    wnpy = str(tmp_path / "w.npy")
    assert prune_octree.main(common + ["--out_dir", str(tmp_path / "pruned"), "--save_weights", wnpy]) == 0
    text = capsys.readouterr().out
    assert "Poses 4, 47 x 47" in text and "Nodes %d -> " % tree6.capacity in text and "seen 5956" in text and "Size" in text
    # the saved weights are the twin's; the output is what kill_unseen + simplify_tree(kill_thresh = 0) give
    w = np.load(wnpy)
    assert np.array_equal(_bits(w), _bits(_host(tree6, cams4)))
    out = tmp_path / "pruned" / "tree.npz"
    info = _probe(out)
    assert info["capacity"] < tree6.capacity and info["N"] == 2 and info["data_dim"] == 28 and info["data_format"] == "SH9"
    c_want, d_want, _, st = R.simplify_tree(tree6.child, R.kill_unseen(tree6.child, tree6.data, w, 0.01), 0.0, backend="cpu")
    with np.load(out) as z:
        assert np.array_equal(z["child"], c_want) and np.array_equal(z["data"].view(np.uint16), d_want.view(np.uint16))
        assert np.array_equal(z["invradius3"], tree6.scale) and np.array_equal(z["offset"], tree6.offset) and str(z["data_format"]) == "SH9"
    print("pruned: %d -> %d nodes" % (tree6.capacity, info["capacity"]))
    # a second run without --overwrite skips; with it the same bytes come back
    before = out.read_bytes()
    assert prune_octree.main(common + ["--out_dir", str(tmp_path / "pruned")]) == 0
    assert " > skip" in capsys.readouterr().out and out.read_bytes() == before
    assert prune_octree.main(common + ["--out_dir", str(tmp_path / "pruned"), "--overwrite"]) == 0
    assert " > skip" not in capsys.readouterr().out
    with np.load(out) as z:
        assert np.array_equal(z["child"], c_want) and np.array_equal(z["data"].view(np.uint16), d_want.view(np.uint16))
    # --no_merge keeps child and changes only density halves
    assert prune_octree.main(common + ["--out_dir", str(tmp_path / "nomerge"), "--no_merge", "--max_imgs", "2"]) == 0
    assert "Poses 2" in capsys.readouterr().out
    with np.load(tmp_path / "nomerge" / "tree.npz") as z:
        assert np.array_equal(z["child"], tree6.child)
        d = z["data"]
    assert np.array_equal(d[..., :-1].view(np.uint16), tree6.data[..., :-1].view(np.uint16))
    w2 = _host(tree6, cams4[:2])
    assert np.array_equal(d.view(np.uint16), R.kill_unseen(tree6.child, tree6.data, w2, 0.01).view(np.uint16))
    assert np.count_nonzero(d[..., -1] != tree6.data[..., -1]) > 5000


def test_prune_octree_tt_poses_refusals_and_stale_keys(tmp_path, tree5, capsys):
    src = str(tmp_path / "tree.npz")
    np.savez(src, data_dim=np.int64(28), data_format=np.array("SH9"), invradius3=tree5.scale, offset=tree5.offset, child=tree5.child,
             data=tree5.data, n_internal=np.int64(7), parent_depth=np.zeros((tree5.capacity, 2), np.int32), my_key=np.arange(3))
    poses = synth.orbit_poses(3)
    pose_dir = synth.write_tt_dataset(str(tmp_path / "tt"), poses)
    args = [src, "--poses", pose_dir, "--dataset", "tt", "--scale", "0.025", "--backend", "cpu", "--weight_thresh", "0"]
    assert prune_octree.main(args + ["--out_dir", str(tmp_path / "out")]) == 0
    assert "Poses 3, 48 x 27, fx 29 fy 29" in capsys.readouterr().out
    with np.load(tmp_path / "out" / "tree.npz") as z:
        assert "n_internal" not in z.files and "parent_depth" not in z.files and np.array_equal(z["my_key"], np.arange(3))
        assert z["child"].shape[0] < tree5.capacity
        trans, w, h, fx, fy = prune_octree.load_poses("tt", pose_dir)
        cams = prune_octree.make_cameras(trans, *prune_octree.scaled_size(w, h, fx, fy, 0.025))
        wts = _host(tree5, cams)
        c_want, d_want, _, _ = R.simplify_tree(tree5.child, R.kill_unseen(tree5.child, tree5.data, wts, 0.0), 0.0, backend="cpu")
        assert np.array_equal(z["child"], c_want) and np.array_equal(z["data"].view(np.uint16), d_want.view(np.uint16))
    # refusals: LLFF, a quantised file, a weight threshold that is no number
    js = synth.write_transforms_json(str(tmp_path / "t.json"), poses)
    assert prune_octree.main([src, "--poses", js, "--dataset", "llff", "--backend", "cpu", "--out_dir", str(tmp_path / "x")]) == 2
    assert "llff" in capsys.readouterr().err
    q = str(tmp_path / "quant.npz")
    tree5.save_quant_npz(q, n_retain=1)
    assert prune_octree.main([q, "--poses", js, "-w", "9", "-h", "9", "--backend", "cpu", "--out_dir", str(tmp_path / "x")]) == 2
    assert "quantised" in capsys.readouterr().err and not (tmp_path / "x" / "quant.npz").exists()
    assert prune_octree.main([src, "--poses", js, "--weight_thresh", "nan", "--backend", "cpu", "--out_dir", str(tmp_path / "x")]) == 2


# ------------------------------------------------------------------ 9. rendering invariance through the oracle
def test_a_weight_0_prune_renders_the_same_bits(tree6, cams4):
    """weight_thresh = 0, stop_thresh = 0, no merge: the leaves no ray of the two cameras reaches with any weight are emptied, and
    the oracle renders the same aux words from the same two cameras at SPP 1, 6 and 32.  (A merged tree is not bit-identical:
    coarser empty leaves change the step sequence.)"""
    cams = cams4[:2]
    w = _host(tree6, cams, stop_thresh=0.0)
    pruned = R.kill_unseen(tree6.child, tree6.data, w, 0.0)
    killed = np.count_nonzero(pruned[..., -1].view(np.uint16) != tree6.data[..., -1].view(np.uint16))
    assert killed > 500, killed
    ht_a = _ht(tree6)
    ht_b = orc.HostTree(tree6.child, pruned, tree6.scale, tree6.offset, tree6.data_format)
    differ = words = 0
    for spp in (1, 6, 32):
        for k, cam in enumerate(cams):
            ocam = orc.camera(cam.width, cam.height, cam.fx, cam.fy, cam.transform.reshape(-1))
            opt = orc.default_options(spp=spp)
            a, _, _ = orc.render_frame(ht_a, ocam, opt, orc.rng(frame=k), want_stats=False)
            b, _, _ = orc.render_frame(ht_b, ocam, opt, orc.rng(frame=k), want_stats=False)
            differ += int(np.count_nonzero(_bits(a) != _bits(b)))
            words += a.size
    print("%d of %d aux words differ (%d leaves emptied)" % (differ, words, killed))
    assert words == 106032 and differ == 0
