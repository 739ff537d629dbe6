"""The host twin of the tree simplifier (rto_tree_simplify_host, csrc/host/tree_simplify.cpp) against the numpy model of
tests/simplify_ref.py, bit for bit (include/rto.h "simplifier" leaves nothing to an implementation: there is no tolerance), the
properties the operation promises (idempotence, pure renumbering, the field at every point, the float64 rendering model), every
refusal, and the simplify_octree command on the host.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import expected_render as E
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import simplify, simplify_octree, synth
from rt_octree_amd._lib import CSimplifyStats

RTO_E_INVALID, RTO_E_FORMAT = -1, -6


def _host(child, data, kill):
    return simplify.simplify_tree(child, data, kill, backend="cpu")


def test_the_model_reproduces_the_node_counts_of_the_table():
    for depth, (nodes, lossless, kill50, kill1e4) in SR.TABLE.items():
        child, data = SR._arrays(SR.synth_tree(depth, 4))
        got = (child.shape[0],) + tuple(SR.simplify(child, data, k)[3]["capacity"] for k in (None, 50.0, 1e4))
        assert got == (nodes, lossless, kill50, kill1e4), depth


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_host_twin_equals_the_model(name):
    child, data, kill, want = SR.case(name)
    SR.assert_same(_host(child, data, kill), want, name)


def test_what_the_cases_cover():
    assert SR.case("sh4_depth6_kill1e4")[3][3]["capacity"] == 1 and SR.case("sh9_depth4_kill_beyond_fp16")[3][3]["capacity"] == 1
    assert SR.case("chain_of_five")[3][3]["merged"] == 5 and SR.case("chain_of_31")[3][3]["merged"] == 31
    assert SR.case("uniform_root")[3][3]["capacity"] == 1 and SR.case("root_made_uniform")[3][3]["capacity"] == 1
    assert (SR.case("sh4_depth5_shuffled_lossless")[0] < 0).any()  # negative offsets
    assert SR.case("sh4_depth4_garbage")[3][3]["unreachable"] == 8
    assert SR.case("rgba_depth7_kill50")[0].shape[0] > 2 * 1024  # the scan's tile is 1024 nodes
    rounded, exact = SR.case("sh4_depth5_kill_rounded")[3], SR.case("sh4_depth5_shuffled_kill50")[3]
    assert rounded[3]["killed"] == exact[3]["killed"]  # 50.004 kills what 50.0 kills
    # the chain's record arrives in the root's slot
    child, data, _, want = SR.case("chain_of_five")
    assert np.array_equal(want[1].reshape(8, -1)[1].view(np.uint16), data.reshape(-1, 8, data.shape[-1])[5, 0].view(np.uint16))


@pytest.mark.parametrize("name", ["sh4_depth6_kill50", "sh4_depth5_shuffled_garbage_kill50", "n4", "special_densities_kill0",
                                  "root_made_uniform"])
def test_simplifying_an_output_changes_nothing(name):
    _, _, kill, want = SR.case(name)
    again = _host(want[0], want[1], kill)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1].view(np.uint16), want[1].view(np.uint16))
    assert again[3]["merged"] == 0 and again[3]["unreachable"] == 0
    assert np.array_equal(again[2], np.arange(want[0].shape[0]))


def renumbering_inputs(name="sh4_depth6_kill50"):
    """-> (T1 shuffled, T1 shuffled with garbage appended): T1 = the model's output of the case"""
    t1 = SR.case(name)[3]
    sc, sd = SR.shuffled(t1[0], t1[1], seed=11)
    gc, gd = SR.with_garbage(sc, sd, seed=13)
    return (sc, sd), (gc, gd)


def test_a_simplified_tree_is_only_renumbered():
    (sc, sd), (gc, gd) = renumbering_inputs()
    got = _host(gc, gd, None)
    assert np.array_equal(got[0], sc) and np.array_equal(got[1].view(np.uint16), sd.view(np.uint16))
    assert got[3]["merged"] == 0 and got[3]["unreachable"] == 8 and np.array_equal(got[2], np.arange(sc.shape[0]))


@pytest.mark.parametrize("name", ["sh4_depth6_lossless", "sh4_depth6_kill50", "sh4_depth5_shuffled_garbage_kill50", "n4_kill",
                                  "special_densities_kill0", "special_densities_kill_minus1", "chain_of_five"])
def test_the_field_is_unchanged_at_every_point(name):
    child, data, kill, _ = SR.case(name)
    got = _host(child, data, kill)
    pts = SR.probe_points(got[3]["levels"] + 3)
    before, lvl_before = SR.descend(child, data, pts)
    after, lvl_after = SR.descend(got[0], got[1], pts)
    live = np.ones(len(pts), bool)
    if kill is not None:
        with np.errstate(over="ignore"):
            live = before[:, -1].view(np.float16) > np.float32(kill).astype(np.float16)
    assert np.array_equal(after[live], before[live])
    assert not after[~live].any()
    assert (lvl_after <= lvl_before).all()
    if got[3]["merged"]:
        assert (lvl_after < lvl_before).any()


@pytest.mark.parametrize("thresh", [50.0, 2.0])
def test_float64_model_renders_the_simplified_tree_like_the_original(thresh):
    """expected_frame (float64) of the original and of the simplified tree, both at sigma_thresh = the kill threshold: mean and
    variance within 1e-9 absolute.  The bound is derived, not measured: the quantities are O(1), the arithmetic is float64 and
    the merged segments change a few hundred roundings at most."""
    t = synth.make_tree(depth_limit=5, basis_dim=4, seed=3, shell=1.5)
    child, data, _, st = _host(t.child, t.data, thresh)
    assert st["merged"] > 100
    W, H = 24, 20
    fx = 0.9 * synth.blender_focal(W)
    pose = synth.orbit_poses(7)[3]
    mean0, var0 = E.expected_frame(E.Scene.of(t), pose, W, H, fx, fx, bg=0.5, sigma_thresh=thresh)
    mean1, var1 = E.expected_frame(E.Scene(child, data, t.scale, t.offset, t.data_format), pose, W, H, fx, fx, bg=0.5, sigma_thresh=thresh)
    print("max |mean difference| %.3e, max |variance difference| %.3e" % (np.abs(mean1 - mean0).max(), np.abs(var1 - var0).max()))
    assert (mean0[3] > 0.05).sum() > 50
    assert np.abs(mean1 - mean0).max() <= 1e-9 and np.abs(var1 - var0).max() <= 1e-9


# ---------------------------------------------------------------- refusals
def _call(child, data, cap, N, D, kill=float("nan"), child_out=0, data_out=0, out_cap=0, node_map=None, stats=None):
    """the raw entry; 0 for an output = a fresh buffer (of the size a sane cap asks for: a refused call writes nothing)"""
    keep = []

    def ptr(a):
        if a is None:
            return None
        if isinstance(a, int):
            return C.c_void_p(a)
        keep.append(a)
        return C.c_void_p(a.ctypes.data)
    if isinstance(child_out, int) and child_out == 0:
        child_out = np.zeros(max(min(cap, 1 << 16), 1) * min(N, 4) ** 3, np.int32)
    if isinstance(data_out, int) and data_out == 0:
        data_out = np.zeros(max(min(cap, 1 << 16), 1) * min(N, 4) ** 3 * max(D, 1), np.uint16)
    oc = C.c_int64(-7) if out_cap == 0 else out_cap
    rc = R.lib().rto_tree_simplify_host(ptr(child), ptr(data), cap, N, D, kill, ptr(child_out), ptr(data_out),
                                        C.byref(oc) if oc is not None else None, ptr(node_map), stats)
    return rc, R.lib().rto_last_error().decode()


@pytest.mark.parametrize("kind", SR.MALFORMED)
def test_refuses_malformed_links(kind):
    child, data = SR.malformed(kind)
    rc, msg = _call(child, data, child.shape[0], 2, data.shape[-1])
    assert rc == RTO_E_FORMAT and msg, (rc, msg)
    with pytest.raises(SR.FormatError):
        SR.simplify(child, data)
    with pytest.raises(R.RtoError) as e:
        _host(child, data, None)
    assert e.value.code == RTO_E_FORMAT


def test_refuses_a_walk_of_more_than_32_levels():
    child, data = SR.too_deep()
    rc, msg = _call(child, data, child.shape[0], 2, 4)
    assert rc == RTO_E_FORMAT and "32 levels" in msg
    with pytest.raises(SR.FormatError):
        SR.simplify(child, data)


def test_refuses_arguments():
    child, data = SR._arrays(SR.synth_tree(3, 1))
    cap = child.shape[0]
    ok = lambda **kw: _call(child, data, cap, 2, 4, **kw)  # noqa: E731
    assert ok()[0] == 0
    for kw in (dict(child_out=None), dict(data_out=None), dict(out_cap=None)):
        rc, msg = ok(**kw)
        assert rc == RTO_E_INVALID and "null" in msg, kw
    for args in ((None, data), (child, None)):
        rc, msg = _call(args[0], args[1], cap, 2, 4)
        assert rc == RTO_E_INVALID and "null" in msg
    for c, n, d, word in ((0, 2, 4, "cap"), (-5, 2, 4, "cap"), (cap, 1, 4, "N"), (cap, 0, 4, "N"), (cap, 2, 0, "D"), (cap, 2, -1, "D"),
                          (1 << 28, 2, 4, "2^31"), (1 << 25, 4, 4, "2^31"), (cap, 2000, 4, "2^31")):
        rc, msg = _call(child, data, c, n, d)
        assert rc == RTO_E_INVALID and word in msg, (c, n, d, msg)
    # an output inside an input, an input inside an output, two outputs on one buffer
    rc, msg = ok(child_out=child)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg = ok(data_out=data.ctypes.data + 2 * 4 * 8)
    assert rc == RTO_E_INVALID and "overlap" in msg
    big = np.zeros(cap * 8 * 4 + cap * 8 * 2, np.uint16)
    rc, msg = ok(data_out=big, child_out=big.ctypes.data + 64)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg = ok(data_out=big, node_map=big.ctypes.data + 8)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg = ok(child_out=big.ctypes.data + 2)
    assert rc == RTO_E_INVALID and "aligned" in msg
    # node_map and stats are optional
    st = CSimplifyStats()
    assert ok(stats=C.byref(st))[0] == 0 and st.reachable == cap
    with pytest.raises(R.RtoError):
        simplify.simplify_tree(child.astype(np.int64), data, backend="cpu")
    with pytest.raises(R.RtoError):
        simplify.simplify_tree(child, data[:, :, :, :1], backend="cpu")
    with pytest.raises(ValueError):
        simplify.simplify_tree(child, data, backend="cuda")


# ---------------------------------------------------------------- the command
def _write_tree(path, depth_limit=5, basis_dim=4):
    t = synth.make_tree(depth_limit=depth_limit, basis_dim=basis_dim, seed=5)
    z = dict(data_dim=np.int64(t.data_dim), data_format=np.array(t.data_format), invradius3=t.scale.astype(np.float32),
             offset=t.offset.astype(np.float32), child=t.child, data=t.data, parent_depth=np.zeros((t.capacity, 2), np.int32),
             geom_resize_fact=np.float64(1.0), n_free=np.int64(0), n_internal=np.int64(t.capacity), depth_limit=np.int64(depth_limit),
             extra_data=np.arange(8, dtype=np.float32).reshape(2, 4))
    np.savez(path, **z)
    return z


def test_simplify_octree_command_on_the_host(tmp_path, capsys):
    src = str(tmp_path / "tree.npz")
    z = _write_tree(src)
    out = tmp_path / "out"
    assert simplify_octree.main([src, "--backend", "cpu", "--out_dir", str(out)]) == 0
    text = capsys.readouterr().out
    want = SR.simplify(z["child"], z["data"], None)
    assert "Nodes %d -> %d" % (z["child"].shape[0], want[0].shape[0]) in text and "MB" in text
    with np.load(str(out / "tree.npz")) as f:
        assert sorted(f.files) == sorted(k for k in z if k not in ("parent_depth", "n_free", "n_internal"))
        assert np.array_equal(f["child"], want[0]) and np.array_equal(f["data"].view(np.uint16), want[1].view(np.uint16))
        for k in ("data_dim", "data_format", "invradius3", "offset", "geom_resize_fact", "depth_limit", "extra_data"):
            assert f[k].dtype == z[k].dtype and np.array_equal(f[k], z[k]), k
    # an existing output is skipped without --overwrite; --sigma_thresh switches the kill on
    assert simplify_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--sigma_thresh", "50"]) == 0
    assert " > skip" in capsys.readouterr().out
    assert simplify_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--sigma_thresh", "50", "--overwrite"]) == 0
    capsys.readouterr()
    killed = SR.simplify(z["child"], z["data"], 50.0)
    with np.load(str(out / "tree.npz")) as f:
        assert np.array_equal(f["child"], killed[0]) and np.array_equal(f["data"].view(np.uint16), killed[1].view(np.uint16))
    assert killed[0].shape[0] < want[0].shape[0]


def test_simplify_octree_refuses_a_quantised_file(tmp_path, capsys):
    from rt_octree_amd import compress_octree
    src = str(tmp_path / "tree.npz")
    _write_tree(src, depth_limit=3)
    assert compress_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "q")]) == 0
    capsys.readouterr()
    assert simplify_octree.main([str(tmp_path / "q" / "tree.npz"), "--backend", "cpu", "--out_dir", str(tmp_path / "s")]) == 2
    err = capsys.readouterr().err
    assert "quantised" in err and "simplify" in err and "compress_octree" in err
    assert not (tmp_path / "s" / "tree.npz").exists()


def test_simplify_then_compress(tmp_path, capsys):
    """the tool chain: the compressed file of the simplified tree decodes to the simplified tree's live records"""
    from rt_octree_amd import compress_octree
    src = str(tmp_path / "tree.npz")
    _write_tree(src, depth_limit=4)
    assert simplify_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "s"), "--sigma_thresh", "2.0"]) == 0
    assert compress_octree.main([str(tmp_path / "s" / "tree.npz"), "--backend", "cpu", "--out_dir", str(tmp_path / "q")]) == 0
    capsys.readouterr()
    with np.load(str(tmp_path / "s" / "tree.npz")) as s, np.load(str(tmp_path / "q" / "tree.npz")) as q:
        assert np.array_equal(q["child"], s["child"])
        assert np.array_equal(q["sigma"].view(np.uint16), s["data"][..., -1].view(np.uint16))
