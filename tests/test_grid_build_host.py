"""The host twin of the grid builder (rto_tree_build_host, csrc/host/grid_build.cpp) against the numpy model of
tests/grid_build_ref.py, bit for bit (include/rto.h "grid builder" leaves nothing to an implementation: there is no tolerance),
the two cross-checks against the simplifier (the grid's full octree simplified; a synthetic tree sampled and rebuilt), every
refusal, and the grid_to_octree command on the host.  No GPU is touched."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import grid_build_ref as GR
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import grid_build, grid_to_octree, simplify
from rt_octree_amd._lib import CGridBuildStats

RTO_E_INVALID = -1


def _host(grid, kill):
    return grid_build.build_tree(np.asarray(grid).view(np.float16), kill, backend="cpu")


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_host_twin_equals_the_model(name):
    grid, kill, want = GR.case(name)
    GR.assert_same(_host(grid, kill), want, name)


def test_what_the_cases_cover():
    n = lambda name: GR.case(name)[2][2]  # noqa: E731
    assert n("single_voxel_L1") == dict(nodes=1, killed=0, levels=1)
    assert n("all_zero") == dict(nodes=1, killed=0, levels=1) and n("all_zero_kill") == dict(nodes=1, killed=512, levels=1)
    assert n("uniform_nonzero")["nodes"] == 1 and n("equal_nan_records")["nodes"] == 1
    assert n("nan_records_differ_in_payload")["nodes"] == 2
    assert n("random_L5_D1") == dict(nodes=4681, killed=0, levels=5)  # 4096 nodes on the deepest level
    assert n("single_voxel_L4") == dict(nodes=4, killed=0, levels=4)  # a chain of L nodes
    assert n("single_voxel_L4_kill") == dict(nodes=4, killed=4095, levels=4)
    for p in range(8):
        assert n("one_voxel_differs_%d" % p)["nodes"] == 2
    for k in ("first_half_differs", "middle_half_differs", "last_half_differs", "plus_zero_against_minus_zero", "minus_zero_density"):
        assert n(k)["nodes"] == 2, k
    assert n("minus_zero_density_kill") == dict(nodes=1, killed=64, levels=1)  # -0 is not above 0: dead like the rest
    assert n("kill_makes_uniform") == dict(nodes=8, killed=8, levels=2) and n("kill_makes_uniform_without_kill")["nodes"] == 9
    assert n("kill_beyond_fp16") == dict(nodes=1, killed=512, levels=1)
    assert n("octant_uniform") == dict(nodes=1 + 7 + 56 + 448, killed=0, levels=4)  # the octant's 1 + 8 + 64 nodes collapse
    assert n("kill_rounded") == GR.build(GR.case("kill_rounded")[0], 0.25)[2]
    child, data, _ = GR.case("kill_makes_uniform")[2]
    assert child.reshape(-1, 8)[0, 0] == 0 and not data.view(np.uint16).reshape(-1, 8, 4)[0, 0].any()  # one zero leaf
    # a NaN density is a record like any other without the kill and dead with it
    grid = GR.case("nan_density")[0]
    nan = (grid[..., -1] & 0x7FFF) > 0x7C00
    assert nan.sum() > 10 and n("nan_density_kill0")["killed"] >= int(nan.sum())
    # uniform regions of every size merge
    assert 1 < n("hier_L4")["nodes"] < 585 and n("hier_L4")["levels"] == 4


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_cross_check_a_the_simplifier_on_the_full_octree(name):
    """the grid's full octree through simplify_tree with the same threshold: the builder's bytes"""
    grid, kill, _ = GR.case(name)
    fc, fd = GR.full_tree(grid)
    c, d, _, st = simplify.simplify_tree(fc, fd, kill, backend="cpu")
    got = _host(grid, kill)
    assert np.array_equal(got[0], c) and np.array_equal(got[1].view(np.uint16), d.view(np.uint16))
    assert got[2]["killed"] == st["killed"] and got[2]["levels"] == st["levels"]
    assert got[2]["nodes"] == st["reachable"] - st["merged"] == c.shape[0]


SYNTH = ((3, 1), (5, 1), (6, 4))  # (depth_limit, basis_dim)


@functools.lru_cache(maxsize=None)
def sampled_synth(depth, basis):
    """the synthetic tree, and its records at the centres of the 2^depth grid by the numpy walk"""
    child, data = SR._arrays(SR.synth_tree(depth, basis))
    grid = GR.sample_tree(child, data, depth)
    grid.setflags(write=False)
    return child, data, grid


@pytest.mark.parametrize("kill", [None, 0.0, 50.0])
@pytest.mark.parametrize("depth,basis", SYNTH)
def test_cross_check_b_a_sampled_tree_rebuilds_to_its_simplified_self(depth, basis, kill):
    child, data, grid = sampled_synth(depth, basis)
    c, d, _, st = simplify.simplify_tree(child, data, kill, backend="cpu")
    got = _host(grid, kill)
    assert np.array_equal(got[0], c) and np.array_equal(got[1].view(np.uint16), d.view(np.uint16))
    assert got[2]["nodes"] == c.shape[0] and got[2]["levels"] == st["levels"]
    if (depth, basis, kill) == (6, 4, None):
        assert (child.shape[0], c.shape[0]) == (4087, 2839)


# ---------------------------------------------------------------- refusals
def _call(grid, L, D, kill=float("nan"), child_out=None, data_out=None, room=0, out_cap=0, stats=None):
    """the raw entry; an int for a pointer is passed as that address"""
    keep = []

    def ptr(a):
        if a is None:
            return None
        if isinstance(a, int):
            return C.c_void_p(a)
        keep.append(a)
        return C.c_void_p(a.ctypes.data)
    oc = C.c_int64(-7) if out_cap == 0 else out_cap
    rc = R.lib().rto_tree_build_host(ptr(grid), L, D, kill, ptr(child_out), ptr(data_out), room, C.byref(oc) if oc is not None else None, stats)
    return rc, R.lib().rto_last_error().decode(), (oc.value if oc is not None else None)


def test_refuses_arguments():
    grid, _, want = GR.case("hier_L2")
    nodes = want[2]["nodes"]
    co, do = np.zeros(nodes * 8, np.int32), np.zeros(nodes * 8 * 4 + 8, np.uint16)
    assert _call(grid, 2, 4, child_out=co, data_out=do, room=nodes)[0] == 0
    for kw, word in ((dict(out_cap=None), "null"), (dict(child_out=co), "null"), (dict(data_out=do), "null")):
        rc, msg, _ = _call(grid, 2, 4, **kw)
        assert rc == RTO_E_INVALID and word in msg, (kw, msg)
    rc, msg, _ = _call(None, 2, 4)
    assert rc == RTO_E_INVALID and "null" in msg
    for L in (0, -1, 11):
        rc, msg, _ = _call(grid, L, 4)
        assert rc == RTO_E_INVALID and "L must lie in 1 .. 10" in msg, (L, msg)
    for D in (0, -3):
        rc, msg, _ = _call(grid, 2, D)
        assert rc == RTO_E_INVALID and "D must be at least 1" in msg, (D, msg)
    rc, msg, _ = _call(grid.ctypes.data + 1, 2, 4)
    assert rc == RTO_E_INVALID and "grid is not aligned" in msg
    rc, msg, _ = _call(grid, 2, 4, child_out=co.ctypes.data + 2, data_out=do, room=nodes - 1)
    assert rc == RTO_E_INVALID and "child_out is not aligned" in msg
    rc, msg, _ = _call(grid, 2, 4, child_out=co, data_out=do.ctypes.data + 1, room=nodes)
    assert rc == RTO_E_INVALID and "data_out is not aligned" in msg
    # an output inside the input, the two outputs on one buffer
    g = np.zeros(64 * 4 + 64, np.uint16)
    rc, msg, _ = _call(g, 2, 4, child_out=co, data_out=g.ctypes.data + 64, room=nodes)
    assert rc == RTO_E_INVALID and "overlaps an input" in msg
    rc, msg, _ = _call(g, 2, 4, child_out=g.ctypes.data + 16, data_out=do, room=nodes)
    assert rc == RTO_E_INVALID and "overlaps an input" in msg
    big = np.zeros(nodes * 8 * 6, np.uint16)
    rc, msg, _ = _call(grid, 2, 4, child_out=big, data_out=big.ctypes.data + 8, room=nodes)
    assert rc == RTO_E_INVALID and "outputs overlap" in msg
    with pytest.raises(R.RtoError):
        grid_build.build_tree(np.zeros((4, 4, 2, 4), np.float16), backend="cpu")
    with pytest.raises(R.RtoError):
        grid_build.build_tree(np.zeros((3, 3, 3, 4), np.float16), backend="cpu")
    with pytest.raises(R.RtoError):
        grid_build.build_tree(np.zeros((4, 4, 4, 4), np.int16), backend="cpu")
    with pytest.raises(ValueError):
        grid_build.build_tree(np.zeros((4, 4, 4, 4), np.float16), backend="cuda")
    # (the refusal of a result with nodes * 8 >= 2^31 needs a grid of 2^28 mixed cells: 1024^3 voxels; it is one comparison
    # in code both entries share and is not run here)


def test_room_too_small_and_count_only():
    grid, kill, want = GR.case("hier_L3_D5_kill")
    nodes = want[2]["nodes"]
    assert nodes > 2
    st = CGridBuildStats()
    rc, _, cap = _call(grid, 3, 5, kill, stats=C.byref(st))  # count only: no outputs
    assert rc == 0 and cap == nodes and (st.nodes, st.killed, st.levels) == (nodes, want[2]["killed"], want[2]["levels"])
    co, do = np.full(nodes * 8, 7, np.int32), np.full(nodes * 8 * 5, 7, np.uint16)
    st = CGridBuildStats()
    rc, msg, cap = _call(grid, 3, 5, kill, child_out=co, data_out=do, room=nodes - 1, stats=C.byref(st))
    assert rc == RTO_E_INVALID and "room for %d nodes, the tree has %d" % (nodes - 1, nodes) in msg
    assert cap == nodes and st.nodes == nodes and (co == 7).all() and (do == 7).all()
    rc, _, cap = _call(grid, 3, 5, kill, child_out=co, data_out=do, room=nodes)
    assert rc == 0 and np.array_equal(co, want[0].reshape(-1)) and np.array_equal(do, want[1].view(np.uint16).reshape(-1))
    co2, do2 = np.full((nodes + 3) * 8, 7, np.int32), np.full((nodes + 3) * 8 * 5, 7, np.uint16)
    rc, _, cap = _call(grid, 3, 5, kill, child_out=co2, data_out=do2, room=nodes + 3)  # more room than needed stays untouched
    assert rc == 0 and cap == nodes and np.array_equal(co2[:nodes * 8], co) and (co2[nodes * 8:] == 7).all() and (do2[nodes * 40:] == 7).all()


def test_a_float32_grid_is_rounded_by_numpy_first():
    g16 = GR.case("hier_L3_D5")[0].view(np.float16)
    rng = np.random.default_rng(2)
    g32 = g16.astype(np.float32) * (1 + rng.uniform(-1e-4, 1e-4, g16.shape).astype(np.float32))  # rounds back to g16
    assert np.array_equal(g32.astype(np.float16).view(np.uint16), g16.view(np.uint16)) and (g32 != g16).any()
    GR.assert_same(grid_build.build_tree(g32, None, backend="cpu"), GR.case("hier_L3_D5")[2], "float32 input")


# ---------------------------------------------------------------- the command
def _probe(path):
    buf = C.create_string_buffer(4096)
    assert R.lib().rto_tree_probe_npz(os.fsencode(str(path)), buf, 4096) == 0, R.lib().rto_last_error()
    return json.loads(buf.value.decode())


def write_grid(path, dtype=np.float16, with_format=True, L=3, basis=2, extra=True):
    g = GR.hier_grid(L, 3 * basis + 1, 77, densities=[0, GR.H(0.25), GR.H(2.0), GR.H(40.0)]).view(np.float16)
    z = dict(grid=g.astype(dtype))
    if with_format:
        z["data_format"] = np.array("SH%d" % basis)
    if extra:
        z["extra_data"] = np.arange(8, dtype=np.float32).reshape(2, 4)
    np.savez(path, **z)
    return g


def test_grid_to_octree_command_on_the_host(tmp_path, capsys):
    src = str(tmp_path / "grid.npz")
    g = write_grid(src)
    out = tmp_path / "out"
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--radius", "1.5", "--center", "0.25", "0", "-0.5"]) == 0
    text = capsys.readouterr().out
    want = GR.build(g, None)
    assert "Nodes %d, 0 voxels killed, %d levels" % (want[2]["nodes"], want[2]["levels"]) in text and "MB" in text
    with np.load(str(out / "tree.npz")) as f:
        assert sorted(f.files) == sorted(["data_dim", "data_format", "invradius3", "offset", "child", "data", "extra_data"])
        assert f["child"].dtype == np.int32 and np.array_equal(f["child"], want[0])
        assert f["data"].dtype == np.float16 and np.array_equal(f["data"].view(np.uint16), want[1].view(np.uint16))
        assert int(f["data_dim"]) == 7 and str(f["data_format"]) == "SH2"
        assert f["invradius3"].dtype == np.float32 and np.array_equal(f["invradius3"], np.full(3, np.float32(0.5 / 1.5)))
        assert np.allclose(f["offset"], 0.5 * (1 - np.array([0.25, 0, -0.5]) / 1.5), rtol=1e-6) and f["offset"].dtype == np.float32
        assert np.array_equal(f["extra_data"], np.arange(8, dtype=np.float32).reshape(2, 4))
    info = _probe(out / "tree.npz")  # the loader takes the file
    assert (info["capacity"], info["N"], info["data_dim"], info["data_format"]) == (want[2]["nodes"], 2, 7, "SH2")
    # an existing output is skipped without --overwrite; --sigma_thresh switches the kill on
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--sigma_thresh", "1"]) == 0
    assert " > skip" in capsys.readouterr().out
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--sigma_thresh", "1", "--overwrite"]) == 0
    killed = GR.build(g, 1.0)
    assert "%d voxels killed" % killed[2]["killed"] in capsys.readouterr().out and killed[2]["killed"] > 0
    with np.load(str(out / "tree.npz")) as f:
        assert np.array_equal(f["child"], killed[0]) and np.array_equal(f["data"].view(np.uint16), killed[1].view(np.uint16))
        assert np.array_equal(f["invradius3"], np.ones(3, np.float32)) and np.array_equal(f["offset"], np.zeros(3, np.float32))


def test_grid_to_octree_takes_float32_and_the_flag_for_the_format(tmp_path, capsys):
    src = str(tmp_path / "grid.npz")
    g = write_grid(src, dtype=np.float32, with_format=False, extra=False)
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "a")]) == 2
    err = capsys.readouterr().err
    assert "data_format" in err and "--data_format" in err and not (tmp_path / "a" / "tree.npz").exists()
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "a"), "--data_format", "SH3"]) == 2
    assert "SH3 does not describe records of 7 values" in capsys.readouterr().err
    assert grid_to_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "a"), "--data_format", "SH2"]) == 0
    capsys.readouterr()
    want = GR.build(g, None)
    with np.load(str(tmp_path / "a" / "tree.npz")) as f:
        assert "extra_data" not in f.files and str(f["data_format"]) == "SH2"
        assert np.array_equal(f["child"], want[0]) and np.array_equal(f["data"].view(np.uint16), want[1].view(np.uint16))
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, grid=np.zeros((4, 4, 4, 4), np.int32), data_format=np.array("RGBA"))
    assert grid_to_octree.main([bad, "--backend", "cpu", "--out_dir", str(tmp_path / "b")]) == 2
    assert "float16 or float32" in capsys.readouterr().err
    np.savez(bad, grid=np.zeros((6, 6, 6, 4), np.float16), data_format=np.array("RGBA"))
    assert grid_to_octree.main([bad, "--backend", "cpu", "--out_dir", str(tmp_path / "b")]) == 2
    assert "power of two" in capsys.readouterr().err
