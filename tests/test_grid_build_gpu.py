"""The HIP grid builder (rto_tree_build_plan / rto_tree_build_write, csrc/build_kernels.hip) against the numpy model of
tests/grid_build_ref.py and the host twin, child / data / stats bit for bit (the definition leaves no freedom: no tolerance), the
two cross-checks against the simplifier on the device, the way back through rto_tree_query (tree_to_grid), a rendered frame of a
built tree against the CPU oracle, a 1024^3 grid (indices beyond 2^32), and the grid_to_octree command on the device against
itself on the host.

Shapes: the host tests' list -- L = 1 .. 5, D = 1, 4, 5, 13, 28, 49 (a record aligned to 2 and to 8 bytes), 4096 nodes on one
level (16 tiles of the scan), buffers that are not aligned to 16 bytes (the half-by-half scatter)."""
import ctypes as C

import numpy as np
import pytest

import grid_build_ref as GR
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import grid_build, grid_to_octree, synth
from rt_octree_amd._lib import CGridBuildStats

from helpers import assert_bits_equal, make_pair, oracle_whole_frame, rcam
from test_grid_build_host import SYNTH, sampled_synth, write_grid

pytestmark = pytest.mark.gpu

RTO_E_INVALID = -1


@pytest.fixture(scope="module")
def builder():
    b = R.TreeBuilder(0)
    yield b
    b.free()


@pytest.fixture(scope="module")
def simplifier():
    s = R.Simplifier(0)
    yield s
    s.free()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to("cuda:0")


def _run(b, grid, kill, stream=None):
    c, d, st = b.build(_dev(np.asarray(grid).view(np.float16)), kill, stream)
    return c.cpu().numpy(), d.cpu().numpy(), st


def _host(grid, kill):
    return grid_build.build_tree(np.asarray(grid).view(np.float16), kill, backend="cpu")


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_kernels_equal_model_and_host_twin(builder, name):
    grid, kill, want = GR.case(name)
    got = _run(builder, grid, kill)
    GR.assert_same(got, want, name + " vs model")
    GR.assert_same(got, _host(grid, kill), name + " vs host twin")


@pytest.mark.parametrize("name", ["hier_L3_D5_kill", "hier_L3_D28", "hier_L5_D4_kill", "hier_L3_D49_kill"])
def test_buffers_not_aligned_to_16_bytes(builder, name):
    """grid and data_out 2 bytes off a 16-byte boundary: records at odd multiples of 2 bytes, the half-by-half scatter"""
    import torch
    grid, kill, want = GR.case(name)
    L, D = grid.shape[0].bit_length() - 1, grid.shape[3]
    src = torch.zeros(grid.size + 8, dtype=torch.float16, device="cuda:0")
    src[1:1 + grid.size] = _dev(grid.view(np.float16)).reshape(-1)
    nodes = want[2]["nodes"]
    dst = torch.zeros(nodes * 8 * D + 8, dtype=torch.float16, device="cuda:0")
    child_out = torch.zeros(nodes * 8, dtype=torch.int32, device="cuda:0")
    cap, st = C.c_int64(0), CGridBuildStats()
    thresh = float("nan") if kill is None else kill
    R._lib.check(R.lib().rto_tree_build_plan(builder._h, None, C.c_void_p(src.data_ptr() + 2), L, D, thresh, C.byref(cap), C.byref(st)))
    assert (cap.value, st.nodes, st.killed, st.levels) == (nodes, nodes, want[2]["killed"], want[2]["levels"])
    R._lib.check(R.lib().rto_tree_build_write(builder._h, None, C.c_void_p(child_out.data_ptr()), C.c_void_p(dst.data_ptr() + 2)))
    torch.cuda.synchronize()
    assert np.array_equal(child_out.cpu().numpy(), want[0].reshape(-1))
    out = dst.cpu().numpy().view(np.uint16)
    assert np.array_equal(out[1:1 + nodes * 8 * D], want[1].reshape(-1).view(np.uint16))
    assert out[0] == 0 and not out[1 + nodes * 8 * D:].any()


def test_one_handle_reuses_its_scratch_large_then_small():
    b = R.TreeBuilder(0)
    try:
        large = GR.hier_grid(6, 4, 5, p=0.3)
        want = _host(large, 1.0)  # (the host tests hold the twin to the model)
        assert want[2]["nodes"] > 5000 and want[2]["levels"] == 6
        first = _run(b, large, 1.0)
        GR.assert_same(first, want, "64^3")
        small = GR.case("hier_L2_kill")
        GR.assert_same(_run(b, small[0], small[1]), small[2], "4^3 after 64^3")
        GR.assert_same(_run(b, large, 1.0), first, "third call")
    finally:
        b.free()


def test_two_runs_are_bit_identical_and_streams_agree(builder):
    import torch
    grid, kill, want = GR.case("hier_L5_D4_kill")
    a = _run(builder, grid, kill)
    GR.assert_same(_run(builder, grid, kill), a, "second run")
    s = torch.cuda.Stream()
    dg = _dev(grid.view(np.float16))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c, d, st = builder.build(dg, kill, s)
    s.synchronize()
    GR.assert_same((c.cpu().numpy(), d.cpu().numpy(), st), want, "non-default stream")


def test_argument_refusals(builder):
    import torch
    grid, _, want = GR.case("hier_L2")
    nodes = want[2]["nodes"]
    dg = _dev(grid.view(np.float16))
    co = torch.full((nodes * 8,), 7, dtype=torch.int32, device="cuda:0")
    do = torch.zeros(nodes * 8 * 4, dtype=torch.float16, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    oc = C.c_int64(0)
    L = R.lib()

    def refused(rc):
        msg = L.rto_last_error().decode()
        assert rc == RTO_E_INVALID and msg, (rc, msg)
        return msg

    fresh = R.TreeBuilder(0)
    try:
        assert "no successful" in refused(L.rto_tree_build_write(fresh._h, None, P(co), P(do)))
    finally:
        fresh.free()
    h, nan = builder._h, float("nan")
    assert "null" in refused(L.rto_tree_build_plan(None, None, P(dg), 2, 4, nan, C.byref(oc), None))
    assert "null" in refused(L.rto_tree_build_plan(h, None, None, 2, 4, nan, C.byref(oc), None))
    assert "null" in refused(L.rto_tree_build_plan(h, None, P(dg), 2, 4, nan, None, None))
    assert "L must" in refused(L.rto_tree_build_plan(h, None, P(dg), 0, 4, nan, C.byref(oc), None))
    assert "L must" in refused(L.rto_tree_build_plan(h, None, P(dg), 11, 4, nan, C.byref(oc), None))
    assert "D must" in refused(L.rto_tree_build_plan(h, None, P(dg), 2, 0, nan, C.byref(oc), None))
    assert "aligned" in refused(L.rto_tree_build_plan(h, None, C.c_void_p(dg.data_ptr() + 1), 2, 4, nan, C.byref(oc), None))
    assert "grid is not memory" in refused(L.rto_tree_build_plan(h, None, C.c_void_p(grid.ctypes.data), 2, 4, nan, C.byref(oc), None))
    # a refused plan leaves the handle without one
    assert "no successful" in refused(L.rto_tree_build_write(h, None, P(co), P(do)))
    R._lib.check(L.rto_tree_build_plan(h, None, P(dg), 2, 4, nan, C.byref(oc), None))
    assert oc.value == nodes
    assert "null" in refused(L.rto_tree_build_write(h, None, None, P(do)))
    assert "null" in refused(L.rto_tree_build_write(h, None, P(co), None))
    assert "aligned" in refused(L.rto_tree_build_write(h, None, C.c_void_p(co.data_ptr() + 2), P(do)))
    assert "aligned" in refused(L.rto_tree_build_write(h, None, P(co), C.c_void_p(do.data_ptr() + 1)))
    assert "overlaps an input" in refused(L.rto_tree_build_write(h, None, P(co), C.c_void_p(dg.data_ptr() + 16)))
    assert "outputs overlap" in refused(L.rto_tree_build_write(h, None, P(do), C.c_void_p(do.data_ptr() + 16)))
    host_out = np.zeros(nodes * 8 * 4, np.uint16)
    assert "data_out is not memory" in refused(L.rto_tree_build_write(h, None, P(co), C.c_void_p(host_out.ctypes.data)))
    host_child = np.zeros(nodes * 8, np.int32)
    assert "child_out is not memory" in refused(L.rto_tree_build_write(h, None, C.c_void_p(host_child.ctypes.data), P(do)))
    torch.cuda.synchronize()
    assert (co == 7).all()  # nothing was enqueued
    R._lib.check(L.rto_tree_build_write(h, None, P(co), P(do)))  # the plan is still good
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), want[0].reshape(-1))
    assert np.array_equal(do.cpu().numpy().view(np.uint16), want[1].reshape(-1).view(np.uint16))


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_cross_check_a_on_the_device(builder, simplifier, name):
    """the grid's full octree through the HIP simplifier with the same threshold: the HIP builder's bytes"""
    grid, kill, _ = GR.case(name)
    fc, fd = GR.full_tree(grid)
    c, d, _, st = simplifier.simplify(_dev(fc), _dev(fd), kill)
    got = _run(builder, grid, kill)
    assert np.array_equal(got[0], c.cpu().numpy()) and np.array_equal(got[1].view(np.uint16), d.cpu().numpy().view(np.uint16))
    assert got[2]["killed"] == st["killed"] and got[2]["levels"] == st["levels"]
    assert got[2]["nodes"] == st["reachable"] - st["merged"]


@pytest.fixture(scope="module")
def device_sampled():
    """(depth, basis) -> the half device tensor tree_to_grid returns for the uploaded synthetic tree"""
    out = {}
    for depth, basis in SYNTH:
        t = SR.synth_tree(depth, basis)
        dt = R.N3Tree.from_arrays(t.child, t.data, t.scale, t.offset, t.data_format)
        out[(depth, basis)] = R.tree_to_grid(dt, depth)
        dt.free()
    return out


@pytest.mark.parametrize("depth,basis", SYNTH)
def test_tree_to_grid_equals_the_numpy_walk(device_sampled, depth, basis):
    g = device_sampled[(depth, basis)]
    assert tuple(g.shape) == (1 << depth,) * 3 + (3 * basis + 1,)
    assert np.array_equal(g.cpu().numpy().view(np.uint16), sampled_synth(depth, basis)[2])


@pytest.mark.parametrize("kill", [None, 0.0, 50.0])
@pytest.mark.parametrize("depth,basis", SYNTH)
def test_cross_check_b_on_the_device(builder, simplifier, device_sampled, depth, basis, kill):
    """a tree sampled on the device and rebuilt there is the tree the HIP simplifier makes of it"""
    child, data, _ = sampled_synth(depth, basis)
    c, d, _, st = simplifier.simplify(_dev(child), _dev(data), kill)
    gc, gd, gst = builder.build(device_sampled[(depth, basis)], kill)
    assert np.array_equal(gc.cpu().numpy(), c.cpu().numpy())
    assert np.array_equal(gd.cpu().numpy().view(np.uint16), d.cpu().numpy().view(np.uint16))
    assert gst["nodes"] == c.shape[0] and gst["levels"] == st["levels"]


@pytest.mark.parametrize("D,fmt", [(13, "SH4"), (28, "SH9")])
def test_round_trip_grid_tree_grid(builder, D, fmt):
    """build, upload, sample at the voxel centres: the input's bits, zeros where killed"""
    grid = GR.hier_grid(4, D, 60 + D)
    kill = 1.0
    c, d, st = _run(builder, grid, kill)
    assert st["killed"] > 100 and 1 < st["nodes"] < 585
    tree = R.N3Tree.from_arrays(c, d, np.ones(3, np.float32), np.zeros(3, np.float32), fmt)
    back = R.tree_to_grid(tree, 4).cpu().numpy().view(np.uint16)
    tree.free()
    want = grid.copy()
    want[~(grid[..., -1].view(np.float16) > np.float16(kill))] = 0
    assert np.array_equal(back, want)


def test_a_built_tree_renders_like_the_oracle_renders_it(builder, device_sampled):
    ref = SR.synth_tree(5, 1)
    c, d, st = builder.build(device_sampled[(5, 1)], None)
    assert st["nodes"] < ref.child.shape[0]
    t = synth.SynthTree(c.cpu().numpy(), d.cpu().numpy(), ref.scale, ref.offset, ref.data_format, 5, {})
    ht, dt = make_pair(t)
    W, H, spp, jump = 32, 24, 6, 3
    cam = rcam(W, H, synth.orbit_poses(8)[1])
    ctx = R.RenderContext(W, H)
    R.launch_renderer_batch(dt, [cam], R.RenderOptions(spp=spp, denoise=False), ctx, rng_jumps=[jump])
    aux = ctx.download_aux()
    aux_o, _ = oracle_whole_frame(ht, cam, cam.fx, spp, jump)
    assert (aux[3] > 0).mean() > 0.05
    assert_bits_equal(aux, aux_o, "built tree")
    dt.free()


def test_indices_beyond_32_bits():
    """L = 10, D = 4: 2^32 halves, one dense voxel in the far corner.  The result is known without a twin: a chain of ten nodes
    through slot 7, the record in the last slot of the last node."""
    import torch
    try:
        grid = torch.zeros((1024, 1024, 1024, 4), dtype=torch.float16, device="cuda:0")
    except RuntimeError as e:  # (torch.cuda.OutOfMemoryError is one)
        pytest.skip("no room for an 8 GiB grid: %s" % str(e).splitlines()[0])
    rec = torch.tensor([0.5, -1.0, 2.0, 3.0], dtype=torch.float16, device="cuda:0")
    grid[1023, 1023, 1023] = rec
    b = R.TreeBuilder(0)
    try:
        c, d, st = b.build(grid, None)
        c, d = c.cpu().numpy().reshape(-1, 8), d.cpu().numpy().reshape(-1, 8, 4)
    finally:
        b.free()
        del grid
        torch.cuda.empty_cache()
    assert st == dict(nodes=10, killed=0, levels=10)
    want_c = np.zeros((10, 8), np.int32)
    want_c[:9, 7] = 1
    want_d = np.zeros((10, 8, 4), np.float16)
    want_d[9, 7] = rec.cpu().numpy()
    assert np.array_equal(c, want_c) and np.array_equal(d.view(np.uint16), want_d.view(np.uint16))


def test_grid_to_octree_on_the_device_writes_the_host_file(tmp_path, capsys):
    src = str(tmp_path / "grid.npz")
    write_grid(src, L=4)
    common = [src, "--sigma_thresh", "1.0004"]
    assert grid_to_octree.main(common + ["--backend", "cpu", "--out_dir", str(tmp_path / "cpu")]) == 0
    assert grid_to_octree.main(common + ["--backend", "hip", "--out_dir", str(tmp_path / "hip")]) == 0
    assert "voxels killed" in capsys.readouterr().out
    with open(str(tmp_path / "cpu" / "tree.npz"), "rb") as a, open(str(tmp_path / "hip" / "tree.npz"), "rb") as b:
        assert a.read() == b.read()
    tree = R.N3Tree(str(tmp_path / "hip" / "tree.npz"))  # the loader takes it
    assert tree.N == 2 and tree.data_dim == 7
    tree.free()
