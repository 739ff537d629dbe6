"""The HIP tree refiner (rto_tree_refine_plan / rto_tree_refine_write, csrc/refine_kernels.hip) against the numpy model of
tests/refine_ref.py and the host twin, child / data / slot_src / stats bit for bit (the definition leaves no freedom: no
tolerance), and what the refined tree does downstream on the device: point queries, the simplifier, the batched render against
the CPU oracle on that same tree, ten SGD steps of the fit with params carried through slot_src, and the two commands on the
device against themselves on the host.

Shapes: the host tests' list -- D = 4, 5, 13, 28, N = 2 and 4, negative offsets, garbage nodes, 1 .. 32 levels -- and those at
which the kernels, not the definition, can go wrong: 0, 1, 1023, 1024 and 1025 candidates; trees of 127, 128 and 129 nodes (one
tile of 1024 slots and one node either side); 18885 nodes; 300001 nodes (2344 tiles of slots: the scan of the tile counts takes
ten chunks of 256) with all keys equal (every lane of every wave in one bin of the histogram, the cut inside a tile of equal
keys), with four key values and with random keys; buffers that are not aligned to 16 bytes (the half-by-half write)."""
import ctypes as C

import numpy as np
import pytest

import refine_ref as RR
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import optimize_octree, refine, refine_octree, synth
from rt_octree_amd._lib import CRefineStats

from helpers import assert_bits_equal, make_pair, oracle_whole_frame, rcam
from test_refine_host import TOOL_ARGS, fit_scene, too_large_tree
from test_simplify_host import _write_tree

pytestmark = pytest.mark.gpu

RTO_E_INVALID, RTO_E_FORMAT = -1, -6


@pytest.fixture(scope="module")
def refiner():
    r = R.Refiner(0)
    yield r
    r.free()


def _dev(a):
    import torch
    a = np.array(a, order="C", copy=True)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _run(r, child, data, key=None, key_thresh=1, max_new=-1, max_level=31, stream=None):
    import torch
    c, d, s, st = r.refine(_dev(child), _dev(data), None if key is None else _dev(key), key_thresh, max_new, max_level, stream)
    (stream or torch.cuda.current_stream()).synchronize()
    return c.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy(), st


@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_kernels_equal_model_and_host_twin(refiner, name):
    child, data, key, thresh, max_new, max_level, want = RR.case(name)
    got = _run(refiner, child, data, key, thresh, max_new, max_level)
    RR.assert_same(got, want, name + " vs model")
    RR.assert_same(got, refine.refine_tree(child, data, key, thresh, max_new, max_level, backend="cpu"), name + " vs host twin")


@pytest.mark.parametrize("count", [0, 1, 1023, 1024, 1025])
def test_candidate_counts_around_one_tile(refiner, count):
    """`count` candidates spread over the 8120 slots of the depth-5 tree, with and without a budget one below the count"""
    child, data = RR.tree("sh4_depth5_shuffled_lossless")
    cand = RR.candidates_of(child)[0]
    rng = np.random.default_rng(count)
    key = np.zeros(child.size, np.uint32)
    key[rng.choice(cand, count, replace=False)] = rng.integers(1, 4, count).astype(np.uint32)
    key = key.reshape(child.shape)
    for max_new in [-1] + ([count - 1] if count else []):
        want = RR.refine(child, data, key, 1, max_new)
        assert want[3]["candidates"] == count
        RR.assert_same(_run(refiner, child, data, key, 1, max_new), want, "%d candidates, budget %d" % (count, max_new))


def full_tree(counts, D, seed=3):
    """nodes per level `counts`, the nodes of a level hanging below the first nodes of the level above"""
    cap = sum(counts)
    child = np.zeros((cap, 8), np.int32)
    first = np.cumsum([0] + list(counts))
    for l in range(len(counts) - 1):
        slots = np.arange(counts[l + 1])
        parent = first[l] + slots // 8
        child[parent, slots % 8] = (first[l + 1] + slots) - parent
    data = np.random.default_rng(seed).standard_normal((cap, 8, D)).astype(np.float16)
    return child.reshape(cap, 2, 2, 2), data.reshape(cap, 2, 2, 2, D)


@pytest.mark.parametrize("nodes", [127, 128, 129])
def test_trees_of_one_tile_of_slots_and_a_node_either_side(refiner, nodes):
    child, data = full_tree([1, 8, 64, nodes - 73], 5)
    assert child.size in (1016, 1024, 1032)
    key = RR.random_keys(child.shape, nodes, "few")
    for max_new in (-1, 300):
        RR.assert_same(_run(refiner, child, data, key, 1, max_new), RR.refine(child, data, key, 1, max_new), "%d nodes" % nodes)


def test_19_tiles_of_nodes(refiner):
    child, data = SR._arrays(SR.synth_tree(7, 1))
    assert child.shape[0] == 18885
    key = RR.density_keys(data)
    for max_new in (-1, 5000):
        RR.assert_same(_run(refiner, child, data, key, 1, max_new), RR.refine(child, data, key, 1, max_new), "18885 nodes")


@pytest.fixture(scope="module")
def wide():
    from test_simplify_gpu import wide_tree
    child, data = wide_tree()
    assert child.shape[0] == 300001 and child.size > 256 * 1024 * 8  # more than one chunk of tile counts, by far
    return child, data


@pytest.mark.parametrize("kind", ["all_equal", "few", "wide"])
def test_300001_nodes(refiner, wide, kind):
    """2.4 M slots.  all_equal: key == NULL with a budget, so all four histogram passes run with every lane of every wave in
    one bin, and the cut falls inside a tile of equal keys."""
    child, data = wide
    key = None if kind == "all_equal" else RR.random_keys(child.shape, 5, kind)
    max_new = {"all_equal": 100000, "few": 700001, "wide": 123457}[kind]
    want = RR.refine(child, data, key, 1, max_new)
    assert want[3]["selected"] == max_new and want[3]["candidates"] == 300001 * 8 - 300000
    if kind == "all_equal":
        last = int(want[2].reshape(-1)[-1])  # the last slot taken: neither the first nor the last of its tile
        assert want[3]["cut_key"] == 1 and 0 < last % 1024 < 1023
    got = _run(refiner, child, data, key, 1, max_new)
    RR.assert_same(got, want, kind + " vs model")
    RR.assert_same(got, refine.refine_tree(child, data, key, 1, max_new, backend="cpu"), kind + " vs host twin")


@pytest.mark.parametrize("name", ["sh4_depth6_wide_budget", "sh9_depth4_wide_budget", "n4_wide_budget", "chain_of_five_budget",
                                  "root_made_uniform_one"])
def test_buffers_not_aligned_to_16_bytes(refiner, name):
    """data and data_out 2 bytes off a 16-byte boundary: the half-by-half write (D = 4, 28, 5 with N = 4, 13, 5)"""
    import torch
    child, data, key, thresh, max_new, max_level, want = RR.case(name)
    cap, N, D = child.shape[0], child.shape[1], data.shape[-1]
    S = N ** 3
    src = torch.zeros(data.size + 8, dtype=torch.float16, device="cuda:0")
    src[1:1 + data.size] = _dev(data).reshape(-1)
    dc, dk = _dev(child), (None if key is None else _dev(key))
    out_cap, st = C.c_int64(0), CRefineStats()
    R._lib.check(R.lib().rto_tree_refine_plan(refiner._h, None, C.c_void_p(dc.data_ptr()), None if dk is None else C.c_void_p(dk.data_ptr()), cap, N, thresh, max_new,
                                              max_level, C.byref(out_cap), C.byref(st)))
    k = out_cap.value
    assert k == want[0].shape[0] and st.selected == want[3]["selected"] and st.cut_key == want[3]["cut_key"]
    dst = torch.zeros(k * S * D + 8, dtype=torch.float16, device="cuda:0")
    child_out = torch.zeros(k * S, dtype=torch.int32, device="cuda:0")
    slot_src = torch.zeros(k * S, dtype=torch.int32, device="cuda:0")
    R._lib.check(R.lib().rto_tree_refine_write(refiner._h, None, C.c_void_p(dc.data_ptr()), C.c_void_p(src.data_ptr() + 2), D,
                                               C.c_void_p(child_out.data_ptr()), C.c_void_p(dst.data_ptr() + 2), C.c_void_p(slot_src.data_ptr())))
    torch.cuda.synchronize()
    assert np.array_equal(child_out.cpu().numpy(), want[0].reshape(-1)) and np.array_equal(slot_src.cpu().numpy(), want[2].reshape(-1))
    out = dst.cpu().numpy().view(np.uint16)
    assert np.array_equal(out[1:1 + k * S * D], want[1].reshape(-1).view(np.uint16))
    assert out[0] == 0 and not out[1 + k * S * D:].any()
    # without slot_src
    child_out.zero_()
    R._lib.check(R.lib().rto_tree_refine_write(refiner._h, None, C.c_void_p(dc.data_ptr()), C.c_void_p(src.data_ptr() + 2), D,
                                               C.c_void_p(child_out.data_ptr()), C.c_void_p(dst.data_ptr() + 2), None))
    torch.cuda.synchronize()
    assert np.array_equal(child_out.cpu().numpy(), want[0].reshape(-1))


def test_two_runs_are_bit_identical_and_streams_agree(refiner):
    import torch
    child, data, key, thresh, max_new, max_level, want = RR.case("sh4_depth6_few_budget1000")
    a = _run(refiner, child, data, key, thresh, max_new, max_level)
    b = _run(refiner, child, data, key, thresh, max_new, max_level)
    RR.assert_same(b, a, "second run")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = _run(refiner, child, data, key, thresh, max_new, max_level, stream=s)
    RR.assert_same(got, want, "non-default stream")


def test_the_write_uses_the_last_plan_and_needs_one():
    import torch
    child, data, key, thresh, _, _, _ = RR.case("sh4_depth6_wide_budget")
    r = R.Refiner(0)
    try:
        dc, dd, dk = _dev(child), _dev(data), _dev(key)
        co = torch.full((child.size,), 7, dtype=torch.int32, device="cuda:0")
        do = torch.zeros(data.size, dtype=torch.float16, device="cuda:0")
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = R.lib().rto_tree_refine_write(r._h, None, P(dc), P(dd), data.shape[-1], P(co), P(do), None)
        assert rc == RTO_E_INVALID and "rto_tree_refine_plan" in R.lib().rto_last_error().decode()
        first, _ = r.plan(dc, dk, thresh, 2500)
        second, st = r.plan(dc, dk, thresh, 40)
        assert first == child.shape[0] + 2500 and second == child.shape[0] + 40
        c, d, s = r.write(dc, dd, second)
        torch.cuda.synchronize()
        RR.assert_same((c.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy(), st), RR.refine(child, data, key, thresh, 40), "second plan")
        # a refused plan leaves no plan behind
        bad, _ = SR.malformed("shared_child")
        with pytest.raises(R.RtoError) as e:
            r.plan(_dev(bad))
        assert e.value.code == RTO_E_FORMAT
        rc = R.lib().rto_tree_refine_write(r._h, None, P(dc), P(dd), data.shape[-1], P(co), P(do), None)
        assert rc == RTO_E_INVALID
        torch.cuda.synchronize()
        assert (co == 7).all()
    finally:
        r.free()


@pytest.mark.parametrize("kind", SR.MALFORMED + ("too_deep",))
def test_malformed_links_are_refused(refiner, kind):
    child, data = SR.too_deep() if kind == "too_deep" else SR.malformed(kind)
    with pytest.raises(R.RtoError) as e:
        _run(refiner, child, data)
    assert e.value.code == RTO_E_FORMAT and e.value.msg
    ok = RR.case("sh4_depth3_mask")  # the handle is fine afterwards
    RR.assert_same(_run(refiner, ok[0], ok[1]), ok[6], "after the refusal")


def test_a_result_that_is_too_large_is_refused_by_the_plan(refiner):
    child, _ = too_large_tree()
    dc = _dev(child)
    out_cap, st = C.c_int64(0), CRefineStats()
    rc = R.lib().rto_tree_refine_plan(refiner._h, None, C.c_void_p(dc.data_ptr()), None, 128, 16, 1, -1, 31, C.byref(out_cap), C.byref(st))
    n = 128 * 4096 - 127
    assert rc == RTO_E_INVALID and "2^31" in R.lib().rto_last_error().decode()
    assert out_cap.value == 128 + n and (st.reachable, st.candidates, st.selected, st.levels, st.cut_key) == (128, n, n, 3, 1)
    fits = (2 ** 31 - 1) // 4096 - 128
    assert refiner.plan(dc, None, 1, fits)[0] == 128 + fits  # (planned only: the result would hold 8 GB of child words)


def test_argument_refusals(refiner):
    import torch
    child, data, _, _, _, _, want = RR.case("sh4_depth3_mask")
    cap, D = child.shape[0], data.shape[-1]
    dc, dd = _dev(child), _dev(data)
    dk = torch.ones(child.size, dtype=torch.int32, device="cuda:0")
    k = want[0].shape[0]
    co = torch.full((k * 8,), 7, dtype=torch.int32, device="cuda:0")
    do = torch.zeros(k * 8 * D, dtype=torch.float16, device="cuda:0")
    ss = torch.zeros(k * 8, dtype=torch.int32, device="cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    oc = C.c_int64(0)
    L, h = R.lib(), refiner._h

    def refused(rc):
        msg = L.rto_last_error().decode()
        assert rc == RTO_E_INVALID and msg, (rc, msg)
        return msg

    plan = lambda *a: refused(L.rto_tree_refine_plan(*a))  # noqa: E731
    assert "child is not memory" in plan(h, None, C.c_void_p(child.ctypes.data), None, cap, 2, 1, -1, 31, C.byref(oc), None)
    host_key = np.ones(child.size, np.uint32)
    assert "key is not memory" in plan(h, None, P(dc), C.c_void_p(host_key.ctypes.data), cap, 2, 1, -1, 31, C.byref(oc), None)
    assert "null" in plan(None, None, P(dc), None, cap, 2, 1, -1, 31, C.byref(oc), None)
    assert "null" in plan(h, None, None, None, cap, 2, 1, -1, 31, C.byref(oc), None)
    assert "null" in plan(h, None, P(dc), None, cap, 2, 1, -1, 31, None, None)
    assert "cap" in plan(h, None, P(dc), None, 0, 2, 1, -1, 31, C.byref(oc), None)
    assert "2^31" in plan(h, None, P(dc), None, 1 << 28, 2, 1, -1, 31, C.byref(oc), None)
    assert "N must" in plan(h, None, P(dc), None, cap, 1, 1, -1, 31, C.byref(oc), None)
    assert "max_level" in plan(h, None, P(dc), None, cap, 2, 1, -1, 0, C.byref(oc), None)
    assert "max_level" in plan(h, None, P(dc), None, cap, 2, 1, -1, 32, C.byref(oc), None)
    assert "aligned" in plan(h, None, C.c_void_p(dc.data_ptr() + 2), None, cap - 1, 2, 1, -1, 31, C.byref(oc), None)
    assert "aligned" in plan(h, None, P(dc), C.c_void_p(dk.data_ptr() + 2), cap - 1, 2, 1, -1, 31, C.byref(oc), None)
    assert refiner.plan(dc, dk)[0] == k
    write = lambda *a: refused(L.rto_tree_refine_write(*a))  # noqa: E731
    assert "null" in write(h, None, P(dc), None, D, P(co), P(do), None)
    assert "null" in write(h, None, P(dc), P(dd), D, None, P(do), None)
    assert "null" in write(h, None, None, P(dd), D, P(co), P(do), None)
    assert "D must" in write(h, None, P(dc), P(dd), 0, P(co), P(do), None)
    assert "data is not memory" in write(h, None, P(dc), C.c_void_p(data.ctypes.data), D, P(co), P(do), None)
    host_out = np.zeros(k * 8 * D, np.float16)
    assert "data_out is not memory" in write(h, None, P(dc), P(dd), D, P(co), C.c_void_p(host_out.ctypes.data), None)
    host_src = np.zeros(k * 8, np.int32)
    assert "slot_src is not memory" in write(h, None, P(dc), P(dd), D, P(co), P(do), C.c_void_p(host_src.ctypes.data))
    assert "overlap" in write(h, None, P(dc), P(dd), D, P(dc), P(do), None)
    assert "overlap" in write(h, None, P(dc), P(dd), D, P(co), C.c_void_p(dd.data_ptr() + 64), None)
    assert "overlap" in write(h, None, P(dc), P(dd), D, P(co), P(do), C.c_void_p(co.data_ptr() + 64))
    assert "aligned" in write(h, None, P(dc), P(dd), D, C.c_void_p(co.data_ptr() + 2), P(do), None)
    torch.cuda.synchronize()
    assert (co == 7).all() and not ss.any()  # nothing was enqueued
    RR.assert_same(_run(refiner, child, data), want, "after the refusals")


# ---------------------------------------------------------------- downstream
def _unit_tree(child, data, fmt="SH4"):
    """in a world that IS tree space: points with exact binary coordinates stay exactly on cell faces"""
    return R.N3Tree.from_arrays(child, data, np.ones(3, np.float32), np.zeros(3, np.float32), fmt)


@pytest.mark.parametrize("name", ["sh4_depth6_mask", "sh4_depth6_density_budget", "shuffled_garbage_few"])
def test_queries_return_the_original_bits(refiner, name):
    child, data, key, thresh, max_new, max_level, _ = RR.case(name)
    got = _run(refiner, child, data, key, thresh, max_new, max_level)
    pts = SR.probe_points(got[3]["levels"] + 2).astype(np.float32)
    a, b = _unit_tree(child, data), _unit_tree(got[0], got[1])
    qa, qb = a.query(pts, values=True, sigma=True, level=True), b.query(pts, values=True, sigma=True, level=True)
    assert_bits_equal(qb["values"].cpu().numpy(), qa["values"].cpu().numpy(), "values")
    assert_bits_equal(qb["sigma"].cpu().numpy(), qa["sigma"].cpu().numpy(), "sigma")
    la, lb = qa["level"].cpu().numpy(), qb["level"].cpu().numpy()
    assert (lb >= la).all() and (lb <= la + 1).all() and (lb > la).any()
    a.free()
    b.free()


@pytest.mark.parametrize("name", ["sh4_depth6_mask", "sh4_depth6_few_budget1000", "shuffled_garbage_few", "n4_wide_budget"])
def test_the_simplifier_undoes_it_on_the_device(refiner, name):
    child, data, key, thresh, max_new, max_level, _ = RR.case(name)
    c, d, _, st = _run(refiner, child, data, key, thresh, max_new, max_level)
    assert st["selected"] > 0
    s = R.Simplifier(0)
    try:
        a = s.simplify(_dev(c), _dev(d))
        b = s.simplify(_dev(child), _dev(data))
        assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(a[2].cpu().numpy(), b[2].cpu().numpy())
        assert_bits_equal(a[1].cpu().numpy().view(np.uint16).astype(np.uint32), b[1].cpu().numpy().view(np.uint16).astype(np.uint32), "data")
        assert a[3]["merged"] == b[3]["merged"] + st["selected"] and a[3]["capacity"] == b[3]["capacity"]
    finally:
        s.free()


def test_refined_tree_renders_like_the_oracle_renders_it(refiner):
    t = synth.make_tree(depth_limit=6, basis_dim=9, seed=7)
    c, d, _, st = _run(refiner, t.child, t.data, RR.density_keys(t.data), 1, 3000)
    assert st["selected"] == 3000
    ht, dt = make_pair(synth.SynthTree(c, d, t.scale, t.offset, t.data_format, t.depth_limit + 1, {}))
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
        assert_bits_equal(aux, aux_o, "refined tree, frame %d" % f)
    dt.free()


def test_ten_sgd_steps_on_a_refined_tree_with_params_carried_through_slot_src(refiner):
    import torch
    from test_fit_gpu import LR10, _cams3
    t = synth.make_tree(5, 9, seed=7)
    cams = _cams3()
    targets = R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, threads=8).render(cams)
    params = t.data.astype(np.float32)
    params[..., :-1] *= np.float32(0.5)
    params[..., -1] *= np.float32(0.8)
    params += np.float32(2.0 ** -14)  # no longer fp16 values
    c, d, src, st = _run(refiner, t.child, t.data, RR.density_keys(t.data), 1, 2000)
    assert st["selected"] == 2000
    D = t.data.shape[-1]
    carried = params.reshape(-1, D)[src.reshape(-1)].reshape(d.shape)
    hf = R.HostTreeFit(c, d, t.scale, t.offset, t.data_format, threads=8)
    df = R.TreeFit(R.N3Tree.from_arrays(c, d, t.scale, t.offset, t.data_format), d)
    hf.params[...] = carried
    df.params.copy_(torch.from_numpy(params).cuda().reshape(-1, D)[torch.from_numpy(src.reshape(-1).astype(np.int64)).cuda()].reshape(d.shape))
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), carried.view(np.uint32))
    tg_dev = [torch.from_numpy(x).cuda() for x in targets]
    words_h, words_d = [], []
    for _ in range(10):
        hf.accumulate(cams, targets)
        df.accumulate(cams, tg_dev)
        words_h.append(int(hf.stats[0]))
        words_d.append(int(df.stats.cpu()[0]))
        assert hf.loss() == df.loss()
        hf.step(LR10)
        df.step(LR10)
    assert words_d == words_h and words_d[-1] < words_d[0], (words_d, words_h)
    assert np.array_equal(df.params.cpu().numpy().view(np.uint32), hf.params.view(np.uint32))
    # the split leaves' children have moved apart: the support has grown
    new = hf.params.reshape(-1, 8, D)[t.child.shape[0]:]
    assert (new != new[:, :1]).any()
    df.tree.free()


def test_refine_octree_backends_write_the_same_bytes(tmp_path, capsys):
    src = str(tmp_path / "tree.npz")
    z = _write_tree(src, depth_limit=6, basis_dim=9)
    w = (np.random.default_rng(8).random(z["child"].shape) ** 4).astype(np.float32)
    np.save(str(tmp_path / "w.npy"), w)
    for extra in ([], ["--max_nodes", "4000", "--sigma_thresh", "2.0"], ["--weights", str(tmp_path / "w.npy"), "--weight_thresh", "0.2"]):
        outs = {}
        for backend in ("cpu", "hip"):
            assert refine_octree.main([src, "--backend", backend, "--out_dir", str(tmp_path / backend), "--overwrite"] + extra) == 0
            outs[backend] = (tmp_path / backend / "tree.npz").read_bytes()
        assert outs["cpu"] == outs["hip"], extra
    capsys.readouterr()
    with np.load(str(tmp_path / "hip" / "tree.npz")) as f:
        assert f["child"].shape[0] > z["child"].shape[0]
    tree = R.N3Tree(str(tmp_path / "hip" / "tree.npz"))  # the file loads
    assert tree.capacity > z["child"].shape[0]
    tree.free()


def test_optimize_octree_with_a_refine_round_backends_write_the_same_bytes(tmp_path, capsys):
    tree = synth.make_tree(4, 4, seed=7)
    js, pert, z = fit_scene(tmp_path, tree)
    outs = {}
    for backend in ("hip", "cpu"):
        assert optimize_octree.main([pert, "--poses", js, "--backend", backend, "--out_dir", str(tmp_path / backend), "--refine_rounds", "1",
                                     "--refine_nodes", "150"] + TOOL_ARGS) == 0
        outs[backend] = (tmp_path / backend / "pert.npz").read_bytes()
    text = capsys.readouterr().out
    assert outs["hip"] == outs["cpu"], "the optimised files differ"
    assert text.count("150 selected") == 2
    with np.load(str(tmp_path / "hip" / "pert.npz")) as f:
        assert f["child"].shape[0] == z["child"].shape[0] + 150
