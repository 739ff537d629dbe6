"""The host twin of the tree refiner (rto_tree_refine_host, csrc/host/tree_refine.cpp) against the numpy model of
tests/refine_ref.py, bit for bit (include/rto.h "refiner" leaves nothing to an implementation: there is no tolerance), the
properties the operation promises (the field at every point, simplify undoes it, data_out == data[slot_src]), the edge cases of
the selection, every refusal, and the refine_octree and optimize_octree --refine_rounds commands on the host.  No GPU is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import refine_ref as RR
import simplify_ref as SR
import rt_octree_amd as R
from rt_octree_amd import optimize_octree, refine, refine_octree, synth
from rt_octree_amd._lib import CRefineStats, check, lib

from test_simplify_host import _write_tree, renumbering_inputs

RTO_E_INVALID, RTO_E_FORMAT = -1, -6
W, H = 23, 19  # the fit tests' image size


def _host(child, data, key=None, key_thresh=1, max_new=-1, max_level=31):
    return refine.refine_tree(child, data, key, key_thresh, max_new, max_level, backend="cpu")


@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_host_twin_equals_the_model(name):
    child, data, key, thresh, max_new, max_level, want = RR.case(name)
    RR.assert_same(_host(child, data, key, thresh, max_new, max_level), want, name)


def test_what_the_cases_cover():
    st = lambda name: RR.case(name)[6][3]  # noqa: E731
    assert {RR.tree(n)[1].shape[-1] for n in RR.TREES} >= {4, 5, 13, 28} and RR.tree("n4")[0].shape[1] == 4
    assert (RR.tree("sh4_depth5_shuffled_lossless")[0] < 0).any()
    assert st("garbage_mask")["reachable"] == st("garbage_mask")["capacity_in"] - 8
    assert st("one_node_mask")["capacity"] == 9 and st("one_node_none")["capacity"] == 1 and st("one_node_none")["cut_key"] == 0
    # the budget cuts inside a class of equal keys, and the cut differs from the largest key elsewhere
    few = RR.case("sh4_depth6_few_budget1000")
    assert few[6][3]["cut_key"] == 0xFFFFFFFF and (few[2].reshape(-1)[RR.candidates_of(few[0], few[2])[0]] == 0xFFFFFFFF).sum() > 1000
    assert st("sh4_depth6_low_byte")["cut_key"] >> 8 == 0x3E99A5 and st("sh4_depth6_high_byte")["cut_key"] & 0xFFFFFF == 0xC0FFEE
    assert st("key_thresh_zero_takes_zero_keys")["cut_key"] == 0


def test_the_chain_of_31_levels_and_max_level():
    """the leaves of the node at level 31 are no candidates; max_level = l excludes exactly the leaves of nodes of level >= l"""
    child, data = RR.tree("chain31")
    level = RR.levels_of(child)
    assert level.max() == 31
    leaves_of = lambda lo, hi: int(((child.reshape(32, 8) == 0) & (level[:, None] >= lo) & (level[:, None] < hi)).sum())  # noqa: E731
    got = _host(child, data)
    assert got[3]["candidates"] == leaves_of(0, 31) == 31 * 7 and got[3]["levels"] == 32
    assert (got[2].reshape(-1)[32 * 8:] // 8 < 31).all()  # no slot of node 31 was split
    for l in (1, 2, 7, 30, 31):
        g = _host(child, data, max_level=l)
        assert g[3]["candidates"] == leaves_of(0, l) and g[3]["selected"] == g[3]["candidates"], l
        RR.assert_same(g, RR.refine(child, data, None, 1, -1, l), "max_level %d" % l)


TREES_OF_THE_INVARIANTS = [("sh4", 5), ("sh4", 6), ("rgba", 7)]  # 1015, 4087 and 18885 nodes


def _keyed(child, data, kind):
    """(key, key_thresh, max_new) of the three key kinds of the invariants"""
    if kind == "mask":
        return None, 1, -1
    if kind == "density_budget":
        key = RR.density_keys(data)
        return key, 1, int((key != 0).sum() // 3)
    return RR.random_keys(child.shape, 17, "few"), 1, 1000


@pytest.mark.parametrize("kind", ["mask", "density_budget", "four_values_budget_1000"])
@pytest.mark.parametrize("which", TREES_OF_THE_INVARIANTS, ids=lambda w: "%s_depth%d" % w)
def test_invariants(which, kind):
    """the field is unchanged at every point, simplify(refine(T)) == simplify(T), data_out == data[slot_src]"""
    child, data = SR._arrays(SR.synth_tree(which[1], 4 if which[0] == "sh4" else 1))
    assert child.shape[0] == {5: 1015, 6: 4087, 7: 18885}[which[1]]
    key, thresh, max_new = _keyed(child, data, kind)
    c, d, src, st = _host(child, data, key, thresh, max_new)
    assert st["selected"] > 100 and st["capacity"] == child.shape[0] + st["selected"]
    D = data.shape[-1]
    assert np.array_equal(d.reshape(-1, D).view(np.uint16), data.reshape(-1, D).view(np.uint16)[src.reshape(-1)])
    pts = SR.probe_points(st["levels"] + 2)
    before, lvl_before = SR.descend(child, data, pts)
    after, lvl_after = SR.descend(c, d, pts)
    assert np.array_equal(after, before)
    assert (lvl_after >= lvl_before).all() and (lvl_after <= lvl_before + 1).all() and (lvl_after > lvl_before).any()
    a, b = SR.simplify(c, d), SR.simplify(child, data)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16)) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- the selection
def test_every_budget_around_the_candidate_count():
    child, data = RR.tree("sh4_depth3_lossless")
    key = RR.random_keys(child.shape, 21, "wide")
    C = RR.candidates_of(child, key)[0].size
    for max_new in (0, 1, C - 1, C, C + 1, -1, -(2 ** 40), 2 ** 40):
        got = _host(child, data, key, 1, max_new)
        RR.assert_same(got, RR.refine(child, data, key, 1, max_new), "max_new %d" % max_new)
        assert got[3]["selected"] == (C if max_new < 0 else min(C, max_new))
    zero = _host(child, data, key, 1, 0)
    assert np.array_equal(zero[0], child) and np.array_equal(zero[1].view(np.uint16), data.view(np.uint16)) and zero[3]["cut_key"] == 0
    assert np.array_equal(zero[2].reshape(-1), np.arange(child.size))


def test_equal_keys_go_by_slot_index_and_a_null_key_is_all_ones():
    child, data = RR.tree("sh4_depth5_shuffled_lossless")
    cand = RR.candidates_of(child)[0]
    for K in (1, 5, 1000, cand.size - 1):
        for key in (None, np.full(child.shape, 1, np.uint32), np.full(child.shape, 0xDEADBEEF, np.uint32)):
            c, d, src, st = _host(child, data, key, 1, K)
            S = 8
            assert np.array_equal(src.reshape(-1, S)[child.shape[0]:, 0], cand[:K]), (K, None if key is None else hex(int(key.flat[0])))
            assert st["cut_key"] == (1 if key is None else int(key.flat[0]))
    RR.assert_same(_host(child, data, None, 1, 1000), _host(child, data, np.ones(child.shape, np.uint32), 1, 1000), "NULL key")


@pytest.mark.parametrize("kind", ["few", "low", "high", "wide"])
def test_budgets_on_and_around_a_class_of_equal_keys(kind):
    """a budget that lands exactly on count(key > cut) (nothing of the next class is taken), one more, and one that takes every
    equal key"""
    child, data = RR.tree("rgba_depth5_lossless")
    key = RR.random_keys(child.shape, 31, kind)
    cand, ck = RR.candidates_of(child, key)
    values = np.unique(ck)[::-1]
    v = values[min(2, len(values) - 1)]
    above, equal = int((ck > v).sum()), int((ck == v).sum())
    for K in (above, above + 1, above + equal - 1, above + equal, above + equal + 1):
        got = _host(child, data, key, 1, K)
        RR.assert_same(got, RR.refine(child, data, key, 1, K), "%s K = %d" % (kind, K))
        taken = got[2].reshape(-1, 8)[child.shape[0]:, 0]
        assert np.array_equal(np.sort(taken), taken)  # ascending slot order
        if 0 < K <= above + equal:
            assert got[3]["cut_key"] == (int(ck[ck > v].min()) if K == above else int(v))


def test_a_threshold_above_every_key_copies_the_tree():
    child, data = RR.tree("n4")
    key = RR.random_keys(child.shape, 3, "low")
    got = _host(child, data, key, int(key.max()) + 1)
    assert got[3]["candidates"] == 0 and got[3]["selected"] == 0 and got[3]["cut_key"] == 0 and got[3]["levels"] == 3
    assert np.array_equal(got[0], child) and np.array_equal(got[1].view(np.uint16), data.view(np.uint16))
    at = _host(child, data, key, int(key.max()))
    assert at[3]["selected"] == at[3]["candidates"] >= 1 and at[3]["cut_key"] == int(key.max())


def test_key_builders():
    w = np.array([0.0, 1e-9, 0.01, 0.5, 1.0, 1.5, -0.25, np.nan, -0.0], np.float32)
    k = R.keys_from_weights(w)
    assert k.dtype == np.uint32
    assert np.array_equal(k, np.array([0.0, 1e-9, 0.01, 0.5, 1.0, 1.0, 0.0, 0.0, 0.0], np.float32).view(np.uint32))
    assert (np.diff(k[:5].astype(np.int64)) > 0).all()  # the bits order as the values do
    child, data = SR.special_densities()
    for th in (0.0, 2.0):
        k = R.keys_from_density(data, th)
        assert k.dtype == np.uint32 and k.shape == child.shape and np.array_equal(k, RR.density_keys(data, th))
        sigma = data[..., -1].astype(np.float32)
        assert (k[np.isnan(sigma)] == 0).all() and (k[sigma <= th] == 0).all() and (k[sigma > th] != 0).all()
    assert refine_octree.weight_thresh_key(0.0) == 1 and refine_octree.weight_thresh_key(0.01) == int(np.float32(0.01).view(np.uint32))


# ---------------------------------------------------------------- refusals
def _call(child, data, cap, N, D, key=None, key_thresh=1, max_new=-1, max_level=31, child_out=0, data_out=0, room=None, out_cap=0,
          slot_src=None, stats=None):
    """the raw entry; 0 for an output = a fresh buffer of `room` nodes (default: twice a sane cap + 8)"""
    keep = []

    def ptr(a):
        if a is None:
            return None
        if isinstance(a, int):
            return C.c_void_p(a)
        keep.append(a)
        return C.c_void_p(a.ctypes.data)
    sane = max(min(cap, 1 << 12), 1) * min(max(N, 1), 4) ** 3
    if room is None:
        room = 9 * max(min(cap, 1 << 12), 1)
    if isinstance(child_out, int) and child_out == 0:
        child_out = np.zeros(9 * sane, np.int32)
    if isinstance(data_out, int) and data_out == 0:
        data_out = np.zeros(9 * sane * max(D, 1), np.uint16)
    oc = C.c_int64(-7) if out_cap == 0 else out_cap
    rc = lib().rto_tree_refine_host(ptr(child), ptr(data), ptr(key), cap, N, D, key_thresh, max_new, max_level, ptr(child_out),
                                    ptr(data_out), room, C.byref(oc) if oc is not None else None, ptr(slot_src), stats)
    return rc, lib().rto_last_error().decode(), (oc.value if oc is not None else None)


@pytest.mark.parametrize("kind", SR.MALFORMED)
def test_refuses_malformed_links(kind):
    child, data = SR.malformed(kind)
    rc, msg, _ = _call(child, data, child.shape[0], 2, data.shape[-1])
    assert rc == RTO_E_FORMAT and msg, (rc, msg)
    with pytest.raises(RR.FormatError):
        RR.refine(child, data)
    with pytest.raises(R.RtoError) as e:
        _host(child, data)
    assert e.value.code == RTO_E_FORMAT


def test_refuses_a_walk_of_more_than_32_levels():
    child, data = SR.too_deep()
    rc, msg, _ = _call(child, data, child.shape[0], 2, 4)
    assert rc == RTO_E_FORMAT and "32 levels" in msg
    with pytest.raises(RR.FormatError):
        RR.refine(child, data)


def test_the_simplifiers_renumbering_inputs_and_their_mutations():
    """the shuffled tree and the one with garbage appended refine like the model; with one offset after another broken the twin
    answers RTO_E_FORMAT exactly where the model does, RTO_OK with the model's bytes elsewhere"""
    (sc, sd), (gc, gd) = renumbering_inputs()
    for c, d in ((sc, sd), (gc, gd)):
        RR.assert_same(_host(c, d, None, 1, 999), RR.refine(c, d, None, 1, 999), "renumbering input")
    rng = np.random.default_rng(77)
    refused = 0
    for trial in range(40):
        c = gc.copy()
        flat = c.reshape(-1)
        for _ in range(int(rng.integers(1, 4))):
            flat[rng.integers(0, flat.size)] = int(rng.choice([0, 1, -1, 7, -9, c.shape[0], 2 ** 31 - 1, -2 ** 31, int(rng.integers(-500, 500))]))
        try:
            want = RR.refine(c, gd, None, 1, 300)
        except RR.FormatError:
            want = None
        if want is None:
            refused += 1
            with pytest.raises(R.RtoError) as e:
                _host(c, gd, None, 1, 300)
            assert e.value.code == RTO_E_FORMAT, trial
        else:
            RR.assert_same(_host(c, gd, None, 1, 300), want, "mutation %d" % trial)
    assert 5 < refused < 40


def test_refuses_arguments():
    child, data = SR._arrays(SR.synth_tree(3, 1))
    cap = child.shape[0]
    key = np.ones(child.shape, np.uint32)
    ok = lambda **kw: _call(child, data, cap, 2, 4, **kw)  # noqa: E731
    assert ok()[0] == 0 and ok(key=key)[0] == 0
    for kw in (dict(child_out=None), dict(data_out=None), dict(out_cap=None)):
        rc, msg, _ = ok(**kw)
        assert rc == RTO_E_INVALID and "null" in msg, kw
    for args in ((None, data), (child, None)):
        rc, msg, _ = _call(args[0], args[1], cap, 2, 4)
        assert rc == RTO_E_INVALID and "null" in msg
    for c, n, d, word in ((0, 2, 4, "cap"), (-5, 2, 4, "cap"), (cap, 1, 4, "N"), (cap, 0, 4, "N"), (cap, 2, 0, "D"), (cap, 2, -1, "D"),
                          (1 << 28, 2, 4, "2^31"), (1 << 25, 4, 4, "2^31"), (cap, 2000, 4, "2^31")):
        rc, msg, _ = _call(child, data, c, n, d)
        assert rc == RTO_E_INVALID and word in msg, (c, n, d, msg)
    for ml in (0, -1, 32, 100):
        rc, msg, _ = ok(max_level=ml)
        assert rc == RTO_E_INVALID and "max_level" in msg, ml
    assert ok(max_level=1)[0] == 0 and ok(max_level=31)[0] == 0
    # an output inside an input, an input inside an output, two outputs on one buffer, misaligned pointers
    rc, msg, _ = ok(child_out=child)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg, _ = ok(data_out=data.ctypes.data + 2 * 4 * 8)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg, _ = ok(key=key, child_out=key.ctypes.data + 4 * 8)
    assert rc == RTO_E_INVALID and "overlap" in msg
    big = np.zeros(9 * cap * 8 * (4 + 2 * 4 + 4), np.uint8)
    rc, msg, _ = ok(data_out=big, child_out=big.ctypes.data + 64)
    assert rc == RTO_E_INVALID and "overlap" in msg
    rc, msg, _ = ok(data_out=big, slot_src=big.ctypes.data + 8)
    assert rc == RTO_E_INVALID and "overlap" in msg
    for kw in (dict(child_out=big.ctypes.data + 2), dict(data_out=big.ctypes.data + 1), dict(slot_src=big.ctypes.data + 2),
               dict(key=key.ctypes.data + 1)):
        rc, msg, _ = ok(**kw)
        assert rc == RTO_E_INVALID and "aligned" in msg, kw
    rc, msg, _ = _call(child.ctypes.data + 2, data, cap - 1, 2, 4)
    assert rc == RTO_E_INVALID and "aligned" in msg
    # counting only; a room that is too small reports capacity and stats all the same
    st = CRefineStats()
    rc, _, k = ok(child_out=None, data_out=None, room=0, stats=C.byref(st))
    want = RR.refine(child, data)[3]
    assert rc == 0 and k == want["capacity"] and st.selected == want["selected"] and st.reachable == cap
    st = CRefineStats()
    rc, msg, k = ok(room=want["capacity"] - 1, stats=C.byref(st))
    assert rc == RTO_E_INVALID and "room" in msg and k == want["capacity"] and st.selected == want["selected"] and st.levels == want["levels"]
    assert ok(room=want["capacity"])[0] == 0
    with pytest.raises(R.RtoError):
        refine.refine_tree(child.astype(np.int64), data, backend="cpu")
    with pytest.raises(R.RtoError):
        refine.refine_tree(child, data[:, :, :, :1], backend="cpu")
    with pytest.raises(R.RtoError):
        refine.refine_tree(child, data, key.reshape(-1)[:-1], backend="cpu")
    with pytest.raises(ValueError):
        refine.refine_tree(child, data, backend="cuda")


def too_large_tree():
    """N = 16: 128 nodes (a root with 127 child nodes) hold 524288 slots; with every leaf split cap_out * 4096 >= 2^31"""
    child = np.zeros((128, 4096), np.int32)
    child[0, :127] = np.arange(1, 128)
    return child.reshape(128, 16, 16, 16), np.zeros((128, 16, 16, 16, 1), np.float16)


def test_a_result_that_is_too_large_is_refused_with_capacity_and_stats():
    child, data = too_large_tree()
    st = CRefineStats()
    rc, msg, k = _call(child, data, 128, 16, 1, child_out=None, data_out=None, room=0, stats=C.byref(st))
    C_ = 128 * 4096 - 127
    assert rc == RTO_E_INVALID and "2^31" in msg and k == 128 + C_ and (k * 4096 >= 2 ** 31)
    assert (st.reachable, st.candidates, st.selected, st.levels, st.cut_key) == (128, C_, C_, 3, 1)
    with pytest.raises(RR.TooLarge) as e:
        RR.refine(child, data)
    assert e.value.stats["capacity"] == k
    # the largest budget that fits is taken
    fits = (2 ** 31 - 1) // 4096 - 128
    rc, msg, k = _call(child, data, 128, 16, 1, max_new=fits, child_out=None, data_out=None, room=0)
    assert rc == 0 and k == 128 + fits
    rc, msg, k = _call(child, data, 128, 16, 1, max_new=fits + 1, child_out=None, data_out=None, room=0)
    assert rc == RTO_E_INVALID and k == 128 + fits + 1


# ---------------------------------------------------------------- the commands
def test_refine_octree_command_on_the_host(tmp_path, capsys):
    src = str(tmp_path / "tree.npz")
    z = _write_tree(src)
    out = tmp_path / "out"
    assert refine_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--max_nodes", "500"]) == 0
    text = capsys.readouterr().out
    want = RR.refine(z["child"], z["data"], RR.density_keys(z["data"]), 1, 500)
    assert "Nodes %d -> %d (%d candidates, 500 selected), %d levels" % (z["child"].shape[0], want[0].shape[0], want[3]["candidates"],
                                                                        want[3]["levels"]) in text and "MB" in text
    with np.load(str(out / "tree.npz")) as f:
        assert sorted(f.files) == sorted(k for k in z if k not in ("parent_depth", "n_free", "n_internal"))
        assert np.array_equal(f["child"], want[0]) and np.array_equal(f["data"].view(np.uint16), want[1].view(np.uint16))
        for k in ("data_dim", "data_format", "invradius3", "offset", "geom_resize_fact", "depth_limit", "extra_data"):
            assert f[k].dtype == z[k].dtype and np.array_equal(f[k], z[k]), k
    assert refine_octree.main([src, "--backend", "cpu", "--out_dir", str(out)]) == 0
    assert " > skip" in capsys.readouterr().out
    # weights: heaviest first above the threshold, --sigma_thresh zeroes keys, --max_level bounds the depth
    rng = np.random.default_rng(8)
    w = (rng.random(z["child"].shape) ** 4).astype(np.float32)
    np.save(str(tmp_path / "w.npy"), w)
    assert refine_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--overwrite", "--weights", str(tmp_path / "w.npy"),
                               "--weight_thresh", "0.25", "--sigma_thresh", "2.0", "--max_level", "5", "--max_nodes", "300"]) == 0
    capsys.readouterr()
    key = np.where(RR.density_keys(z["data"], 2.0) != 0, w.view(np.uint32), np.uint32(0))
    want = RR.refine(z["child"], z["data"], key, int(np.float32(0.25).view(np.uint32)), 300, 5)
    assert 0 < want[3]["selected"] <= 300 and want[3]["levels"] <= 6
    with np.load(str(out / "tree.npz")) as f:
        assert np.array_equal(f["child"], want[0]) and np.array_equal(f["data"].view(np.uint16), want[1].view(np.uint16))
    np.save(str(tmp_path / "short.npy"), w[:-1])
    assert refine_octree.main([src, "--backend", "cpu", "--out_dir", str(out), "--overwrite", "--weights", str(tmp_path / "short.npy")]) == 2
    assert "weights" in capsys.readouterr().err


def test_refine_octree_refuses_a_quantised_file(tmp_path, capsys):
    from rt_octree_amd import compress_octree
    src = str(tmp_path / "tree.npz")
    _write_tree(src, depth_limit=3)
    assert compress_octree.main([src, "--backend", "cpu", "--out_dir", str(tmp_path / "q")]) == 0
    capsys.readouterr()
    assert refine_octree.main([str(tmp_path / "q" / "tree.npz"), "--backend", "cpu", "--out_dir", str(tmp_path / "s")]) == 2
    err = capsys.readouterr().err
    assert "quantised" in err and "compress_octree" in err
    assert not (tmp_path / "s" / "tree.npz").exists()


def fit_scene(tmp_path, tree):
    """the fit tests' small scene as files: three 23 x 19 training images of `tree` and a perturbed tree file -> (pose file, tree
    file, the dict of the tree file)"""
    from helpers import rcam
    cams = [rcam(W, H, p) for p in synth.orbit_poses(4)[:3]]
    images = R.HostTreeFit(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, threads=8).render(cams)
    os.makedirs(tmp_path / "test")
    js = synth.write_transforms_json(str(tmp_path / "transforms_train.json"), synth.orbit_poses(4)[:3])
    for i, im in enumerate(images):
        u8 = np.concatenate([np.clip(np.rint(im * 255), 0, 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
        u8 = np.ascontiguousarray(u8)
        check(lib().rto_image_write_png(str(tmp_path / "test" / ("r_%d.png" % i)).encode(), u8.ctypes.data, W, H))
    src = tree.save_npz(str(tmp_path / "tree.npz"))
    with np.load(src) as f:
        z = {k: f[k] for k in f.files}
    d = tree.data.astype(np.float32)
    d[..., :-1] *= 0.5
    z["data"] = d.astype(np.float16)
    pert = str(tmp_path / "pert.npz")
    np.savez_compressed(pert, **z)
    return js, pert, z


TOOL_ARGS = ["--epochs", "2", "--batch_imgs", "2", "--lr", "4000"]


def test_optimize_octree_with_one_refine_round_on_the_host(tmp_path, capsys):
    tree = synth.make_tree(4, 4, seed=7)
    js, pert, z = fit_scene(tmp_path, tree)
    assert optimize_octree.main([pert, "--poses", js, "--backend", "cpu", "--out_dir", str(tmp_path / "out"), "--refine_rounds", "1",
                                 "--refine_nodes", "150"] + TOOL_ARGS) == 0
    text = capsys.readouterr().out
    # the pieces by hand, in the tool's order
    options = R.RenderOptions(step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2, background_brightness=1.0)
    cams, targets = optimize_octree.load_views("blender", js, 1.0, 0, 1.0)
    fit, to_dev = optimize_octree.make_fit(z, options, "cpu")
    first = []
    optimize_octree.optimize(fit, to_dev, cams, targets, 4000.0, 2, 2, say=lambda s: None, losses=first)
    halves = fit.data_half()
    w = R.leaf_weights_host(z["child"], halves, fit.scale, fit.offset, cams, options, threads=4)
    c, d, src, st = refine.refine_tree_host(z["child"], halves, R.keys_from_weights(w), refine_octree.weight_thresh_key(0.01), 150)
    assert st["selected"] == 150 and st["candidates"] > 150
    fit2 = R.HostTreeFit(c, d, fit.scale, fit.offset, fit.data_format, options, threads=4)
    fit2.params[...] = fit.params.reshape(-1, halves.shape[-1])[src.reshape(-1)].reshape(fit2.params.shape)
    assert (fit2.params.astype(np.float16).astype(np.float32) != fit2.params).any()  # the state did not pass through fp16
    second = []
    optimize_octree.optimize(fit2, to_dev, cams, targets, 4000.0, 2, 2, say=lambda s: None, losses=second)
    lines = [l.strip() for l in text.splitlines()]
    assert "> round 0: nodes %d -> %d (%d candidates, 150 selected), %d levels" % (z["child"].shape[0], z["child"].shape[0] + 150,
                                                                                   st["candidates"], st["levels"]) in lines
    psnr = [l for l in lines if l.startswith("> epoch")]
    assert len(psnr) == 4 and psnr == ["> epoch %d: train psnr %.4f" % (e, optimize_octree.psnr_of(*x)) for e, x in
                                       ((0, first[0]), (1, first[1]), (0, second[0]), (1, second[1]))]
    # the loss word itself, through the function the tool runs
    got = []
    f0, td = optimize_octree.make_fit(z, options, "cpu")
    optimize_octree.optimize_rounds(z, f0, td, cams, targets, options, "cpu", 4000.0, 2, 2, 1, 150, say=lambda s: None, losses=got)
    assert got == first + second and len({x[0] for x in got}) == 4
    with np.load(str(tmp_path / "out" / "pert.npz")) as f:
        assert np.array_equal(f["child"], c) and f["child"].shape[0] == z["child"].shape[0] + 150
        assert np.array_equal(f["data"].view(np.uint16), fit2.data_half().view(np.uint16))
        assert sorted(f.files) == sorted(k for k in z if k not in ("parent_depth", "n_free", "n_internal"))


def test_optimize_octree_without_refine_rounds_writes_todays_bytes(tmp_path, capsys):
    tree = synth.make_tree(4, 4, seed=7)
    js, pert, z = fit_scene(tmp_path, tree)
    assert optimize_octree.main([pert, "--poses", js, "--backend", "cpu", "--out_dir", str(tmp_path / "a"), "--refine_rounds", "0"]
                                + TOOL_ARGS) == 0
    assert optimize_octree.main([pert, "--poses", js, "--backend", "cpu", "--out_dir", str(tmp_path / "b")] + TOOL_ARGS) == 0
    capsys.readouterr()
    # the unmodified code path: make_fit, optimize(), data_half, savez_compressed
    options = R.RenderOptions(step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2, background_brightness=1.0)
    cams, targets = optimize_octree.load_views("blender", js, 1.0, 0, 1.0)
    fit, to_dev = optimize_octree.make_fit(z, options, "cpu")
    optimize_octree.optimize(fit, to_dev, cams, targets, 4000.0, 2, 2, say=lambda s: None)
    zz = dict(z)
    zz["data"] = fit.data_half()
    np.savez_compressed(str(tmp_path / "by_hand.npz"), **zz)
    want = (tmp_path / "by_hand.npz").read_bytes()
    assert (tmp_path / "a" / "pert.npz").read_bytes() == want and (tmp_path / "b" / "pert.npz").read_bytes() == want
    assert optimize_octree.main([pert, "--poses", js, "--backend", "cpu", "--out_dir", str(tmp_path / "c"), "--refine_rounds", "-1"]) == 2
    assert "refine_rounds" in capsys.readouterr().err
