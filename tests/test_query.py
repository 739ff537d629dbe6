"""rto_tree_query / N3Tree.query: what the tree holds at a point, bit for bit against the oracle's orc_query (the reference's
query_single_from_root, n3tree_query.hpp:13-48) on the host arrays that were uploaded -- whichever image the kernel walks and
whichever form the coefficients are resident in.  orc_query's `levels` counts the nodes it visits, the root included: the
convention of rto_tree_info.max_depth, so it is compared as it is."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rt_octree_amd as R
from rt_octree_amd import _lib, synth

E_INVALID, E_UNSUPPORTED = -1, -3
f32 = np.float32


# ------------------------------------------------------------------ no device needed
def test_query_symbol_is_declared_and_exported():
    assert "rto_tree_query" in _lib.SYMBOLS
    L = R.lib()
    assert L.rto_tree_query.restype is C.c_int and len(L.rto_tree_query.argtypes) == 5


def test_query_argument_checks_run_before_any_device_use():
    L = R.lib()
    out = _lib.CQueryOut()
    fake = C.create_string_buffer(64)  # never dereferenced: every check below returns first
    tree = C.cast(fake, C.c_void_p)
    pts = C.cast(fake, C.c_void_p)

    def refused(rc):
        assert rc == E_INVALID and L.rto_last_error().decode().startswith("rto_tree_query:")

    refused(L.rto_tree_query(None, pts, 1, C.byref(out), None))
    refused(L.rto_tree_query(tree, pts, 1, None, None))
    refused(L.rto_tree_query(tree, pts, -1, C.byref(out), None))
    refused(L.rto_tree_query(tree, None, 1, C.byref(out), None))
    out.cube = 8
    refused(L.rto_tree_query(tree, pts, 1, C.byref(out), None))


def test_numpy_widens_halves_like_the_oracle():
    """the expected `values` below are numpy's float16 -> float32; the oracle's orc_half2float gives the same floats"""
    import orc
    h = np.arange(65536, dtype=np.uint16)
    ours = h.view(np.float16).astype(f32).view(np.uint32)
    theirs = np.array([orc.lib().orc_half2float(int(v)) for v in h], f32).view(np.uint32)
    nan = np.isnan(h.view(np.float16))
    assert np.array_equal(ours[~nan], theirs[~nan]) and np.isnan(theirs.view(f32)[nan]).all()


# ------------------------------------------------------------------ the oracle's answer
def _expected(tree, pts):
    """orc_query at xyz = offset + scale * p (float32, two roundings) -> values [n, dd], sigma, level, cube [n, 4]; a point
    with a non-finite coordinate: level -1, zeros"""
    import orc
    ht = orc.HostTree(tree.child, tree.data, tree.scale, tree.offset, tree.data_format)
    q = orc.lib().orc_query
    dd = ht.data_dim
    data = ht.data.reshape(-1, dd)
    pts = np.asarray(pts, f32)
    n = pts.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        xyz = (ht.offset[None, :] + ht.scale[None, :] * pts).astype(f32)
    hi = f32(1.0) - f32(1e-6)  # VOLREND_MIN / VOLREND_MAX as the reference writes them: a < b ? a : b, a > b ? a : b
    with np.errstate(invalid="ignore"):
        clamped = np.where(xyz < hi, xyz, hi)
        clamped = np.where(clamped > 0, clamped, f32(0.0)).astype(f32)
    values = np.zeros((n, dd), f32)
    level = np.full(n, -1, np.int32)
    cube = np.zeros((n, 4), f32)
    buf, cs, lv = (C.c_float * 3)(), C.c_float(), C.c_int()
    tc = C.byref(ht.c)
    for i in np.flatnonzero(np.isfinite(pts).all(1)):
        buf[0], buf[1], buf[2] = xyz[i]
        slot = q(tc, buf, C.byref(cs), C.byref(lv))
        values[i] = data[slot].view(np.float16).astype(f32)
        level[i] = lv.value
        local = np.array(buf[:], f32)
        cube[i, :3] = clamped[i] - local / f32(cs.value)
        cube[i, 3] = f32(1.0) / f32(cs.value)
    return {"values": values, "sigma": values[:, -1].copy(), "level": level, "cube": cube}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(dt, tree, pts, what, values=True):
    import torch
    exp = _expected(tree, pts)
    got = dt.query(torch.from_numpy(np.ascontiguousarray(pts, f32)).cuda(), values=values, sigma=True, level=True, cube=True)
    torch.cuda.synchronize()
    for k, v in got.items():
        g = v.cpu().numpy()
        assert g.shape == exp[k].shape, (what, k, g.shape)
        if len(pts) == 0:
            continue
        bad = np.flatnonzero((_bits(g) != _bits(exp[k])).reshape(len(pts), -1).any(1))
        assert bad.size == 0, "%s: %s differs at %d of %d points; first %d = %r: %r vs %r" % (
            what, k, bad.size, len(pts), bad[0], pts[bad[0]], g[bad[0]], exp[k][bad[0]])
    return got


def _world(tree, xyz):
    """world points whose float32 image offset + scale * p is exactly the tree coordinate xyz, where one exists (searched among
    the neighbours of the float64 solution); rows without one are dropped"""
    xyz = np.asarray(xyz, f32)
    p = ((xyz.astype(np.float64) - tree.offset) / tree.scale).astype(f32)
    best = p.copy()
    ok = np.zeros(xyz.shape, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for step in range(-3, 4):
            cand = p.copy()
            for _ in range(abs(step)):
                cand = np.nextafter(cand, f32(np.inf if step > 0 else -np.inf))
            hit = ((tree.offset + tree.scale * cand).astype(f32) == xyz) & ~ok
            best[hit] = cand[hit]
            ok |= hit
    return best[ok.all(1)]


def _hard_points(tree, depth):
    """every cell boundary k / 2^d down to `depth` with the floats on either side, zeros, subnormals, the clamp's edge, points
    outside the volume, non-finite coordinates -- as world points of `tree`"""
    rng = np.random.default_rng(5)
    t = [np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.1754944e-38, 1.0, 2.0, -1.0, 0.5, 1e30, -1e30], f32)]
    edge = f32(1.0) - f32(1e-6)
    t.append(np.array([edge, np.nextafter(edge, f32(0)), np.nextafter(edge, f32(2)), np.nextafter(f32(1), f32(0))], f32))
    for d in range(1, depth + 1):
        k = np.arange(0, 2 ** d + 1) if d <= 6 else rng.integers(0, 2 ** d + 1, 96)
        b = (k / 2.0 ** d).astype(f32)
        t += [b, np.nextafter(b, f32(-1)), np.nextafter(b, f32(2))]
    t = np.unique(np.concatenate(t).view(np.uint32)).view(f32)
    # each special coordinate on each axis against random partners, and all three axes special at once
    other = rng.uniform(0, 1, (t.size, 3)).astype(f32)
    rows = [np.stack([t, t[::-1], np.roll(t, 7)], 1)]
    for ax in range(3):
        r = other.copy()
        r[:, ax] = t
        rows.append(r)
    tree_pts = np.concatenate(rows).astype(f32)
    world = _world(tree, tree_pts)
    # the raw values as WORLD coordinates too (subnormal and huge inputs to the mapping itself)
    world = np.concatenate([world, np.stack([t, t[::-1], np.roll(t, 3)], 1)])
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for ax in range(3):
            r = rng.uniform(-1, 1, 3).astype(f32)
            r[ax] = v
            bad.append(r)
    return np.concatenate([world, np.array(bad, f32)]).astype(f32)


def _box_points(tree, n, seed=1):
    """uniform in a box 10 % larger than the tree's"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.05, 1.05, (n, 3))
    return ((u - tree.offset) / tree.scale).astype(f32)


@functools.lru_cache(maxsize=None)
def _sh(basis, depth=5, seed=7):
    return synth.make_tree(depth_limit=depth, basis_dim=basis, seed=seed)


def _upload(tree, **kw):
    return R.N3Tree.from_arrays(tree.child, tree.data, tree.scale, tree.offset, tree.data_format, extra_data=tree.extra, **kw)


def _n4_tree():
    """a small N = 4 tree: the root, two of its 64 cells refined, one of those refined once more"""
    rng = np.random.default_rng(2)
    child = np.zeros((4, 4, 4, 4), np.int32)
    child[0, 1, 2, 3] = 1
    child[0, 3, 0, 1] = 2
    child[2, 0, 3, 2] = 1
    data = rng.normal(0, 1, (4, 4, 4, 4, 28)).astype(np.float16)
    data[..., -1] = np.abs(data[..., -1]) * (rng.uniform(0, 1, (4, 4, 4, 4)) < 0.5)
    return synth.SynthTree(child, data, (0.4, 0.3, 0.5), (0.5, 0.45, 0.55), "SH9", 3, {})


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_default_tree_every_size_hard_points_and_a_large_batch():
    """dense SH9, the default upload: child[] / data[] released, entry-ordered records, the two-level image"""
    import torch
    tree = _sh(9, depth=6)
    dt = _upload(tree)
    assert dt.wide_nodes > 0
    bytes_before = dt.device_bytes
    big = _box_points(tree, 100000)
    got = _check(dt, tree, big, "100000 points")
    dt._refresh()
    assert dt.device_bytes == bytes_before, "a values query brought child[] / data[] back"
    assert (got["level"].cpu().numpy() > 0).all() and int(got["level"].max()) == dt.max_depth
    _check(dt, tree, _hard_points(tree, dt.max_depth), "hard points")
    for n in (0, 1, 63, 64, 65, 257):
        r = _check(dt, tree, big[:n], "n = %d" % n)
        assert r["values"].shape == (n, 28) and r["cube"].shape == (n, 4) and r["level"].dtype == torch.int32
    # splitting one call into two gives the same bytes
    p = torch.from_numpy(big[:1000]).cuda()
    whole = dt.query(p, sigma=True, level=True, cube=True)
    a, b = dt.query(p[:333].contiguous(), sigma=True, level=True, cube=True), dt.query(p[333:].contiguous(), sigma=True, level=True, cube=True)
    for k in whole:
        assert torch.equal(whole[k].view(torch.int32), torch.cat([a[k], b[k]]).view(torch.int32)), k
    # sigma alone (the occupancy path), and the checks of _ray_tensor
    s = dt.query(p, values=False, sigma=True)
    assert list(s) == ["sigma"] and torch.equal(s["sigma"].view(torch.int32), whole["sigma"].view(torch.int32))
    with pytest.raises(R.RtoError):
        dt.query(p.double())
    with pytest.raises(R.RtoError):
        dt.query(p[:, :2])
    with pytest.raises(R.RtoError):
        dt.query(p.cpu())


def _variants():
    sh9 = _sh(9)
    from helpers import FRAME_ANISO, reframe, rgba_tree
    return {
        "sh16": (lambda: _sh(16), {}),
        "sh25": (lambda: _sh(25, depth=4), {}),
        "rgba": (lambda: rgba_tree(sh9), {}),
        "sg9_lobes": (lambda: synth.with_lobes(sh9, "SG", seed=2), {}),
        "compact": (lambda: sh9, {"compact": True}),
        "keep_reference": (lambda: sh9, {"keep_reference": True}),
        "no_culling": (lambda: sh9, {"no_culling": True}),
        "compact_records_keep_reference": (lambda: sh9, {"compact_records": True, "keep_reference": True}),
        "reframed": (lambda: reframe(sh9, *FRAME_ANISO), {}),
        "shuffled": (lambda: synth.shuffle_nodes(reframe(sh9, *FRAME_ANISO), seed=3), {}),
        # levels below the top grid (which covers min(max_depth - 1, 6) levels): one at depths 4 .. 7, two at depth 8
        "depth_4": (lambda: _sh(9, depth=4), {}),
        "depth_7_odd_below_grid": (lambda: _sh(4, depth=7), {}),
        "depth_8_even_below_grid": (lambda: _sh(4, depth=8), {}),
        "n4": (_n4_tree, {}),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sh16", "sh25", "rgba", "sg9_lobes", "compact", "keep_reference", "no_culling",
                                  "compact_records_keep_reference", "reframed", "shuffled", "depth_4",
                                  "depth_7_odd_below_grid", "depth_8_even_below_grid", "n4"])
def test_storage_forms_and_tree_shapes(name):
    make, kw = _variants()[name]
    tree = make()
    dt = _upload(tree, **kw)
    if name == "n4":
        assert dt.N == 4 and dt.wide_nodes == 0
    pts = np.concatenate([_box_points(tree, 3000, seed=4), _hard_points(tree, min(dt.max_depth + 1, 9))])
    _check(dt, tree, pts, name)


@pytest.mark.gpu
def test_the_two_images_and_the_shuffled_file_give_the_same_answers():
    """an upload with RTO_NO_WIDE=1 walks the one-level image (slot-ordered records); a tree whose nodes are shuffled in the
    file answers like the ordered one"""
    import torch
    tree = _sh(9)
    pts = np.concatenate([_box_points(tree, 3000, seed=6), _hard_points(tree, 6)])
    wide = _upload(tree)
    os.environ["RTO_NO_WIDE"] = "1"
    try:
        narrow = _upload(tree)
    finally:
        del os.environ["RTO_NO_WIDE"]
    assert wide.wide_nodes > 0 and narrow.wide_nodes == 0
    a = _check(narrow, tree, pts, "one-level image")
    b = _check(wide, tree, pts, "two-level image")
    c = _check(_upload(synth.shuffle_nodes(tree, seed=9)), tree, pts, "shuffled nodes")
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) and torch.equal(a[k].view(torch.int32), c[k].view(torch.int32))


@pytest.mark.gpu
def test_trees_that_cannot_reproduce_their_values(tmp_path):
    """RTO_TREE_COMPACT_RECORDS keeps the coefficients of leaves with sigma > 0 only (the upload releases data[], and
    ensure_reference_arrays rebuilds the others as zeros); a quantised-direct tree keeps codebooks.  `values` is refused for
    both, sigma / level / cube answer as for the expanded tree."""
    import torch
    tree = _sh(9)
    pts = np.concatenate([_box_points(tree, 2000, seed=8), _hard_points(tree, 6)])
    p = torch.from_numpy(pts).cuda()
    cr = _upload(tree, compact_records=True)
    with pytest.raises(R.RtoError) as e:
        cr.query(p)
    assert e.value.code == E_UNSUPPORTED and "RTO_TREE_KEEP_REFERENCE" in e.value.msg
    _check(cr, tree, pts, "compact records", values=False)
    path = str(tmp_path / "quant.npz")
    tree.save_quant_npz(path, n_retain=1, quantiser="luminance")
    qd, ex = R.N3Tree(path, quant_direct=True), R.N3Tree(path)
    with pytest.raises(R.RtoError) as e:
        qd.query(p)
    assert e.value.code == E_UNSUPPORTED
    a, b = qd.query(p, values=False, sigma=True, level=True, cube=True), ex.query(p, values=False, sigma=True, level=True, cube=True)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert (a["level"].cpu().numpy()[np.isfinite(pts).all(1)] > 0).all()


@pytest.mark.gpu
def test_a_query_between_two_renders_changes_nothing():
    import torch
    from helpers import cameras
    tree = _sh(9)
    dt = _upload(tree)
    _, cam = cameras(64, 48, synth.orbit_poses(4)[1])
    ctx = R.RenderContext(64, 48)
    opt = R.RenderOptions(spp=6, denoise=False)
    R.launch_renderer(dt, cam, opt, ctx)
    aux0, img0, rng0 = ctx.download_aux(), ctx.download_image(), ctx.rng_get()
    dt.query(torch.from_numpy(_box_points(tree, 5000)).cuda(), sigma=True, level=True, cube=True)
    assert ctx.rng_get() == rng0
    R.launch_renderer(dt, cam, opt, ctx)
    assert np.array_equal(_bits(ctx.download_aux()), _bits(aux0)) and np.array_equal(_bits(ctx.download_image()), _bits(img0))
