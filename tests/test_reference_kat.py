"""The oracle and the HIP kernels against the REFERENCE's own ray core, executed on the host.

tests/golden/ref_rt_core.npz holds what `internal::query_single_from_root`, `internal::maybe_precalc_basis`,
`device::sample_dst<SPP>` and `device::trace_ray<float, SPP>` of rt_core.cuh / n3tree_query.hpp / lumisphere.hpp return when
they are compiled as they lie behind stand-in CUDA headers (oracle/ref_kat/rt_core_kat.cpp, authoring machine only) -- with
`__logf` / `__expf` / the lobes' `expf` meaning this project's det_logf / det_expf -- for hand-sized trees (SH4 / 9 / 16 / 25,
RGBA, SG9, ASG4, one anisotropic off-centre frame, one whose densities sit on both sides of the threshold) and these rays:
hits and misses; origins inside the box and inside a dense leaf; rays in a face, along an edge, through corners shared by
several leaves; direction components 0, -0, +-1e-9f (where `dir + 1e-9` cancels), +-1e-10f; a depth limit inside a leaf, in
an empty gap, below tmin, and the default 1e9; a non-default step size, a cropped box, a basis mask, a raised density
threshold (one leaf's density equal to it); leaves thick enough to take several samples at SPP 16 / 32.

Everything is compared on bit patterns.  The file is self-contained (tree arrays, inputs, outputs); nothing here reads the
reference or oracle/_ref -- except the one test that, where oracle/_ref/rt_core_kat exists, reruns it and requires the
committed outputs."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import rt_octree_amd as R
import sg_asg_ref
from rt_octree_amd import _lib
from test_rays import ray_oracle, ray_setup

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
KAT_EXE = os.path.join(ROOT, "oracle", "_ref", "rt_core_kat")
f32 = np.float32

TREES = ("sh9", "sh16", "sh25", "sh4", "rgba", "sg9", "asg4", "aniso", "thresh")
CASES = TREES + ("sh9.step", "sh16.crop", "sh9.mask", "thresh.raised")
SPPS = (1, 2, 3, 4, 6, 8, 16, 32)
KERNELS = (R.KERNEL_AUTO, R.KERNEL_GENERIC, R.KERNEL_FAST)


@functools.lru_cache(maxsize=None)
def _z():
    with np.load(os.path.join(GOLDEN, "ref_rt_core.npz")) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def _tree(name):
    z = _z()
    t = {k: z["tree.%s.%s" % (name, k)] for k in ("child", "data", "scale", "offset", "fmt")}
    t["data_format"] = str(z["tree.%s.data_format" % name])
    t["extra"] = z.get("tree.%s.extra" % name)
    return t


def _case(name):
    z = _z()
    pre = "case.%s." % name
    c = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
    c["tree"] = str(c["tree"])
    return c


@functools.lru_cache(maxsize=None)
def _host(name):
    t = _tree(name)
    return orc.HostTree(t["child"], t["data"], t["scale"], t["offset"], t["data_format"], extra=t["extra"])


def _optkw(case):
    optf, opti = case["optf"], case["opti"]
    return dict(step_size=float(optf[0]), sigma_thresh=float(optf[1]), render_bbox=[float(v) for v in optf[2:8]],
                basis_minmax=[int(opti[0]), int(opti[1])])


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8, 2: np.uint16}[got.dtype.itemsize]
    bad = np.flatnonzero((got.view(u) != want.view(u)).reshape(got.shape[0], -1).any(1))
    assert bad.size == 0, "%s: %d of %d rows differ; first %d: %r vs the reference's %r" % (
        what, bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(autouse=True)
def _det_math():
    orc.lib().orc_set_math_mode(orc.MATH_DET)
    yield


# ------------------------------------------------------------------ the fixture holds what the issue asks for


def test_fixture_covers_the_classes():
    z = _z()
    assert tuple(z["spps"]) == SPPS
    assert os.path.getsize(os.path.join(GOLDEN, "ref_rt_core.npz")) <= 733186
    lo, hi = np.array([0x211e, 0x211f], np.uint16).view(np.float16)
    sig = _tree("thresh")["data"][..., -1]
    assert f32(lo) < f32(1e-2) < f32(hi) and (sig == lo).any() and (sig == hi).any() and (sig == np.float16(0.5)).any()
    assert len(set(_tree("aniso")["scale"].tolist())) == 3 and len(set(_tree("aniso")["offset"].tolist())) == 3
    through = 0
    for name in TREES:
        c = _case(name)
        t = _tree(name)
        assert 100 <= c["tmax"].size <= 400 and t["child"].shape[0] <= 300
        d = c["ray_dir"].reshape(-1, 3)
        out32 = c["trace32_out"].reshape(-1, 4)
        assert (out32[:, 3] > 0).sum() > 50 and (c["trace32_draws"] == 0).sum() > 10  # hits, and rays that miss the box
        through += int(((out32[:, 3] == 0) & (c["trace32_draws"] == 32)).sum())  # in the box, nothing hit
        cen = c["ray_cen"].reshape(-1, 3)
        assert (((cen > 0) & (cen < 1)).all(1)).sum() >= 20  # origins inside the box
        zero = (d == 0)
        assert (zero & ~np.signbit(d)).any() and (zero & np.signbit(d)).any()  # 0 and -0
        assert (c["tmax"] == f32(1e9)).any() and (c["tmax"] < 100).sum() >= 20
        # several samples in one leaf: alpha 1 at SPP 32 from a ray whose SPP-1 twin hit too
        assert (out32[:, 3] == 1).any()
    assert through >= 5
    iso = _case("sh9")["ray_dir"].reshape(-1, 3)  # (scale 0.5: the tiny components reach `dir + 1e-9` unchanged)
    for v in (f32(1e-9), -f32(1e-9), f32(1e-10), -f32(1e-10)):
        assert (iso == v).any(), v
    q = _case("sh9")["q_xyz"].reshape(-1, 3)
    for v in (f32(0), f32(0.5), f32(0.25), f32(1) - f32(1e-6), f32(1)):
        assert (q == v).any(), v
    assert (q < 0).any() and (q > 1).any()  # clamped
    dyadic = (q * 64 == np.floor(q * 64)) & (q > 0) & (q < 1)  # on a cell boundary k / 2^d
    assert (dyadic.sum(1) == 1).any() and (dyadic.sum(1) == 2).any() and (dyadic.sum(1) == 3).any()  # face, edge, corner


# ------------------------------------------------------------------ CPU: the oracle against the reference


@pytest.mark.parametrize("name", TREES)
def test_query_matches_the_reference(name):
    c, ht, t = _case(name), _host(name), _tree(name)
    pts = c["qpts"]
    with np.errstate(over="ignore"):
        xyz = (ht.offset[None, :] + ht.scale[None, :] * pts).astype(f32)
    _same(xyz, c["q_xyz"].reshape(-1, 3), "%s: offset + scale * p" % name)
    q = orc.lib().orc_query
    n = pts.shape[0]
    leaf, cube, local = np.zeros(n, np.int64), np.zeros(n, f32), np.zeros((n, 3), f32)
    buf, cs, lv = (C.c_float * 3)(), C.c_float(), C.c_int()
    for i in range(n):
        buf[0], buf[1], buf[2] = xyz[i]
        leaf[i] = q(C.byref(ht.c), buf, C.byref(cs), C.byref(lv))
        cube[i] = cs.value
        local[i] = buf[:]
    _same(leaf, c["q_leaf"], "%s: leaf slot" % name)
    _same(cube, c["q_cube_sz"], "%s: cube_sz" % name)
    _same(local, c["q_local"].reshape(-1, 3), "%s: leaf-local xyz" % name)
    sigma = t["data"].reshape(-1, t["data"].shape[-1])[leaf, -1].astype(f32)
    _same(sigma, c["q_sigma"], "%s: sigma" % name)
    assert len(set(cube.tolist())) >= 4  # (several depths)


@pytest.mark.parametrize("name", [n for n in TREES if n != "rgba"])
def test_basis_matches_the_reference(name):
    c, t = _case(name), _tree(name)
    dirs = c["bdirs"]
    want = c["basis"].reshape(-1, 25)
    kind, B = int(t["fmt"][0]), int(t["fmt"][1])
    got = np.zeros((dirs.shape[0], 25), f32)
    if kind == orc.FMT_SH:
        fn = orc.lib().orc_sh_basis
        buf = (C.c_float * 25)()
        for i, d in enumerate(dirs):
            fn(B, (C.c_float * 3)(*[float(v) for v in d]), buf)
            got[i, :B] = buf[:B]
        _same(got, want, "%s: orc_sh_basis" % name)
    else:
        fn = orc.lib().orc_lobe_basis
        fn.restype = None
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lobes = np.ascontiguousarray(t["extra"], f32)
        for i, d in enumerate(dirs):
            fn(kind, B, lobes.ctypes.data, np.ascontiguousarray(d).ctypes.data, got[i].ctypes.data)
        _same(got, want, "%s: orc_lobe_basis" % name)
        _same(sg_asg_ref.basis({2: "SG", 3: "ASG"}[kind], lobes, dirs), want, "%s: sg_asg_ref" % name)
        assert (want[:, :B] == 0).any() and (np.abs(want[:, :B]) > 1e-3).any()  # underflow and ordinary values
    assert not want[:, B:].any()


def test_rgba_tree_has_no_basis():
    assert not _case("rgba")["basis"].any()


@pytest.mark.parametrize("spp", SPPS)
def test_sample_dst_matches_the_reference(spp):
    z = _z()
    want = z["dst.dst%d" % spp].reshape(-1, spp + 1)
    want_state = z["dst.dst%d_state" % spp]
    L = orc.lib()
    got, state = np.zeros_like(want), np.zeros_like(want_state)
    for i in range(want.shape[0]):
        r = orc.rng(seed=int(z["rng_seed"][0]))
        L.orc_pcg32_advance(C.byref(r), i * spp)
        L.orc_sample_dst(spp, C.byref(r), got[i].ctypes.data_as(C.c_void_p))
        state[i] = r.state
    _same(got, want, "sample_dst<%d>" % spp)
    _same(state, want_state, "RNG state after sample_dst<%d>" % spp)
    assert want.shape[0] >= 32 and (want[:, -1] == np.finfo(f32).max).all()


@pytest.mark.parametrize("name", CASES)
def test_ray_setup_matches_the_reference(name):
    c = _case(name)
    d, cen, vdir = ray_setup(_host(c["tree"]), c["origins"], c["dirs"])
    _same(d, c["ray_dir"].reshape(-1, 3), "%s: normalised direction" % name)
    _same(cen, c["ray_cen"].reshape(-1, 3), "%s: offset + scale * origin" % name)
    _same(vdir, d, "%s: vdir" % name)


@functools.lru_cache(maxsize=None)
def _oracle_trace(name, spp):
    c = _case(name)
    draws = np.full(c["tmax"].size, 255, np.uint8)
    out = ray_oracle(_host(c["tree"]), c["origins"], c["dirs"], spp, t_max=c["tmax"], bg=0.0, draws=draws, **_optkw(c))
    out.setflags(write=False)
    return out, draws


def _is_rgba(case):
    return int(_tree(case["tree"])["fmt"][1]) < 0


def _same_trace(got, case, spp, what):
    """out[4] against the trace table.  RGBA trees: alpha at every SPP, the colour at SPP 1 only -- above that the library
    deviates on purpose, see test_rgba_colour_deviation_from_the_reference"""
    want = case["trace%d_out" % spp].reshape(-1, 4)
    if _is_rgba(case) and spp > 1:
        got, want = got[:, 3:], want[:, 3:]
    _same(got, want, what)


@pytest.mark.parametrize("name", CASES)
def test_trace_ray_matches_the_reference(name):
    c = _case(name)
    for spp in SPPS:
        out, draws = _oracle_trace(name, spp)
        _same_trace(out, c, spp, "%s: orc_trace_ray, SPP %d" % (name, spp))
        _same(draws, c["trace%d_draws" % spp], "%s: RNG draws consumed, SPP %d" % (name, spp))


def test_rgba_colour_deviation_from_the_reference():
    """A deliberate deviation.  rt_core.cuh:320 shades every hit entry of an RGBA tree from `tree_val`,
    which in that branch is the function's variable of :225 -- the leaf the march queried LAST (:247) -- because the
    declaration `const half* tree_val = tree_vals[i]` (:289) lives inside the SH branch only.  The library shades entry i from
    its own leaf tree_vals[i], as the SH branch does and as the rendering equation asks (tests/expected_render.py pins it).
    The two agree where the last queried leaf is the only hit leaf: always at SPP 1 (the march breaks on its first hit).
    Pinned here: alpha and the draws agree with the reference for every ray and SPP, the colour at SPP 1; above SPP 1 the
    colours differ on some rays (the march went on past the hit leaf, or hit several), and there the reference's colour
    is ONE data[] row times alpha."""
    c, t = _case("rgba"), _tree("rgba")
    rows = t["data"].reshape(-1, 4)[:, :3].astype(f32)
    differing = 0
    for spp in SPPS:
        out, _ = _oracle_trace("rgba", spp)
        ref = c["trace%d_out" % spp].reshape(-1, 4)
        _same(out[:, 3], ref[:, 3], "alpha, SPP %d" % spp)
        diff = (out[:, :3].view(np.uint32) != ref[:, :3].view(np.uint32)).any(1)
        if spp == 1:
            assert not diff.any()
            continue
        differing += int(diff.sum())
        # the reference's colour: (sum_i colour * cnt_i) / SPP with ONE colour -- some leaf's row reproduces it to rounding
        for i in np.flatnonzero(diff):
            err = np.abs(rows * ref[i, 3] - ref[i, :3]).max(1).min()
            assert err <= 1e-5 * max(1.0, np.abs(ref[i, :3]).max()), (spp, i, err)
    assert differing > 50


def test_option_cases_differ_from_the_defaults():
    """(each option set changes what the reference returns for its rays)"""
    for name in ("sh9.step", "sh16.crop", "sh9.mask", "thresh.raised"):
        c = _case(name)
        plain = ray_oracle(_host(c["tree"]), c["origins"], c["dirs"], 6, t_max=c["tmax"], bg=0.0)
        assert (plain.view(np.uint32) != c["trace6_out"].reshape(-1, 4).view(np.uint32)).any(1).sum() >= 5, name


def _probe_npz(path):
    buf = C.create_string_buffer(4096)
    _lib.check(R.lib().rto_tree_probe_npz(os.fsencode(path), buf, 4096))
    return json.loads(buf.value.decode())


@pytest.mark.parametrize("stem", ["npz_dense", "npz_quant"])
def test_host_loader_matches_the_reference_n3tree(stem):
    """src/n3tree.cpp's N3Tree(path), quantised decode included, against the host loader"""
    ref = json.loads(str(_z()["n3tree." + stem]))
    info = _probe_npz(os.path.join(GOLDEN, stem + ".npz"))
    assert info["child_fnv1a64"] == ref["child_fnv1a64"] and info["data_fnv1a64"] == ref["data_fnv1a64"]
    assert info["data_format"] == ref["data_format"] and info["data_dim"] == ref["data_dim"]
    assert info["capacity"] == ref["capacity"] and info["N"] == ref["N"]
    assert ref["data_shape"] == [ref["capacity"], 2, 2, 2, ref["data_dim"]] and ref["data_word_size"] == 2
    assert np.array(info["scale"], f32).view(np.uint32).tolist() == ref["scale_bits"]
    assert np.array(info["offset"], f32).view(np.uint32).tolist() == ref["offset_bits"]


@pytest.mark.skipif(not os.path.exists(KAT_EXE), reason="oracle/_ref/rt_core_kat is built on the authoring machine only")
def test_recipe_reproduces_the_fixture(tmp_path):
    """the committed outputs are what oracle/ref_kat produces from the committed inputs"""
    sys.path.insert(0, GOLDEN)
    try:
        import make_goldens as mg
    finally:
        sys.path.remove(GOLDEN)
    z = _z()
    compared = 0
    for ci, name in enumerate(CASES):
        c = _case(name)
        t = _tree(c["tree"])
        cpath, opath = str(tmp_path / "case.npz"), str(tmp_path / "out.bin")
        mg.write_kat_case(cpath, t, c)
        subprocess.check_call([KAT_EXE, cpath, opath])
        res = mg.kat_states_to_draws(mg.read_kat_tables(opath))
        for k, v in res.items():
            if v.size == 0:
                continue
            want = z["dst." + k] if k.startswith("dst") else c[k]
            _same(v, want, "%s: %s" % (name, k))
            compared += 1
    assert compared > 200
    for stem in ("npz_dense", "npz_quant"):
        jpath = str(tmp_path / (stem + ".json"))
        subprocess.check_call([KAT_EXE, "--n3tree", os.path.join(GOLDEN, stem + ".npz"), jpath], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        assert json.load(open(jpath)) == json.loads(str(z["n3tree." + stem]))


# ------------------------------------------------------------------ GPU: the kernels against the reference


@functools.lru_cache(maxsize=None)
def _dev(name):
    t = _tree(name)
    return R.N3Tree.from_arrays(t["child"], t["data"], t["scale"], t["offset"], t["data_format"], extra_data=t["extra"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_render_rays_matches_the_reference(name):
    import torch
    c = _case(name)
    dt = _dev(c["tree"])
    dev = torch.device("cuda", 0)
    o, d, tm = (torch.as_tensor(np.ascontiguousarray(c[k]), device=dev) for k in ("origins", "dirs", "tmax"))
    ctx = R.RenderContext(8, 8)
    ctx.rng_seed(int(_z()["rng_seed"][0]))
    for kernel in KERNELS:
        ctx.set_kernel(kernel)
        for spp in SPPS:
            opt = R.RenderOptions(spp=spp, background_brightness=0.0, **_optkw(c))
            got = R.render_rays(dt, o, d, opt, ctx, t_max=tm, first_ray=0).cpu().numpy()
            _same_trace(got, c, spp, "%s: render_rays, kernel %d, SPP %d" % (name, kernel, spp))


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
def test_tree_query_matches_the_reference(name):
    import torch
    c, t = _case(name), _tree(name)
    got = _dev(name).query(torch.as_tensor(np.ascontiguousarray(c["qpts"]), device="cuda:0"), values=False, sigma=True, level=True,
                           cube=True)
    torch.cuda.synchronize()
    _same(got["sigma"].cpu().numpy(), c["q_sigma"], "%s: sigma" % name)
    cube_sz = c["q_cube_sz"]
    xyz = c["q_xyz"].reshape(-1, 3)
    hi = f32(1.0) - f32(1e-6)
    clamped = np.where(xyz < hi, xyz, hi)
    clamped = np.where(clamped > 0, clamped, f32(0.0)).astype(f32)
    want = np.concatenate([clamped - c["q_local"].reshape(-1, 3) / cube_sz[:, None], (f32(1.0) / cube_sz)[:, None]], 1).astype(f32)
    _same(got["cube"].cpu().numpy(), want, "%s: leaf corner and side" % name)
    _same(got["level"].cpu().numpy(), np.log2(cube_sz).astype(np.int32), "%s: level" % name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in TREES if n != "rgba"])
def test_probe_basis_matches_the_reference(name):
    c = _case(name)
    dirs = np.ascontiguousarray(c["bdirs"], f32)
    co = R.RenderOptions().to_c()
    for path in (0, 1):
        out = np.empty((dirs.shape[0], 25), f32)
        _lib.check(R.lib().rto_probe_basis(_dev(name)._h, C.byref(co), C.c_void_p(dirs.ctypes.data), dirs.shape[0], path,
                                           C.c_void_p(out.ctypes.data)))
        want = c["basis"].reshape(-1, 25)
        B = int(_tree(name)["fmt"][1])  # (the reference leaves the entries from basis_dim on unwritten)
        _same(out[:, :B], want[:, :B], "%s: rto_probe_basis path %d" % (name, path))
        if path == 1:
            _same(out, want, "%s: rto_probe_basis path 1, all 25" % name)
