"""The denoise kernels at BATCH launch shape and under arbitrary tile marks.

guidance_fused / guidance_general and filter_fast walk a strip of tiles along x whose length follows from the launch size
(rto_denoise_launch_strips): 5 / 13 tiles for a batch like the benchmark's, 1 for the small launches of the other tests.  The
prefetch of the next live tile, the per-strip bit budgets (position ts of a tile in its strip), the skip chains and the partial
last strip only exist at strip > 1.  Here: 902 x 61 frames (29 tile columns, a partial last strip at every length: 5 x 5 + 4 and 13 + 13 + 3; no
multiple of 8 either way), batches of 86 / 80 / 60 / 44 / 17 frames = filter strips 5 / 4 / 3 / 2 / 1, network strips 13 / 9 / 7 / 5 / 1, built from K base frames (frame f = base f mod
K, so a wrong blockIdx.z shows) and, for the culled and sparse routes, from mark patterns no render produces (denoise_synth.py).

  a  the batch == the same base frames sent one at a time (strip 1, what the rest of the suite pins), bit for bit
  b  the batch's exact filter == the host oracle bit for bit; the factorised / packed routes and the planes within the bounds
     of test_filter_parity / test_guidance_fused
  c  every culled entry under the synthetic marks == the unculled kernels, bit for bit, outputs prefilled with -7
  d  every tile the host predicate calls skippable IS skipped (a poisoned input inside it changes nothing), and the poison does
     reach the plain kernels: over-skipping fails c, under-skipping fails d
  e  the sparse route (NaN in every unmarked tile, dirty packed scratch) == the full route, bit for bit
The CPU tests prove, through the query and the predicates, that the batches reach the strips, positions and patterns claimed."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_synth as ds
import rt_octree_amd as R
from rt_octree_amd import _lib

torch = pytest.importorskip("torch")
from rt_octree_amd import denoiser  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
DEV = "cuda:0"

H, W, K = 61, 902, 4
LONG = 86
BATCHES = {86: (5, 13), 80: (4, 9), 60: (3, 7), 44: (2, 5), 17: (1, 1)}  # n -> (filter strip, network strip) at 902 x 61
NETS = {"c32_l4_n2": (32, 4, 2), "c16_l3_n2": (16, 3, 2), "c32_l4_n3": (32, 4, 3)}  # the reference shape, test_guidance_shapes' general nets


# ---------------------------------------------------------------- not gpu

def test_query_is_declared_exported_and_equals_the_rule():
    hdr = open(os.path.join(ROOT, "include", "rto.h")).read()
    assert "int rto_denoise_launch_strips(" in hdr and "rto_denoise_launch_strips" in _lib.SYMBOLS
    getattr(C.CDLL(R.LIB_PATH), "rto_denoise_launch_strips")
    # the launch shapes of the suite and of the benchmark
    for (w, h, n), want in {(400, 304, 5): (1, 1), (333, 257, 5): (1, 1), (520, 420, 4): (1, 1), (200, 152, 3): (1, 1),
                            (800, 800, 4): (2, 4), (800, 800, 5): (3, 6), (1920, 1080, 2): (3, 8), (800, 800, 100): (5, 13),
                            (430, 56, 171): (5, 13), (430, 24, 344): (5, 13), (430, 24, 300): (4, 6), (430, 24, 230): (3, 6),
                            (430, 24, 160): (2, 3)}.items():
        assert ds.launch_strips(n, h, w) == want == ds.strips_by_rule(n, h, w), (w, h, n)
    rs = np.random.RandomState(1)
    seen = set()
    for _ in range(400):
        n, h, w = int(rs.randint(1, 400)), int(rs.randint(1, 1200)), int(rs.randint(1, 2000))
        got = ds.launch_strips(n, h, w)
        assert got == ds.strips_by_rule(n, h, w), (n, h, w)
        seen.add(got)
    assert {s[0] for s in seen} == set(range(1, 6)) and len({s[1] for s in seen}) >= 10
    for n, want in BATCHES.items():
        assert ds.launch_strips(n, H, W) == want, n


def test_query_refuses_bad_arguments_without_a_device():
    lib = R.lib()
    a, b = C.c_int(7), C.c_int(7)
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8), (1, -1, 8), (1, 8, -1)):
        assert lib.rto_denoise_launch_strips(n, h, w, C.byref(a), C.byref(b)) == -1
    assert lib.rto_denoise_launch_strips(1, 8, 8, None, C.byref(b)) == -1
    assert lib.rto_denoise_launch_strips(1, 8, 8, C.byref(a), None) == -1
    assert (a.value, b.value) == (7, 7)
    assert b"rto_denoise_launch_strips" in lib.rto_last_error()


def test_frames_keep_the_marks_promise():
    rs = np.random.RandomState(3)
    rty, rtx = ds.mark_dims(H, W)
    assert (rty, rtx) == (8, 113) and H % 8 and W % 8
    marks = rs.random_sample((rty, rtx)) < 0.3
    marks[-1, -1] = marks[0, 0] = True  # (the ragged corner tile: 6 x 5 pixels)
    for bg in (0.0, 0.25, 1.0):
        noisy, aux = ds.frame_from_marks(marks, H, W, bg, rs)
        assert noisy.shape == (H, W, 4) and aux.shape == (8, H, W) and noisy.dtype == aux.dtype == np.float32
        px = np.repeat(np.repeat(marks, 8, 0), 8, 1)[:H, :W]
        assert np.all(noisy[~px] == np.array([bg, bg, bg, 0], np.float32))
        held = (noisy[..., 3] > 0).reshape(-1)
        assert not held[~px.reshape(-1)].any()
        tiles_held = np.zeros((rty, rtx), bool)
        ys, xs = np.nonzero(noisy[..., 3] > 0)
        tiles_held[ys >> 3, xs >> 3] = True
        assert not (tiles_held & ~marks).any()
        blank = marks & ~tiles_held  # a mark only says "may": some marked tiles hold nothing but background
        assert 0 < blank.sum() < marks.sum() // 2
        inside = noisy[px & np.repeat(np.repeat(tiles_held, 8, 0), 8, 1)[:H, :W]]
        assert np.all((inside[:, 3] > 0) & (inside[:, 3] <= 1)) and np.all((inside[:, :3] >= 0) & (inside[:, :3] < 1))
        assert np.array_equal(aux[:4], noisy.transpose(2, 0, 1)) and np.array_equal(aux[4:], aux[:4] * aux[:4])
    # packing: bit t = tile t row-major, bit 0 of the last word = keep-all
    tiles = np.stack([marks, np.zeros_like(marks), np.ones_like(marks)])
    words = ds.pack_marks(tiles, [False, True, False], H, W)
    assert words.shape == (3, (rty * rtx + 31) // 32 + 1) and words.dtype == np.uint32
    for (r, c) in ((0, 0), (3, 57), (7, 112)):
        t = r * rtx + c
        assert ((int(words[0, t >> 5]) >> (t & 31)) & 1) == int(marks[r, c])
    assert words[0, -1] == 0 and words[1, -1] == 1 and not words[1, :-1].any() and words[2, -1] == 0
    back, keep = ds.unpack_marks(words, H, W)
    assert np.array_equal(back, tiles) and keep.tolist() == [False, True, False]
    assert ds.net_tiles_skipped_and_computed(words[1:2], H, W, 2) == (0, 8 * 29)  # kept whole: nothing skipped


def _batches_of(n, levels=4):
    """the mark batches the GPU tests launch at n frames: [(tiles, keep_all, names)], every pattern in one of them"""
    fs, ns = ds.launch_strips(n, H, W)
    patterns = ds.mark_patterns(H, W, fs, ns, levels)
    return patterns, [ds.batch_marks(patterns, n, first) for first in range(0, len(patterns) if n < len(patterns) else 1, n)]


def _check_coverage(n, want):
    fs, ns = ds.launch_strips(n, H, W)
    assert (fs, ns) == want, "the batch of %d frames no longer launches strips of %r but %r" % (n, want, (fs, ns))
    assert ds.filter_strip_in_kernel(W, fs) == fs  # (filter_fast derives its strip from the grid: the same number here)
    tiles_x = ds.ceil_div(W, 32)
    if fs > 1:
        assert tiles_x % fs and tiles_x % ns and tiles_x > 2 * ns, "no partial last strip behind two full ones"
    patterns, batches = _batches_of(n)
    names = [nm for b in batches for nm in b[2]]
    assert set(names) == {p[0] for p in patterns}, "a pattern is missing from the batch"
    families = [nm.split("_")[0] for nm, _t, _k in patterns]
    assert families.count("filter") == fs and families.count("net") == len({0, 1, ns // 2, ns - 2, ns - 1} & set(range(ns)))
    assert families.count("reach") == 8 and families.count("seq") == len(ds.SEQUENCES)
    assert {"none", "all", "keep_all", "corners", "edges", "hole", "checkerboard", "random_2", "random_20", "ragged_column",
            "ragged_row"} <= set(names)
    tiles = np.concatenate([b[0] for b in batches])
    keep = np.concatenate([b[1] for b in batches])
    kinds = [("filter", fs, ds.filter_tiles_skippable(tiles, keep, H, W, 4)), ("filter, 3 levels", fs, ds.filter_tiles_skippable(tiles, keep, H, W, 3)),
             ("network", ns, ds.net_tiles_skippable(tiles, keep, H, W, 2)), ("network, 3 layers", ns, ds.net_tiles_skippable(tiles, keep, H, W, 3))]
    for what, strip, skip in kinds:
        sk, lv = ds.positions_seen(skip, strip)
        assert sk == set(range(strip)) and lv == set(range(strip)), (what, sk, lv)  # every ts both skipped and computed
        last_full = ((tiles_x - 1) // strip - 1) * strip  # (the last strip that does not hold the ragged last tile column)
        assert skip[:, :, last_full:last_full + strip].any(), what  # a skippable tile in the last full strip
        assert W % 32 and not skip[:, :, -1].any() and not skip[:, :, 0].any(), what  # none where the frame edge forbids it
        assert not skip[:, 0].any() and not skip[:, -1].any(), what
    seqs = ds.strip_sequences(kinds[0][2], fs)
    for s in ds.SEQUENCES:
        assert s[:fs] in seqs, (s, sorted(seqs))
    # the reach of the filter: the render tile beside a tile's own columns / rows wakes it, the one after that does not
    mid = fs + min(2, fs - 1)
    row = ds.skippable_rows(H, ds.FILT_H, 6)[0]
    for nm, t, _k in patterns:
        if nm.startswith("reach_"):
            live = not ds.filter_tiles_skippable(t[None], [False], H, W, 4)[0, row, mid]
            assert live == nm.endswith("_in"), nm
    # isolated tiles: one computed network tile between skipped ones and the reverse
    nseq = ds.strip_sequences(kinds[2][2], ns)
    if ns >= 3:
        assert any("SLS" in s for s in nseq) and any("LSL" in s for s in ds.strip_sequences(kinds[0][2], fs) | nseq)
    return fs, ns


def test_fixture_covers_the_classes():
    """what the GPU tests below claim to reach, proved on the host through the query and the restated skip predicates"""
    assert _check_coverage(LONG, (5, 13)) == (5, 13)
    reached = [_check_coverage(n, want) for n, want in BATCHES.items() if n != LONG]
    assert {f for f, _ in reached} == {1, 2, 3, 4} and any(3 < s < 13 for _, s in reached)
    assert max(BATCHES) * H * W < 6_000_000


def test_the_query_guards_the_shapes():
    """a small batch in the long-strip batch's place fails the coverage test: the strips come from the query, not from belief"""
    with pytest.raises(AssertionError, match="no longer launches strips"):
        _check_coverage(K, (5, 13))
    with pytest.raises(AssertionError, match="no longer launches strips"):
        _check_coverage(80, (5, 13))


# ---------------------------------------------------------------- gpu

def _same(got, want, what, names=None):
    """bit for bit, compared on the device; a mismatch names its frames (and their mark patterns)"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if torch.equal(g, w):
        return
    bad = g != w
    frames = bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten().tolist()
    first = bad.nonzero()[0].tolist()
    raise AssertionError("%s: %d of %d words differ, in frames %r%s; first at %r: %r vs %r" % (
        what, int(bad.sum()), bad.numel(), frames[:20], "" if names is None else " = " + repr([names[f] for f in frames[:20]]), first,
        float(got[tuple(first)]), float(want[tuple(first)])))


def _upsample(tile_mask, th, tw):
    """bool [n][rows][cols] of th x tw tiles -> bool [n][H][W] on the device"""
    m = torch.from_numpy(np.ascontiguousarray(tile_mask)).to(DEV)
    return m.repeat_interleave(th, 1).repeat_interleave(tw, 2)[:, :H, :W]


def _per_tile_any(px, th, tw):
    """bool [n][H][W] -> bool [n][rows][cols]: any pixel of the th x tw tile"""
    n = px.shape[0]
    ny, nx = ds.ceil_div(H, th), ds.ceil_div(W, tw)
    full = torch.zeros((n, ny * th, nx * tw), dtype=torch.bool, device=DEV)
    full[:, :H, :W] = px
    return full.view(n, ny, th, nx, tw).any(4).any(2)


def _interior(th, tw, margin):
    """bool [H][W]: pixels at least `margin` from every border of their th x tw tile"""
    y, x = torch.arange(H, device=DEV) % th, torch.arange(W, device=DEV) % tw
    return ((y >= margin) & (y < th - margin))[:, None] & ((x >= margin) & (x < tw - margin))[None, :]


class _Scene:
    """K base colour fields on the device and the frames built from them"""

    def __init__(self):
        rs = np.random.RandomState(5)
        self.colours_np = np.stack([ds.random_colours(H, W, rs) for _ in range(K)])
        self.colours = torch.from_numpy(self.colours_np).to(DEV)
        self.nets = {}
        self.single = {}

    def net(self, key):
        if key not in self.nets:
            from test_guidance_shapes import _default_net
            compact = _default_net(*NETS[key], seed=3)
            self.nets[key] = (compact, denoiser.FusedGuidanceNet(compact))
        return self.nets[key]

    def expand(self, content, bg):
        """content bool [n][rows][cols] -> (noisy [n][H][W][4], aux [n][8][H][W]): frame f = compose(base f mod K, content[f], bg)"""
        n = content.shape[0]
        px = _upsample(content, 8, 8)
        bgpix = torch.tensor([bg, bg, bg, 0.0], device=DEV)
        noisy = torch.where(px[..., None], self.colours[torch.arange(n, device=DEV) % K], bgpix).contiguous()
        planes = noisy.permute(0, 3, 1, 2)
        aux = torch.cat([planes, planes * planes], 1).contiguous()
        for f in (0, n - 1):  # the device twin of denoise_synth.compose
            noisy_h, aux_h = ds.compose(self.colours_np[f % K], content[f], bg)
            assert np.array_equal(noisy[f].cpu().numpy().view(np.uint32), noisy_h.view(np.uint32))
            assert np.array_equal(aux[f].cpu().numpy().view(np.uint32), aux_h.view(np.uint32))
        return noisy, aux

    def plain_frames(self, n, bg=0.25):
        """the batch of test a: base f mod K with base content (everything; a fifth of the tiles; a checkerboard; background)"""
        rty, rtx = ds.mark_dims(H, W)
        rs = np.random.RandomState(9)
        yy, xx = np.mgrid[0:rty, 0:rtx]
        base = [np.ones((rty, rtx), bool), rs.random_sample((rty, rtx)) < 0.2, (yy + xx) % 2 == 0, np.zeros((rty, rtx), bool)]
        return self.expand(np.stack([base[f % K] for f in range(n)]), bg)

    def marked_frames(self, tiles, keep, bg, seed):
        rs = np.random.RandomState(seed)
        eff = tiles | keep[:, None, None]
        content = np.stack([ds.content_tiles(e, rs) for e in eff])
        noisy, aux = self.expand(content, bg)
        words = ds.pack_marks(tiles, keep, H, W)
        dev_words = torch.from_numpy(words.view(np.int32)).to(DEV)
        n = tiles.shape[0]
        return noisy, aux, eff, dev_words, (dev_words.data_ptr(), int(words.shape[1]), 0, n, bg)


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def _net_input(mode, aux, noisy):
    if mode == "aux":
        return aux, {}
    if mode == "squares_implied":
        poisoned = aux.clone()
        poisoned[:, 4:] = 123.0  # must not be read
        return poisoned, {"squares_implied": True}
    return noisy, {"rgba": True}  # the interleaved image of a lean launch: r, g, b, alpha


def _planes(fused, inp, prefill=False, **kw):
    if prefill:
        for t in fused(inp, **{k: v for k, v in kw.items() if k != "cull"}):
            t.fill_(-7.0)
    return tuple(t.clone() for t in fused(inp, **kw))


def _filtered(wm, gm, noisy, mode):
    out = torch.full_like(noisy, -7.0)
    R.filtering(None, wm, gm, noisy, out, mode=mode)
    return out


def _packed(fused, inp, noisy, kw=None, cull_net=None, cull_filter=None, noisy_filter=None):
    out = torch.full_like(noisy, -7.0)
    fused.forward_packed(inp, cull=cull_net, **(kw or {}))
    fused.filter_packed(noisy if noisy_filter is None else noisy_filter, out, shape=tuple(noisy.shape[:3]), cull=cull_filter)
    return out


def _unculled(fused, aux, noisy):
    """every route's output without marks"""
    wm, gm = _planes(fused, aux)
    out = {"wm": wm, "gm": gm, "fast": _filtered(wm, gm, noisy, R.FILTER_FAST), "exact": _filtered(wm, gm, noisy, R.FILTER_EXACT)}
    if fused.packed_route:
        out["packed"] = _packed(fused, aux, noisy)
    return out


def _one_at_a_time(scene, key):
    """the K base frames of test a, each in a launch of its own (strip 1)"""
    if key not in scene.single:
        assert ds.launch_strips(1, H, W) == (1, 1)
        _compact, fused = scene.net(key)
        noisy, aux = scene.plain_frames(K)
        outs = [_unculled(fused, aux[k:k + 1].contiguous(), noisy[k:k + 1].contiguous()) for k in range(K)]
        scene.single[key] = {name: torch.cat([o[name] for o in outs]) for name in outs[0]}
    return scene.single[key]


@gpu
@pytest.mark.parametrize("n", [86, 80, 60, 44])
@pytest.mark.parametrize("key", list(NETS))
def test_batch_equals_its_frames_sent_one_at_a_time(scene, key, n):
    """a (and f: n = 80 / 60 / 44 launch filter strips 4 / 3 / 2)"""
    assert ds.launch_strips(n, H, W) == BATCHES[n]
    _compact, fused = scene.net(key)
    single = _one_at_a_time(scene, key)
    idx = torch.arange(n, device=DEV) % K
    want = {name: t[idx] for name, t in single.items()}
    noisy, aux = scene.plain_frames(n)
    torch.cuda.synchronize()
    for mode in ("aux", "squares_implied", "rgba"):
        inp, kw = _net_input(mode, aux, noisy)
        wm, gm = _planes(fused, inp, prefill=True, **kw)
        _same(wm, want["wm"], "weight planes, input %s, %d frames" % (mode, n))
        _same(gm, want["gm"], "guidance planes, input %s, %d frames" % (mode, n))
        if fused.packed_route:
            _same(_packed(fused, inp, noisy, kw), want["packed"], "packed route, input %s, %d frames" % (mode, n))
    _same(_filtered(wm, gm, noisy, R.FILTER_FAST), want["fast"], "factorised filter on planes, %d frames" % n)
    _same(_filtered(wm, gm, noisy, R.FILTER_EXACT), want["exact"], "exact filter, %d frames" % n)
    if fused.packed_route:
        _same(want["packed"], want["fast"], "packed route vs factorised filter on planes")


@gpu
@pytest.mark.parametrize("n", [86, 17])
@pytest.mark.parametrize("key", list(NETS))
def test_batch_against_the_host_oracle_and_the_fp32_network(scene, key, n):
    """b: anchored to something that is not these kernels, on two frames from deep inside the batch"""
    import orc
    from helpers import oracle_threads
    compact, fused = scene.net(key)
    noisy, aux = scene.plain_frames(n)
    got = _unculled(fused, aux, noisy)
    torch.cuda.synchronize()
    for f in (K + 1, n - 4):  # (bases 1 and 2: a fifth of the tiles filled; a checkerboard)
        wm, gm, img = (t[f].cpu().numpy() for t in (got["wm"], got["gm"], noisy))
        ref = orc.filter_levels(wm, gm, img, threads=oracle_threads())
        assert np.array_equal(got["exact"][f].cpu().numpy().view(np.uint32), ref.view(np.uint32)), "exact filter vs the oracle, frame %d" % f
        for route in ("fast", "packed") if fused.packed_route else ("fast",):
            o = got[route][f].cpu().numpy()
            print("%s n %d frame %d: %s route vs the oracle, max |diff| %.3e" % (key, n, f, route, np.abs(o[..., :3] - ref[..., :3]).max()))
            assert np.all(o[..., 3] == 1.0)
            assert np.allclose(o[..., :3], ref[..., :3], rtol=2e-5, atol=2e-6), (route, f, np.abs(o - ref).max())
        if key == "c32_l4_n2":  # test_fused_matches_fp32_network's bound, for the net it states it for
            with torch.no_grad():
                w_ref, g_ref = compact(aux[f:f + 1].cpu())
            print("%s n %d frame %d: planes vs the fp32 network, guidance %.3e weights %.3e" % (
                key, n, f, float((torch.from_numpy(gm) - g_ref[0]).abs().max()), float((torch.from_numpy(wm) - w_ref[0]).abs().max())))
            assert float((torch.from_numpy(gm) - g_ref[0]).abs().max()) < 3e-2
            assert float((torch.from_numpy(wm) - w_ref[0]).abs().max()) < 1e-2
            assert np.allclose(wm.sum(0), 1.0, atol=1e-5)


@gpu
@pytest.mark.parametrize("n", [86, 80, 60, 44, 17])
@pytest.mark.parametrize("key", list(NETS))
def test_culled_entries_under_synthetic_marks(scene, key, n):
    """c (and f): every culled entry == the unculled kernels on frames that keep the marks' promise"""
    _compact, fused = scene.net(key)
    levels, layers = fused.levels, fused.num_layers
    patterns, batches = _batches_of(n, levels)
    bg = 0.25
    for bi, (tiles, keep, names) in enumerate(batches):
        noisy, aux, _eff, _words, cull = scene.marked_frames(tiles, keep, bg, seed=40 + bi)
        want = _unculled(fused, aux, noisy)
        for mode in ("aux", "squares_implied", "rgba"):
            inp, kw = _net_input(mode, aux, noisy)
            wm, gm = _planes(fused, inp, prefill=True, cull=cull, **kw)
            _same(wm, want["wm"], "weight planes, culled network, input %s" % mode, names)
            _same(gm, want["gm"], "guidance planes, culled network, input %s" % mode, names)
        if layers > 2:
            continue  # (rto_filtering_culled: a three-layer net culls its network tiles only)
        for mode, name in ((R.FILTER_EXACT, "exact"), (R.FILTER_FAST, "fast")):
            out = torch.full_like(noisy, -7.0)
            fused.filter_planes(wm, gm, noisy, out, mode=mode, cull=cull)
            _same(out, want[name], "culled %s filter on planes" % name, names)
        if fused.packed_route:
            inp, kw = _net_input("squares_implied", aux, noisy)
            _same(_packed(fused, inp, noisy, kw, cull_net=cull), want["packed"], "culled network, plain packed filter", names)
            _same(_packed(fused, aux, noisy, cull_filter=cull), want["packed"], "plain network, culled packed filter", names)
            _same(_packed(fused, noisy, noisy, {"rgba": True}, cull_net=cull, cull_filter=cull), want["packed"], "both stages culled", names)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("n", [86, 17])
@pytest.mark.parametrize("key", list(NETS))
def test_every_skippable_tile_is_skipped(scene, key, n):
    """d: the poison inside a tile the predicate calls skippable never reaches a culled output, and does reach the plain one"""
    _compact, fused = scene.net(key)
    levels, layers = fused.levels, fused.num_layers
    patterns, batches = _batches_of(n, levels)
    bg = 0.25
    gen = torch.Generator(device=DEV).manual_seed(77)
    for bi, (tiles, keep, names) in enumerate(batches):
        noisy, aux, _eff, _words, cull = scene.marked_frames(tiles, keep, bg, seed=40 + bi)
        want = _unculled(fused, aux, noisy)
        # ---- network tiles (32 x 8): aux pixels at least `layers` inside the tile are read by that tile alone
        nskip = ds.net_tiles_skippable(tiles, keep, H, W, layers)
        assert nskip.any() and not nskip.all()
        spot = _upsample(nskip, 8, 32) & _interior(8, 32, layers)[None]
        bad_aux = aux.clone()
        rnd = torch.rand(aux[:, :3].shape, device=DEV, generator=gen) * 0.5 + 0.5
        bad_aux[:, :3] = torch.where(spot[:, None], rnd, aux[:, :3])
        bad_aux[:, 4:7] = bad_aux[:, :3] * bad_aux[:, :3]
        wm, gm = _planes(fused, bad_aux, prefill=True, cull=cull)
        _same(wm, want["wm"], "weight planes, culled network on poisoned aux", names)
        _same(gm, want["gm"], "guidance planes, culled network on poisoned aux", names)
        wm_p, gm_p = _planes(fused, bad_aux)
        hit = _per_tile_any(((wm_p != want["wm"]) | (gm_p != want["gm"])).any(1), 8, 32)
        missed = torch.from_numpy(nskip).to(DEV) & ~hit
        print("%s n %d batch %d: %d of %d network tiles skippable, the poison reached %d tiles of the plain network" % (
            key, n, bi, int(nskip.sum()), nskip.size, int(hit.sum())))
        assert not bool(missed.any()), "the poison did not reach the plain network in tiles %r" % missed.nonzero()[:8].tolist()
        if fused.packed_route:
            _same(_packed(fused, bad_aux, noisy, cull_net=cull), want["packed"], "culled packed network on poisoned aux", names)
        if layers > 2:
            continue
        # ---- filter tiles (32 x 16): noisy pixels at least `levels` inside the tile are staged by that tile alone
        fskip = ds.filter_tiles_skippable(tiles, keep, H, W, levels)
        assert fskip.any() and not fskip.all()
        spot = _upsample(fskip, 16, 32) & _interior(16, 32, levels)[None]
        bad_noisy = noisy.clone()
        rnd = torch.rand(noisy[..., :3].shape, device=DEV, generator=gen) * 0.5 + 0.5
        bad_noisy[..., :3] = torch.where(spot[..., None], rnd, noisy[..., :3])
        out = torch.full_like(noisy, -7.0)
        fused.filter_planes(want["wm"], want["gm"], bad_noisy, out, mode=R.FILTER_FAST, cull=cull)
        _same(out, want["fast"], "culled factorised filter on a poisoned image", names)
        plain = _filtered(want["wm"], want["gm"], bad_noisy, R.FILTER_FAST)
        hit = _per_tile_any((plain != want["fast"]).any(-1), 16, 32)
        missed = torch.from_numpy(fskip).to(DEV) & ~hit
        print("%s n %d batch %d: %d of %d filter tiles skippable, the poison reached %d tiles of the plain filter" % (
            key, n, bi, int(fskip.sum()), fskip.size, int(hit.sum())))
        assert not bool(missed.any()), "the poison did not reach the plain filter in tiles %r" % missed.nonzero()[:8].tolist()
        if fused.packed_route:
            _same(_packed(fused, aux, noisy, cull_filter=cull, noisy_filter=bad_noisy), want["packed"], "culled packed filter on a poisoned image", names)
            plain = _packed(fused, aux, noisy, noisy_filter=bad_noisy)
            missed = torch.from_numpy(fskip).to(DEV) & ~_per_tile_any((plain != want["packed"]).any(-1), 16, 32)
            assert not bool(missed.any()), "the poison did not reach the plain packed filter in tiles %r" % missed.nonzero()[:8].tolist()
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("n,bg", [(86, 0.0), (86, 0.25), (86, 1.0), (44, 0.25), (17, 1.0)])
def test_sparse_route_under_synthetic_marks(scene, n, bg):
    """e: nothing stored for unmarked tiles (NaN there), stale maps in the scratch -- the same images as the full route"""
    _compact, fused = scene.net("c32_l4_n2")
    patterns, batches = _batches_of(n)
    gen = torch.Generator(device=DEV).manual_seed(78)
    for bi, (tiles, keep, names) in enumerate(batches):
        assert keep.any() and (~tiles.any((1, 2)) & ~keep).any()  # keep-all frames and all-unmarked frames belong in the batch
        noisy, aux, eff, _words, cull = scene.marked_frames(tiles, keep, bg, seed=60 + bi)
        want = _packed(fused, aux, noisy)
        sparse = torch.where(_upsample(eff, 8, 8)[..., None], noisy, torch.full_like(noisy, float("nan")))
        fused.forward_packed(torch.rand(aux.shape, device=DEV, generator=gen))  # unrelated frames of the same extent dirty the scratch
        out = torch.full_like(noisy, -7.0)
        fused.forward_packed(sparse, rgba=True, sparse=True, cull=cull)
        fused.filter_packed(sparse, out, shape=(n, H, W), cull=cull)
        _same(out, want, "sparse route, bg %g" % bg, names)
    torch.cuda.synchronize()
