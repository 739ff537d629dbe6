"""The fused GuidanceNet kernels' output bits, pinned to digests recorded before the two kernels were given one strip frame
(csrc/guidance_strip.inc): SHA-256 of the raw output bytes of guidance_fused<32, 4> and guidance_general on every route, on
an MI355X.  tests/golden/guidance_bits.json holds the digests; `python tests/test_guidance_bits.py OUT.json` writes them anew
(on a GPU, from the build whose bits are to be pinned).

Inputs are integer formulas in numpy (a multiplicative hash of the element index), no RNG of any library, so the digests
move with the kernels only.  n = 2 frames of 101 x 27: 4 tile columns (the last 5 pixels wide), 4 tile rows (the last 3
high), border tiles on all four sides.  The input regions (36 x 12 at halo 2, 38 x 14 at halo 3) of tiles (1, 1), (2, 1),
(1, 2) and (2, 2) lie inside the image; the mark pattern leaves the render tiles under tile (1, 1)'s region unmarked and
marks everything else, so tile (1, 1) -- which also takes stage B's tile_interior path -- is the one tile that is skipped, in
frame 0; frame 1 is kept whole (keep_all).  test_the_marks_leave_exactly_one_tile_skippable proves that on the host.

What is digested: the fp32 weight and guidance planes; on the packed route (whose fp16 maps stay in the handle's scratch)
the image the factorised filter makes of them, so a map byte that moved shows in the pixels around it.  Strip 1 only:
test_denoise_launch_shape ties every longer strip to these launches, bit for bit."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import denoise_synth as ds

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "guidance_bits.json")
gpu = pytest.mark.gpu

N, H, W, BG = 2, 27, 101, 0.25
REF = (32, 4, 2)  # (c1, levels, layers): the reference net, guidance_fused
GENERAL = [(16, 3, 2), (32, 4, 3), (64, 6, 3)]
GENERAL_MARKED = GENERAL[:2]
MODES = ("aux", "squares_implied", "rgba")


def unit(count, salt):
    """float32 [count] in [0, 1): a multiplicative hash of the index, 24 bits of it"""
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(count, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B9)) & m
    x = (x * np.uint64(2654435761)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    x ^= x >> np.uint64(13)
    return (x >> np.uint64(8)).astype(np.float32) / np.float32(1 << 24)


def marks():
    """(tiles bool [N][4][13], keep_all bool [N]): frame 0 marks every render tile but those under tile (1, 1)'s input region
    (columns 3..8 of rows 0..2, the same for halo 2 and halo 3); frame 1 marks nothing and is kept whole"""
    rty, rtx = ds.mark_dims(H, W)
    tiles = np.zeros((N, rty, rtx), bool)
    tiles[0] = True
    tiles[0, 0:3, 3:9] = False
    return tiles, np.array([False, True])


def frames():
    """-> {"plain" | "marked": (noisy [N][H][W][4], aux [N][8][H][W])}: colours in [0, 1.5]; aux planes 4..7 are values of their
    own where a frame holds content (input mode 0 must read them), the squares of the background where it does not.  The marked
    frames keep the marks' promise: exactly (BG, BG, BG, 0) in every unmarked render tile."""
    colours = (unit(N * H * W * 4, 1) * np.float32(1.5)).reshape(N, H, W, 4)
    upper = (unit(N * 4 * H * W, 2) * np.float32(1.5)).reshape(N, 4, H, W)
    tiles, keep = marks()
    out = {}
    for name, content in (("plain", np.ones_like(tiles)), ("marked", tiles | keep[:, None, None])):
        noisy, aux = zip(*(ds.compose(colours[f], content[f], BG) for f in range(N)))
        noisy, aux = np.stack(noisy), np.stack(aux)
        px = np.repeat(np.repeat(content, ds.RT, 1), ds.RT, 2)[:, None, :H, :W]
        aux[:, 4:] = np.where(px, upper, aux[:, 4:])
        out[name] = (noisy, aux)
    return out


def hashed_net(c1, levels, layers, salt):
    """a GuidanceNetCompact whose weights are (u - 0.5) * 4 / cin -- within [-0.5, 0.5], scaled by a power of two so that the
    sums of a wide layer stay inside ReLU6's range -- and whose biases are u - 0.5"""
    import torch
    from rt_octree_amd import denoiser
    net = denoiser.GuidanceNetCompact(8, c1, layers, levels).eval()
    with torch.no_grad():
        for i, layer in enumerate(net.layers):
            w, b = layer.conv.weight, layer.conv.bias
            wv = (unit(w.numel(), salt + 2 * i) - np.float32(0.5)) * np.float32(4.0 / w.shape[1])
            w.copy_(torch.from_numpy(wv.reshape(tuple(w.shape))))
            b.copy_(torch.from_numpy(unit(b.numel(), salt + 2 * i + 1) - np.float32(0.5)))
    return net


def case_ids():
    ids = []
    for kind in ("plain", "marked"):
        ids += ["c32_l4_n2-%s-%s-%s" % (mode, route, kind) for mode in MODES for route in ("planes", "packed")]
    ids.append("c32_l4_n2-rgba-sparse-marked")
    ids += ["c%d_l%d_n%d-%s-planes-plain" % (s + (mode,)) for s in GENERAL for mode in MODES]
    ids += ["c%d_l%d_n%d-%s-planes-marked" % (s + (mode,)) for s in GENERAL_MARKED for mode in MODES]
    return ids


# ---------------------------------------------------------------- not gpu

def test_the_marks_leave_exactly_one_tile_skippable():
    tiles, keep = marks()
    want = np.zeros((N, ds.ceil_div(H, ds.NET_H), ds.ceil_div(W, ds.NET_W)), bool)
    assert want.shape == (N, 4, 4) and W % 32 == 5 and H % 8 == 3
    want[0, 1, 1] = True
    for halo in (2, 3):
        assert np.array_equal(ds.net_tiles_skippable(tiles, keep, H, W, halo), want), halo
        # (unmarked, four tiles' input regions lie inside the image: the pattern wakes three of them)
        free = ds.net_tiles_skippable(np.zeros_like(tiles), np.zeros_like(keep), H, W, halo)
        assert free.sum(axis=(1, 2)).tolist() == [4, 4] and free[0, 1:3, 1:3].all()
    assert 32 >= 1 and 32 + ds.NET_W + 1 <= W and 8 >= 1 and 8 + ds.NET_H + 1 <= H  # tile (1, 1): guidance_fused's tile_interior
    f = frames()
    noisy, aux = f["marked"]
    px = np.repeat(np.repeat(tiles | keep[:, None, None], ds.RT, 1), ds.RT, 2)[:, :H, :W]
    assert np.all(noisy[~px] == np.array([BG, BG, BG, 0], np.float32)) and (~px).sum() == 24 * 48
    assert np.array_equal(aux[:, :4], noisy.transpose(0, 3, 1, 2)) and not np.array_equal(aux[:, 4:], aux[:, :4] * aux[:, :4])
    assert np.array_equal(aux[:, 4:].transpose(0, 2, 3, 1)[~px], (aux[:, :4] * aux[:, :4]).transpose(0, 2, 3, 1)[~px])
    assert 0 <= f["plain"][0].min() and 1.4 < f["plain"][0].max() <= 1.5


def test_the_fixture_holds_a_digest_per_case():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(case_ids()) and len(golden) == 28
    assert all(len(d) == 64 and int(d, 16) >= 0 for d in golden.values())
    assert len(set(golden.values())) > len(GENERAL) + 2  # (input modes agree with each other; nets, routes and frames do not)


# ---------------------------------------------------------------- gpu

class _Bits:
    def __init__(self):
        import torch
        from rt_octree_amd import denoiser
        self.torch, self.dev = torch, "cuda:0"
        test_the_marks_leave_exactly_one_tile_skippable()  # (a condition on the input the digests were recorded on)
        self.frames = {k: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in v) for k, v in frames().items()}
        tiles, keep = marks()
        words = ds.pack_marks(tiles, keep, H, W)
        self.words = torch.from_numpy(words.view(np.int32)).to(self.dev)
        self.cull = (self.words.data_ptr(), int(words.shape[1]), 0, N, BG)
        px = np.repeat(np.repeat(tiles | keep[:, None, None], ds.RT, 1), ds.RT, 2)[:, :H, :W]
        self.stored = torch.from_numpy(px).to(self.dev)
        self.nets = {s: denoiser.FusedGuidanceNet(hashed_net(*s, salt=10 + 10 * i)) for i, s in enumerate([REF] + GENERAL)}
        assert self.nets[REF].packed_route and not any(self.nets[s].packed_route for s in GENERAL)

    def digest(self, case):
        torch = self.torch
        shape, mode, route, kind = case.split("-")
        fused = self.nets[tuple(int(p[1:]) for p in shape.split("_"))]
        noisy, aux = self.frames[kind]
        cull = self.cull if kind == "marked" else None
        if mode == "aux":
            inp, kw = aux, {}
        elif mode == "squares_implied":
            inp, kw = aux.clone(), {"squares_implied": True}
            inp[:, 4:] = 123.0  # must not be read
        else:
            inp, kw = noisy, {"rgba": True}
        if route == "planes":
            for t in fused(inp, **kw):
                t.fill_(-7.0)
            outs = fused(inp, cull=cull, **kw)
        else:
            out = torch.full_like(noisy, -7.0)
            if route == "sparse":  # nothing was stored for the unmarked render tiles; the scratch holds another frame's maps
                inp = torch.where(self.stored[..., None], noisy, torch.full_like(noisy, float("nan")))
                fused.forward_packed(self.frames["plain"][1])
                fused.forward_packed(inp, cull=cull, sparse=True, **kw)
                fused.filter_packed(inp, out, shape=(N, H, W), cull=cull)
            else:
                fused.forward_packed(inp, cull=cull, **kw)
                fused.filter_packed(noisy, out, shape=(N, H, W))
            outs = (out,)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in outs:
            a = t.cpu().numpy()
            assert np.isfinite(a).all() and not (a == -7.0).any(), case
            h.update(a.tobytes())
        return h.hexdigest()


@pytest.fixture(scope="module")
def bits():
    return _Bits()


@gpu
@pytest.mark.parametrize("case", case_ids())
def test_output_bits_are_the_recorded_ones(bits, case):
    got, want = bits.digest(case), json.load(open(GOLDEN))[case]
    print(case, got)
    assert got == want, case


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    b = _Bits()
    with open(sys.argv[1], "w") as f:
        json.dump({c: b.digest(c) for c in case_ids()}, f, indent=1, sort_keys=True)
        f.write("\n")
