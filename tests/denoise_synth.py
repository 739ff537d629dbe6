"""Synthetic inputs of the denoise stage at batch launch shape: frames built from arbitrary tile marks, the mark patterns a
render of one tree never produces, and the skip decisions of the kernels restated on the host.  Pure numpy; no GPU.

The culled entry points (rto_*_culled) take a bare pointer to tile marks: bit t of a frame's words = the 8x8 render tile t
(row-major) MAY hold something, bit 0 of the frame's last word = keep the whole frame.  The promise behind a clear bit: every
pixel of that tile is the background, colour (bg, bg, bg), alpha 0.  frame_from_marks builds frames that keep it.

A workgroup of the factorised filter (tiles 32 x 16) and of the GuidanceNet kernels (tiles 32 x 8) walks a strip of tiles
along x; the strip's length follows from the launch size (rto_denoise_launch_strips; strips_by_rule restates the rule)."""
import numpy as np

RT = 8                       # render tile edge
FILT_W, FILT_H = 32, 16      # filter_fast's output tile
EXACT_W, EXACT_H = 32, 8     # filter_fused's
NET_W, NET_H = 32, 8         # guidance_fused's / guidance_general's
MAP_HALO = 2                 # what the filter kernels add to their staged region for the network's receptive field
SEQUENCES = ("LSLSL", "SLSLS", "SSSSL", "LSSSS", "SSLSS")  # live / skipped filter tiles of one strip


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- launch shape

def strips_by_rule(n, H, W):
    """(filter strip, network strip) of a launch of n frames of H x W: the launchers' rule, restated"""
    def rule(s, tw, th):
        tiles_x, tiles_y = ceil_div(W, tw), ceil_div(H, th)
        while s > 1 and ceil_div(tiles_x, s) * tiles_y * n < 2048:
            s -= 1
        return s
    return rule(5, FILT_W, FILT_H), rule(13, NET_W, NET_H)


def launch_strips(n, H, W):
    """the same from the library (rto_denoise_launch_strips: computed by the functions the launchers call)"""
    import ctypes as C

    import rt_octree_amd as R
    from rt_octree_amd import _lib
    fs, ns = C.c_int(-1), C.c_int(-1)
    _lib.check(R.lib().rto_denoise_launch_strips(n, H, W, C.byref(fs), C.byref(ns)))
    return fs.value, ns.value


def filter_strip_in_kernel(W, fs):
    """filter_fast derives its strip from the grid the launcher chose: ceil(tiles_x / gridDim.x)"""
    tiles_x = ceil_div(W, FILT_W)
    return ceil_div(tiles_x, ceil_div(tiles_x, fs))


# ---------------------------------------------------------------- marks

def mark_dims(H, W):
    return ceil_div(H, RT), ceil_div(W, RT)


def mark_words(H, W):
    rty, rtx = mark_dims(H, W)
    return ceil_div(rty * rtx, 32) + 1


def pack_marks(tiles, keep_all, H, W):
    """tiles bool [n][rows][cols] of render tiles, keep_all bool [n] -> uint32 [n][(tiles + 31) // 32 + 1]: bit t = tile t,
    row-major; bit 0 of the last word = keep the whole frame"""
    tiles = np.asarray(tiles, bool)
    n = tiles.shape[0]
    assert tiles.shape[1:] == mark_dims(H, W)
    flat = tiles.reshape(n, -1)
    words = mark_words(H, W)
    out = np.zeros((n, words), np.uint32)
    t = np.arange(flat.shape[1])
    for f in range(n):
        idx = t[flat[f]]
        np.bitwise_or.at(out[f], idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
        out[f, words - 1] = 1 if keep_all[f] else 0
    return out


def unpack_marks(words, H, W):
    """uint32 [n][words] -> (tiles bool [n][rows][cols], keep_all bool [n])"""
    words = np.asarray(words, np.uint32)
    rty, rtx = mark_dims(H, W)
    t = np.arange(rty * rtx)
    bits = (words[:, t >> 5] >> (t & 31).astype(np.uint32)) & 1
    return bits.astype(bool).reshape(-1, rty, rtx), (words[:, -1] & 1).astype(bool)


# ---------------------------------------------------------------- the kernels' skip decisions, restated

def tiles_skippable(tiles, keep_all, H, W, tw, th, grow):
    """bool [n][ceil(H / th)][ceil(W / tw)]: the tw x th tile's region grown by `grow` pixels lies inside the frame and in
    unmarked render tiles of a frame that is not kept whole.  The factorised filter: (32, 16, levels + 2); the exact filter:
    (32, 8, levels + 2); the network: (32, 8, number of layers)."""
    tiles = np.asarray(tiles, bool)
    n = tiles.shape[0]
    ny, nx = ceil_div(H, th), ceil_div(W, tw)
    out = np.zeros((n, ny, nx), bool)
    for ty in range(ny):
        y0, y1 = ty * th - grow, ty * th + th + grow
        if y0 < 0 or y1 > H:
            continue
        for tx in range(nx):
            x0, x1 = tx * tw - grow, tx * tw + tw + grow
            if x0 < 0 or x1 > W:
                continue
            marked = tiles[:, y0 >> 3:((y1 - 1) >> 3) + 1, x0 >> 3:((x1 - 1) >> 3) + 1].any((1, 2))
            out[:, ty, tx] = ~marked & ~np.asarray(keep_all, bool)
    return out


def filter_tiles_skippable(tiles, keep_all, H, W, levels=4, exact=False):
    tw, th = (EXACT_W, EXACT_H) if exact else (FILT_W, FILT_H)
    return tiles_skippable(tiles, keep_all, H, W, tw, th, levels + MAP_HALO)


def net_tiles_skippable(tiles, keep_all, H, W, layers=2):
    return tiles_skippable(tiles, keep_all, H, W, NET_W, NET_H, layers)


def net_tiles_skipped_and_computed(words, H, W, halo):
    """from packed tile marks [n][words]: (network tiles 32 x 8 whose input region lies inside the image and in unmarked render
    tiles, others)"""
    tiles, keep_all = unpack_marks(words, H, W)
    skip = net_tiles_skippable(tiles, keep_all, H, W, halo)
    return int(skip.sum()), int(skip.size - skip.sum())


def strip_sequences(skip, strip):
    """skip bool [n][tiles_y][tiles_x] -> the set of strings a workgroup sees along its strip: L = computed, S = skipped"""
    n, ny, nx = skip.shape
    seen = set()
    for x0 in range(0, nx, strip):
        part = skip[:, :, x0:x0 + strip].reshape(n * ny, -1)
        for row in np.unique(part, axis=0):
            seen.add("".join("S" if s else "L" for s in row))
    return seen


def positions_seen(skip, strip):
    """-> (set of strip positions ts at which some tile is skipped, ... is computed)"""
    nx = skip.shape[2]
    ts = np.arange(nx) % strip
    sk = {int(t) for t in np.unique(ts[skip.any((0, 1))])}
    lv = {int(t) for t in np.unique(ts[(~skip).any((0, 1))])}
    return sk, lv


# ---------------------------------------------------------------- frames

def random_colours(H, W, rs):
    """[H][W][4] float32: colours in [0, 1), alpha in (0, 1]"""
    c = rs.random_sample((H, W, 4)).astype(np.float32)
    c[..., 3] = np.float32(1.0) - c[..., 3] * np.float32(0.98)
    return c


def content_tiles(marks_2d, rs):
    """the marked tiles that hold something: a mark only says "may", so of a frame with more than 8 marked tiles about a fifth
    stay entirely at background.  (A frame with few marks keeps all of them filled: a tile wrongly skipped there must show.)"""
    marks_2d = np.asarray(marks_2d, bool)
    if marks_2d.sum() <= 8:
        return marks_2d.copy()
    return marks_2d & (rs.random_sample(marks_2d.shape) >= 0.2)


def compose(colours, content, bg):
    """colours [H][W][4] inside the 8x8 tiles of `content`, (bg, bg, bg, 0) elsewhere -> (noisy [H][W][4], aux [8][H][W]):
    aux planes 0..3 = r, g, b, alpha, planes 4..7 their fp32 squares (what the renderer writes)"""
    H, W = colours.shape[:2]
    px = np.repeat(np.repeat(np.asarray(content, bool), RT, 0), RT, 1)[:H, :W]
    noisy = np.where(px[..., None], colours, np.array([bg, bg, bg, 0.0], np.float32)).astype(np.float32)
    planes = np.ascontiguousarray(noisy.transpose(2, 0, 1))
    return noisy, np.concatenate([planes, planes * planes], 0)


def frame_from_marks(marks_2d, H, W, bg, rs):
    """one frame that keeps the marks' promise -> (noisy RGBA [H][W][4], aux [8][H][W]).  marks_2d: bool [rows][cols] of render
    tiles (all True for a frame that is kept whole).  Pixels of unmarked tiles are exactly (bg, bg, bg, 0); marked tiles hold
    random colours with alpha in (0, 1], some of them nothing but background."""
    assert np.asarray(marks_2d).shape == mark_dims(H, W)
    colours = random_colours(H, W, rs)
    return compose(colours, content_tiles(marks_2d, rs), bg)


# ---------------------------------------------------------------- the mark patterns

def skippable_rows(H, th, grow):
    return [ty for ty in range(ceil_div(H, th)) if ty * th - grow >= 0 and ty * th + th + grow <= H]


def mark_patterns(H, W, fs, ns, levels=4, seed=11):
    """[(name, tiles bool [rows][cols], keep_all)] for a launch whose filter workgroups walk strips of fs tiles and whose network
    workgroups strips of ns.  A filter tile is made live by the render tile at its columns 8..15: further than the filter's
    reach (levels + 2 <= 8) from both neighbours along x, so they stay skippable."""
    rty, rtx = mark_dims(H, W)
    rs = np.random.RandomState(seed)
    ftx, ntx = ceil_div(W, FILT_W), ceil_div(W, NET_W)
    frows = skippable_rows(H, FILT_H, levels + MAP_HALO)
    nrows = skippable_rows(H, NET_H, 3)
    assert len(frows) >= 2 and len(nrows) >= 4, "the frame is too low for a tile row to be skippable (H >= 54)"
    fr1, fr2 = 2 * frows[0], 2 * frows[-1] + 1  # render rows inside the first / last skippable filter tile row
    nr1, nr2 = nrows[1], nrows[-2]                # ... network tile rows (a mark also wakes the rows above and below)
    out = []

    def empty():
        return np.zeros((rty, rtx), bool)

    def add(name, tiles, keep_all=False):
        out.append((name, tiles, keep_all))

    def put(tiles, row, col):
        if 0 <= row < rty and 0 <= col < rtx:
            tiles[row, col] = True

    add("none", empty())
    add("all", np.ones((rty, rtx), bool))
    add("keep_all", empty(), True)
    t = empty()
    for r, c in ((0, 0), (0, rtx - 1), (rty - 1, 0), (rty - 1, rtx - 1)):
        t[r, c] = True
    add("corners", t)
    t = empty()
    for r, c in ((0, rtx // 2), (rty - 1, rtx // 2), (rty // 2, 0), (rty // 2, rtx - 1)):
        t[r, c] = True
    add("edges", t)
    mid = fs + min(2, fs - 1)  # a filter tile in the middle of the second strip
    t = np.ones((rty, rtx), bool)
    t[fr1, 4 * mid + 1] = False
    add("hole", t)
    for ts in range(fs):  # one marked tile inside filter tile ts of the first strip and of the second
        t = empty()
        put(t, fr1, 4 * ts + 1)
        put(t, fr2, 4 * (fs + ts) + 1)
        add("filter_ts%d" % ts, t)
    for ts in sorted({0, 1, ns // 2, ns - 2, ns - 1} & set(range(ns))):  # ... network tile ts; ts 0: the second strip's first tile
        t = empty()
        put(t, nr1, 4 * ts + 1)
        put(t, nr2, 4 * (ns + ts) + 1)
        add("net_ts%d" % ts, t)
    # beside a filter tile in the middle of a strip: the render-tile column / row next to the tile's own lies inside the filter's
    # reach (the tile is live), the one after it outside (skipped)
    c0, r0 = 4 * mid, 2 * frows[0]
    for name, row, col in (("left_in", fr1, c0 - 1), ("left_out", fr1, c0 - 2), ("right_in", fr1, c0 + 4), ("right_out", fr1, c0 + 5),
                           ("above_in", r0 - 1, c0 + 1), ("above_out", r0 - 2, c0 + 1), ("below_in", r0 + 2, c0 + 1),
                           ("below_out", r0 + 3, c0 + 1)):
        t = empty()
        put(t, row, col)
        add("reach_" + name, t)
    for seq in SEQUENCES:  # live and skipped filter tiles inside one strip: the second strip, and the last full one
        t = empty()
        last_full = ((ftx - 1) // fs - 1) * fs  # (the last strip that does not hold the ragged last tile column)
        for x0, row in ((fs, fr1), (last_full, fr2)):
            for ts, ch in enumerate(seq[:fs]):
                if ch == "L":
                    put(t, row, 4 * (x0 + ts) + 1)
        add("seq_" + seq, t)
    yy, xx = np.mgrid[0:rty, 0:rtx]
    add("checkerboard", (yy + xx) % 2 == 0)
    add("random_2", rs.random_sample((rty, rtx)) < 0.02)
    add("random_20", rs.random_sample((rty, rtx)) < 0.20)
    t = empty()
    t[:, rtx - 1] = True
    add("ragged_column", t)
    t = empty()
    t[rty - 1, :] = True
    add("ragged_row", t)
    return out


def batch_marks(patterns, n, first=0):
    """frame f of a batch carries pattern (first + f) mod len(patterns) -> (tiles bool [n][rows][cols], keep_all bool [n], names)"""
    pick = [patterns[(first + f) % len(patterns)] for f in range(n)]
    return np.stack([p[1] for p in pick]), np.array([p[2] for p in pick], bool), [p[0] for p in pick]
