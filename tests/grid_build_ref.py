"""numpy model of the grid builder as include/rto.h "grid builder" defines it (the pyramid of uniform cells bottom-up, then the
nodes breadth-first), the grid's full octree (what the simplifier is given in cross-check A), and the grids the host and GPU
tests share.  Grids are uint16 bit patterns [R,R,R,D]."""
import functools

import numpy as np

CORNER = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.int64)  # slot 4 i + 2 j + k


def _thresh(kill_thresh):
    with np.errstate(over="ignore"):
        return np.float32(kill_thresh).astype(np.float16)


def build(grid, kill_thresh=None):
    """grid uint16 / float16 [R,R,R,D] -> (child int32 [n,2,2,2], data float16 [n,2,2,2,D], stats dict)"""
    rec = np.ascontiguousarray(grid).view(np.uint16).copy()
    R, D = rec.shape[0], rec.shape[3]
    L = R.bit_length() - 1
    assert rec.shape[:3] == (R, R, R) and 1 << L == R and L >= 1
    killed = 0
    if kill_thresh is not None:
        dead = ~(rec[..., D - 1].view(np.float16) > _thresh(kill_thresh))
        rec[dead] = 0
        killed = int(dead.sum())
    # the pyramid: uni[l][x,y,z] and the record of the cell's min-corner voxel rep[l][x,y,z]
    uni, rep = {L: np.ones((R, R, R), bool)}, {L: rec}
    for l in range(L - 1, -1, -1):
        n = 1 << l
        u = uni[l + 1].reshape(n, 2, n, 2, n, 2)
        r = rep[l + 1].reshape(n, 2, n, 2, n, 2, D)
        same = (r == r[:, :1, :, :1, :, :1]).all((1, 3, 5, 6))
        uni[l] = u.all((1, 3, 5)) & same
        rep[l] = r[:, 0, :, 0, :, 0]
    # the nodes, level by level; within a level parents in order, then slots: Morton order
    coords = np.zeros((1, 3), np.int64)
    childs, datas = [], []
    first = 0
    levels = 0
    for l in range(L):
        n = coords.shape[0]
        sub = coords[:, None, :] * 2 + CORNER[None]
        u = uni[l + 1][sub[..., 0], sub[..., 1], sub[..., 2]]
        mixed = ~u
        ids = np.zeros((n, 8), np.int64)
        ids[mixed] = first + n + np.arange(int(mixed.sum()))
        childs.append(np.where(mixed, ids - (first + np.arange(n))[:, None], 0).astype(np.int32))
        datas.append(np.where(u[..., None], rep[l + 1][sub[..., 0], sub[..., 1], sub[..., 2]], 0).astype(np.uint16))
        levels = l + 1
        first += n
        coords = sub[mixed]
        if coords.shape[0] == 0:
            break
    child = np.concatenate(childs, 0).reshape(-1, 2, 2, 2)
    data = np.concatenate(datas, 0).reshape(-1, 2, 2, 2, D).view(np.float16)
    return child, data, dict(nodes=int(child.shape[0]), killed=killed, levels=levels)


def morton_coords(l):
    """[8^l, 3]: the coordinates of the cells of level l in Morton order (x the most significant bit of each triple)"""
    m = np.arange(1 << (3 * l), dtype=np.int64)
    out = np.zeros((m.size, 3), np.int64)
    for b in range(l):
        out[:, 2] |= ((m >> (3 * b)) & 1) << b
        out[:, 1] |= ((m >> (3 * b + 1)) & 1) << b
        out[:, 0] |= ((m >> (3 * b + 2)) & 1) << b
    return out


def full_tree(grid):
    """every cell subdivided to level L, breadth-first in Morton order, the voxel records in the deepest nodes' slots, interior
    slots zero -> (child int32 [n,2,2,2], data float16 [n,2,2,2,D])"""
    g = np.ascontiguousarray(grid).view(np.uint16)
    R, D = g.shape[0], g.shape[3]
    L = R.bit_length() - 1
    counts = [1 << (3 * l) for l in range(L)]
    start = np.concatenate([[0], np.cumsum(counts)])
    n = int(start[-1])
    child = np.zeros((n, 8), np.int32)
    data = np.zeros((n, 8, D), np.uint16)
    for l in range(L - 1):
        m = np.arange(counts[l], dtype=np.int64)
        child[start[l]:start[l + 1]] = (start[l + 1] + 8 * m[:, None] + np.arange(8)[None]) - (start[l] + m[:, None])
    c = morton_coords(L)
    data[start[L - 1]:] = g[c[:, 0], c[:, 1], c[:, 2]].reshape(-1, 8, D)
    return child.reshape(n, 2, 2, 2), data.reshape(n, 2, 2, 2, D).view(np.float16)


# ---------------------------------------------------------------- grids
H = lambda x: int(np.float16(x).view(np.uint16))  # noqa: E731


def hier_grid(L, D, seed, p=0.35, values=None, densities=None):
    """uniform regions of every size: a random record, then per level the grid doubled and a share p of the cells redrawn.
    values / densities: the few bit patterns the halves are drawn from (so that equal records are common)"""
    rng = np.random.default_rng(seed)
    values = np.asarray(values if values is not None else [0, H(0.5), H(-1.25), H(3.0)], np.uint16)
    densities = np.asarray(densities if densities is not None else [0, H(0.25), H(2.0), H(40.0)], np.uint16)

    def draw(n):
        r = values[rng.integers(0, values.size, (n, D))]
        r[:, D - 1] = densities[rng.integers(0, densities.size, n)]
        return r
    g = draw(1).reshape(1, 1, 1, D)
    for l in range(1, L + 1):
        g = g.repeat(2, 0).repeat(2, 1).repeat(2, 2)
        pick = rng.random(g.shape[:3]) < (p if l < L else p / 2)
        g[pick] = draw(int(pick.sum()))
    return np.ascontiguousarray(g)


def random_grid(L, D, seed):
    R = 1 << L
    return np.random.default_rng(seed).integers(0, 0x7C00, (R, R, R, D)).astype(np.uint16)  # finite, non-negative, all different


def filled(L, D, record):
    R = 1 << L
    return np.ascontiguousarray(np.broadcast_to(np.asarray(record, np.uint16), (R, R, R, D)))


def _ramp(D):
    return (np.arange(D, dtype=np.float32) * 0.25 + 1.0).astype(np.float16).view(np.uint16)


def one_voxel_differs(pos, D=4):
    """L = 2: a uniform grid but for one voxel of the block at (2, 2, 0), at position pos of the block"""
    g = filled(2, D, _ramp(D)).copy()
    g[2 + (pos >> 2), 2 + ((pos >> 1) & 1), pos & 1, 0] ^= 1
    return g


def one_half_differs(j, D=13):
    g = filled(2, D, _ramp(D)).copy()
    g[1, 2, 3, j] ^= 0x0200
    return g


def octant_uniform():
    g = random_grid(4, 5, 3)
    g[8:, :8, 8:] = _ramp(5)
    return g


def single_voxel(L, D=4):
    g = filled(L, D, np.zeros(D, np.uint16)).copy()
    g[-1, -1, -1] = _ramp(D)
    return g


def kill_makes_uniform():
    """L = 2: the block at the origin holds eight different records, all with density 1; every other voxel is dense"""
    g = random_grid(2, 4, 8)
    g[..., 3] = H(5.0)
    g[:2, :2, :2, 3] = H(1.0)
    return g


SPECIAL = [0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x8001, 0x0000, H(65504.0), H(-2.0), H(1.0)]


def special_grid(L=3, D=4, seed=14):
    """densities from NaN, the infinities, -0, subnormals, 65504 and ordinary ones; colours 0 or 0.5, so that all-zero records
    with a live density (under a negative threshold) meet dead records"""
    return hier_grid(L, D, seed, p=0.5, values=[0, 0, H(0.5)], densities=SPECIAL)


# name -> builder of (grid, kill_thresh): what the host twin and the kernels are both held to
CASES = {}
for _L in (1, 2, 3, 4):
    CASES["hier_L%d" % _L] = lambda L=_L: (hier_grid(L, 4, 10 + L), None)
    CASES["hier_L%d_kill" % _L] = lambda L=_L: (hier_grid(L, 4, 20 + L), 0.25)
CASES["random_L5_D1"] = lambda: (random_grid(5, 1, 1), None)  # 4096 nodes on the deepest level: 16 tiles of the scan
CASES["hier_L5_D4_kill"] = lambda: (hier_grid(5, 4, 31, p=0.2), 1.0)
for _D in (1, 4, 5, 13, 28, 49):
    CASES["hier_L3_D%d" % _D] = lambda D=_D: (hier_grid(3, D, 40 + D), None)
    CASES["hier_L3_D%d_kill" % _D] = lambda D=_D: (hier_grid(3, D, 50 + D), 1.0)
CASES["all_zero"] = lambda: (filled(2, 4, np.zeros(4, np.uint16)), None)
CASES["all_zero_kill"] = lambda: (filled(3, 5, np.zeros(5, np.uint16)), 0.0)
CASES["uniform_nonzero"] = lambda: (filled(3, 13, _ramp(13)), None)
CASES["octant_uniform"] = lambda: (octant_uniform(), None)
for _p in range(8):
    CASES["one_voxel_differs_%d" % _p] = lambda p=_p: (one_voxel_differs(p), None)
CASES["first_half_differs"] = lambda: (one_half_differs(0), None)
CASES["middle_half_differs"] = lambda: (one_half_differs(6), None)
CASES["last_half_differs"] = lambda: (one_half_differs(12), None)
CASES["plus_zero_against_minus_zero"] = lambda: (_with(filled(2, 4, np.zeros(4, np.uint16)), (3, 0, 1, 1), 0x8000), None)
CASES["minus_zero_density"] = lambda: (_with(filled(2, 4, np.zeros(4, np.uint16)), (0, 1, 2, 3), 0x8000), None)
CASES["minus_zero_density_kill"] = lambda: (_with(filled(2, 4, np.zeros(4, np.uint16)), (0, 1, 2, 3), 0x8000), 0.0)
CASES["equal_nan_records"] = lambda: (filled(2, 5, np.full(5, 0x7E00, np.uint16)), None)
CASES["nan_records_differ_in_payload"] = lambda: (_with(filled(2, 5, np.full(5, 0x7E00, np.uint16)), (2, 3, 0, 2), 0x7E01), None)
CASES["nan_density"] = lambda: (special_grid(), None)
CASES["nan_density_kill0"] = lambda: (special_grid(), 0.0)
CASES["kill_makes_uniform"] = lambda: (kill_makes_uniform(), 2.0)
CASES["kill_makes_uniform_without_kill"] = lambda: (kill_makes_uniform(), None)
CASES["kill_65504"] = lambda: (special_grid(seed=15), 65504.0)
CASES["kill_beyond_fp16"] = lambda: (special_grid(seed=16), 1e6)  # the threshold becomes an infinity: everything is dead
CASES["kill_negative"] = lambda: (special_grid(seed=17), -1.0)
CASES["kill_minus_inf"] = lambda: (special_grid(seed=18), -np.inf)
CASES["kill_rounded"] = lambda: (hier_grid(3, 4, 19), 0.25006)  # rounds to 0.25 in fp16
CASES["single_voxel_L1"] = lambda: (single_voxel(1), None)
CASES["single_voxel_L4"] = lambda: (single_voxel(4), None)
CASES["single_voxel_L4_kill"] = lambda: (single_voxel(4, 5), 0.0)


def _with(g, at, value):
    g = g.copy()
    g[at] = value
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """(grid uint16, kill_thresh, want) with want = the model's (child, data, stats), computed once"""
    grid, kill = CASES[name]()
    grid = np.ascontiguousarray(grid, np.uint16)
    want = build(grid, kill)
    for a in (grid,) + want[:2]:
        a.setflags(write=False)
    return grid, kill, want


def assert_same(got, want, where=""):
    """got / want: (child, data, stats)"""
    assert {k: got[2][k] for k in ("nodes", "killed", "levels")} == want[2], (where, got[2], want[2])
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (where, got[0].shape, want[0].shape)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), where + ": child differs"
    g, w = np.ascontiguousarray(got[1]).view(np.uint16), np.ascontiguousarray(want[1]).view(np.uint16)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d halves of data differ, first at %s" % (where, len(bad), bad[0].tolist())


def sample_tree(child, data, L):
    """the tree sampled at the voxel centres of the 2^L grid with the numpy walk of simplify_ref.descend -> uint16 [R,R,R,D]"""
    import simplify_ref as SR
    R = 1 << L
    c = (np.arange(R) + 0.5) / R
    pts = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    rec, _ = SR.descend(child, data, pts)
    return rec.reshape(R, R, R, -1)
