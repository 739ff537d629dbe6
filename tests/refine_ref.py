"""numpy model of the tree refiner as include/rto.h "refiner" defines it, the trees and keys the host and GPU tests share (the
simplifier's trees, imported from simplify_ref, plus a one-node tree and a 31-level chain), and the comparison of two results."""
import functools

import numpy as np

import simplify_ref as SR
from simplify_ref import FormatError  # noqa: F401

STAT_KEYS = ("reachable", "candidates", "selected", "levels", "cut_key", "capacity_in", "capacity")


class TooLarge(Exception):
    def __init__(self, stats):
        super().__init__("cap_out * N^3 >= 2^31")
        self.stats = stats


def levels_of(child):
    """the level of every node (-1 = unreachable) by the simplifier's rules; FormatError for what they refuse"""
    child = np.asarray(child)
    cap = child.shape[0]
    ch = child.reshape(cap, -1).astype(np.int64)
    n_of, s_of = np.nonzero(ch)
    tgt = n_of + ch[n_of, s_of]
    if ((tgt < 1) | (tgt >= cap)).any():
        raise FormatError("an offset refers outside [1, cap)")
    if np.unique(tgt).size != tgt.size:
        raise FormatError("a node is referred to by more than one slot")
    level = np.full(cap, -1, np.int64)
    level[0] = 0
    l = 0
    while True:
        nodes = np.flatnonzero(level == l)
        if nodes.size == 0:
            break
        if l >= 32:
            raise FormatError("the walk from the root does not end within 32 levels")
        rows = ch[nodes]
        level[(nodes[:, None] + rows)[rows != 0]] = l + 1
        l += 1
    return level


def refine(child, data, key=None, key_thresh=1, max_new=-1, max_level=31):
    """child int32 [cap,N,N,N], data float16 [cap,N,N,N,D], key uint32 per slot or None -> (child, data, slot_src int32, stats)"""
    child = np.asarray(child)
    cap, N, D = child.shape[0], child.shape[1], data.shape[-1]
    S = N ** 3
    level = levels_of(child)
    ch = child.reshape(-1)
    keys = np.ones(cap * S, np.uint32) if key is None else np.asarray(key).reshape(-1).view(np.uint32)
    lv = np.repeat(level, S)
    cand = np.flatnonzero((ch == 0) & (lv >= 0) & (lv + 1 <= max_level) & (keys >= np.uint32(key_thresh)))
    C = cand.size
    K = C if max_new < 0 else min(C, int(max_new))
    order = np.lexsort((cand, -keys[cand].astype(np.int64)))  # key descending, then slot ascending
    sel = np.sort(cand[order[:K]])
    cap_out = cap + K
    stats = dict(reachable=int((level >= 0).sum()), candidates=int(C), selected=int(K),
                 levels=int(max(level.max(), (lv[sel] + 1).max() if K else 0)) + 1,
                 cut_key=int(keys[sel].min()) if K else 0, capacity_in=int(cap), capacity=int(cap_out))
    if cap_out * S >= 2 ** 31:
        raise TooLarge(stats)
    slot_src = np.concatenate([np.arange(cap * S, dtype=np.int32), np.repeat(sel.astype(np.int32), S)])
    child_out = np.concatenate([ch, np.zeros(K * S, np.int32)]).astype(np.int32)
    child_out[sel] = (cap + np.arange(K)) - sel // S
    rec = np.ascontiguousarray(data, np.float16).reshape(cap * S, D).view(np.uint16)
    data_out = rec[slot_src].view(np.float16)
    shp = (cap_out,) + child.shape[1:]
    return child_out.reshape(shp), data_out.reshape(shp + (D,)), slot_src.reshape(shp), stats


def assert_same(got, want, where=""):
    """got / want: (child, data, slot_src, stats)"""
    assert {k: got[3][k] for k in STAT_KEYS} == {k: want[3][k] for k in STAT_KEYS}, (where, got[3], want[3])
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (where, got[0].shape, want[0].shape)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), where + ": child differs"
    g, w = np.ascontiguousarray(got[1]).view(np.uint16), np.ascontiguousarray(want[1]).view(np.uint16)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d halves of data differ, first at %s" % (where, len(bad), bad[0].tolist())
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), where + ": slot_src differs"


# ---------------------------------------------------------------- trees
def one_node(D=4):
    """a root of eight different leaves"""
    data = (np.arange(8 * D, dtype=np.float32) * 0.5 - 3.0).astype(np.float16)
    return np.zeros((1, 2, 2, 2), np.int32), data.reshape(1, 2, 2, 2, D)


def chain31(D=4):
    """levels 0 .. 31: node k refers to node k + 1; the leaves of node k hold records that name k"""
    child, data = SR.chain_tree(31, D=D)
    data = data.copy()
    data += np.arange(32, dtype=np.float32).astype(np.float16).reshape(32, 1, 1, 1, 1)
    return child, data


# name -> (child, data): the simplifier's trees (D = 4, 5, 13, 28; N = 2 and 4; negative offsets; garbage nodes) and two more
TREES = {name: (lambda name=name: SR.CASES[name]()[:2]) for name in (
    "sh4_depth3_lossless", "sh4_depth6_lossless", "rgba_depth5_lossless", "sh9_depth4_kill50", "sh4_depth5_shuffled_lossless",
    "sh4_depth4_garbage", "sh4_depth5_shuffled_garbage_kill50", "chain_of_five", "uniform_root", "root_made_uniform", "n4",
    "special_densities_kill0")}
TREES["one_node"] = one_node
TREES["chain31"] = chain31


@functools.lru_cache(maxsize=None)
def tree(name):
    child, data = TREES[name]()
    child, data = np.ascontiguousarray(child, np.int32), np.ascontiguousarray(data, np.float16)
    child.setflags(write=False)
    data.setflags(write=False)
    return child, data


def density_keys(data, thresh=0.0):
    """the model of keys_from_density, written apart from it"""
    sigma = np.ascontiguousarray(np.asarray(data)[..., -1]).astype(np.float32)
    out = sigma.view(np.uint32).copy()
    out[~(sigma > np.float32(thresh))] = 0  # (a NaN compares false)
    return out


def random_keys(shape, seed, kind):
    """uint32 keys per slot: "few" = four values, "low" / "high" = keys that differ in the lowest / highest byte only, "wide" =
    any 32 bits"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "few":
        k = np.array([3, 0x3F000000, 0x3F000001, 0xFFFFFFFF], np.uint32)[rng.integers(0, 4, n)]
    elif kind == "low":
        k = np.uint32(0x3E99A500) + rng.integers(0, 256, n).astype(np.uint32)
    elif kind == "high":
        k = (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00C0FFEE)
    elif kind == "wide":
        k = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    else:
        raise KeyError(kind)
    return k.reshape(shape)


# name -> (tree, key builder (child, data) -> key or None, key_thresh, max_new, max_level): what the twin and the kernels are held to
def _k(kind, seed=1):
    return lambda child, data: random_keys(child.shape, seed, kind)


_density = lambda child, data: density_keys(data)  # noqa: E731
_mask = lambda child, data: None  # noqa: E731
CASES = {
    "sh4_depth3_mask": ("sh4_depth3_lossless", _mask, 1, -1, 31),
    "sh4_depth6_mask": ("sh4_depth6_lossless", _mask, 1, -1, 31),
    "sh4_depth6_density_budget": ("sh4_depth6_lossless", _density, 1, 700, 31),
    "sh4_depth6_few_budget1000": ("sh4_depth6_lossless", _k("few"), 1, 1000, 31),
    "sh4_depth6_wide_budget": ("sh4_depth6_lossless", _k("wide"), 1, 2500, 31),
    "sh4_depth6_wide_thresh": ("sh4_depth6_lossless", _k("wide", 2), 0xC0000000, -1, 31),
    "sh4_depth6_low_byte": ("sh4_depth6_lossless", _k("low"), 1, 3000, 31),
    "sh4_depth6_high_byte": ("sh4_depth6_lossless", _k("high"), 1, 3000, 31),
    "sh4_depth6_max_level5": ("sh4_depth6_lossless", _k("wide", 3), 1, -1, 5),
    "rgba_depth5_density": ("rgba_depth5_lossless", _density, 1, -1, 31),
    "rgba_depth5_few_budget": ("rgba_depth5_lossless", _k("few", 4), 1, 777, 31),
    "sh9_depth4_wide_budget": ("sh9_depth4_kill50", _k("wide", 5), 1, 300, 31),      # D = 28
    "shuffled_wide_budget": ("sh4_depth5_shuffled_lossless", _k("wide", 6), 1, 1500, 31),  # negative offsets
    "garbage_mask": ("sh4_depth4_garbage", _mask, 1, -1, 31),                         # unreachable nodes stay, never split
    "shuffled_garbage_few": ("sh4_depth5_shuffled_garbage_kill50", _k("few", 7), 1, 400, 31),
    "chain_of_five_mask": ("chain_of_five", _mask, 1, -1, 31),                        # D = 13
    "chain_of_five_budget": ("chain_of_five", _k("wide", 8), 1, 11, 31),
    "uniform_root_mask": ("uniform_root", _mask, 1, -1, 31),
    "root_made_uniform_one": ("root_made_uniform", _mask, 1, 1, 31),                  # D = 5
    "n4_mask": ("n4", _mask, 1, -1, 31),
    "n4_wide_budget": ("n4", _k("wide", 9), 1, 100, 31),
    "special_densities": ("special_densities_kill0", _density, 1, 200, 31),
    "one_node_mask": ("one_node", _mask, 1, -1, 31),
    "one_node_none": ("one_node", _mask, 2, -1, 31),                                  # key_thresh above every key: a copy
    "chain31_mask": ("chain31", _mask, 1, -1, 31),                                    # the leaves of level 31 are no candidates
    "chain31_max_level7": ("chain31", _mask, 1, -1, 7),
    "key_thresh_zero_takes_zero_keys": ("sh4_depth3_lossless", lambda c, d: (random_keys(c.shape, 10, "few") == 3).astype(np.uint32) * 5, 0, -1, 31),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(child, data, key, key_thresh, max_new, max_level, want) with want = the model's result, computed once"""
    tname, kf, thresh, max_new, max_level = CASES[name]
    child, data = tree(tname)
    key = kf(child, data)
    want = refine(child, data, key, thresh, max_new, max_level)
    for a in want[:3]:
        a.setflags(write=False)
    if key is not None:
        key.setflags(write=False)
    return child, data, key, thresh, max_new, max_level, want


def candidates_of(child, key=None, key_thresh=1, max_level=31):
    """the candidate slots, ascending, and their keys"""
    child = np.asarray(child)
    S = child.shape[1] ** 3
    lv = np.repeat(levels_of(child), S)
    keys = np.ones(child.size, np.uint32) if key is None else np.asarray(key).reshape(-1).view(np.uint32)
    cand = np.flatnonzero((child.reshape(-1) == 0) & (lv >= 0) & (lv + 1 <= max_level) & (keys >= np.uint32(key_thresh)))
    return cand, keys[cand]
