"""numpy model of the median-cut quantiser as include/rto.h "quantiser" defines it (one lexsort((row, key, box)) per round,
int64 sums), the inputs the host and GPU tests share, and the numpy builder of the file compress_octree must write."""
import functools

import numpy as np


def keys_of(rows):
    h = np.ascontiguousarray(rows, np.float16).view(np.uint16).astype(np.uint32)
    return np.where(h & 0x8000, ~h & 0xFFFF, h | 0x8000).astype(np.uint32)


def _values_of_keys(k):
    h = np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16)
    return h.view(np.float16).astype(np.float32)


def fixed_of(rows):
    """every fp16 value in units of 2^-24, an exact int64"""
    h = np.ascontiguousarray(rows, np.float16).view(np.uint16).astype(np.int64)
    e, f = (h >> 10) & 31, h & 1023
    mag = np.where(e > 0, (1024 + f) << np.maximum(e - 1, 0), f)
    return np.where(h & 0x8000, -mag, mag)


def median_cut(rows, bits):
    """rows float16 [m, 3] -> (palette float16 [2^bits, 3], ids uint16 [m])"""
    rows = np.ascontiguousarray(rows, np.float16)
    m = rows.shape[0]
    assert m >= 1 and rows.shape == (m, 3) and 1 <= bits <= 16 and np.isfinite(rows.astype(np.float32)).all()
    key = keys_of(rows)
    row = np.arange(m, dtype=np.int64)
    box = np.zeros(m, np.int64)
    for level in range(bits):
        nb = 1 << level
        cnt = np.bincount(box, minlength=nb)
        first = np.cumsum(cnt) - cnt
        by_box = np.argsort(box, kind="stable")
        full = np.flatnonzero(cnt)
        lo = np.zeros((nb, 3), np.uint32)
        hi = np.zeros((nb, 3), np.uint32)
        lo[full] = np.minimum.reduceat(key[by_box], first[full], axis=0)
        hi[full] = np.maximum.reduceat(key[by_box], first[full], axis=0)
        extent = _values_of_keys(hi) - _values_of_keys(lo)  # one float32 subtraction
        assert extent.dtype == np.float32
        axis = np.argmax(extent, axis=1)  # the lowest axis among equals
        k = key[row, axis[box]]
        order = np.lexsort((row, k, box))
        sb = box[order]
        rank = np.arange(m, dtype=np.int64) - first[sb]
        upper = rank >= (cnt[sb] + 1) // 2
        nxt = np.empty_like(box)
        nxt[order] = 2 * sb + upper
        box = nxt
    nb = 1 << bits
    cnt = np.bincount(box, minlength=nb)
    S = np.zeros((nb, 3), np.int64)
    np.add.at(S, box, fixed_of(rows))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = S.astype(np.float64) / cnt.astype(np.float64)[:, None] * 2.0 ** -24
    mean[cnt == 0] = 0.0
    palette = mean.astype(np.float32).astype(np.float16)
    return palette, box.astype(np.uint16)


def _f16(a):
    return np.ascontiguousarray(a, dtype=np.float16)


FOUR_VALUES = np.array([-1.0, -0.0, 0.0, 0.25], np.float16)


def normal_rows(m, seed):
    return _f16(np.random.default_rng(seed).standard_normal((m, 3)))


def four_value_rows(m, seed):
    return _f16(FOUR_VALUES[np.random.default_rng(seed).integers(0, 4, (m, 3))])


def distinct_rows(m, seed):
    """distinct values on every axis: no ties anywhere"""
    rng = np.random.default_rng(seed)
    pool = np.arange(0x0400, 0x7BFF, dtype=np.uint16)  # the positive normal halves
    cols = []
    for c in range(3):
        h = rng.choice(pool, m, replace=False)
        sign = (rng.integers(0, 2, m) << 15).astype(np.uint16)
        cols.append(h | sign)
    # (a positive and a negative of one magnitude are different values)
    return np.stack(cols, 1).view(np.float16)


def extreme_rows(m, seed):
    """+-65504, subnormals and +-0 among ordinary values"""
    rng = np.random.default_rng(seed)
    special = np.array([0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000, 0x0400, 0x3C00], np.uint16)
    h = special[rng.integers(0, special.size, (m, 3))]
    plain = normal_rows(m, seed + 1).view(np.uint16)
    return np.where(rng.random((m, 3)) < 0.5, h, plain).astype(np.uint16).view(np.float16)


def constant_column_rows(m, seed):
    r = normal_rows(m, seed)
    r[:, 1] = np.float16(0.375)
    return r


# name -> (rows builder, bits): what the host twin and the kernels are both held to
CASES = {}
for _m in (1, 2, 3, 63, 64, 65, 257):
    CASES["normal_m%d" % _m] = (functools.partial(normal_rows, _m, 100 + _m), 16)
CASES["normal_m1000_bits1"] = (functools.partial(normal_rows, 1000, 7), 1)
CASES["normal_m1000_bits5"] = (functools.partial(normal_rows, 1000, 7), 5)
CASES["distinct_m4096"] = (functools.partial(distinct_rows, 4096, 11), 16)
CASES["identical_m70000"] = (lambda: _f16(np.tile(np.array([[0.5, -2.0, 3.25]]), (70000, 1))), 16)
CASES["constant_column_m5000"] = (functools.partial(constant_column_rows, 5000, 13), 16)
CASES["four_values_m5000"] = (functools.partial(four_value_rows, 5000, 17), 16)
CASES["extremes_m5000"] = (functools.partial(extreme_rows, 5000, 19), 16)
CASES["normal_m65537"] = (functools.partial(normal_rows, 65537, 23), 16)


@functools.lru_cache(maxsize=None)
def case(name):
    """(rows, bits, palette, ids) of the model, computed once"""
    build, bits = CASES[name]
    rows = build()
    pal, ids = median_cut(rows, bits)
    for a in (rows, pal, ids):
        a.setflags(write=False)
    return rows, bits, pal, ids


def assert_same(got_pal, got_ids, want_pal, want_ids, where=""):
    got_ids = np.asarray(got_ids).view(np.uint16)
    assert got_ids.shape == want_ids.shape, where
    bad = np.flatnonzero(got_ids != want_ids)
    assert bad.size == 0, "%s: %d ids differ, first at row %d: %d != %d" % (where, bad.size, bad[0], got_ids[bad[0]], want_ids[bad[0]])
    g, w = np.asarray(got_pal).view(np.uint16), np.asarray(want_pal).view(np.uint16)
    assert g.shape == w.shape, where
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d palette entries differ, first at %s: %#06x != %#06x" % (
        where, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


SVOX_KEYS = ("parent_depth", "geom_resize_fact", "n_free", "n_internal", "depth_limit")


def expected_file(z, bits=16, retain=1, sigma_thresh=2.0):
    """the arrays compress_octree must write for the dense tree arrays z (a dict), with this file's model as the quantiser"""
    out = {k: v for k, v in z.items() if k not in SVOX_KEYS and k != "data"}
    data = np.asarray(z["data"], np.float16)
    cap, N, D = data.shape[0], data.shape[1], data.shape[-1]
    B = (D - 1) // 3
    flat = data.reshape(-1, D)
    with np.errstate(over="ignore"):
        thresh = np.float32(sigma_thresh).astype(np.float16)  # torch: half tensor > python float compares in half
    live = flat[:, -1] > thresh
    out["sigma"] = np.where(live, flat[:, -1], np.float16(0)).astype(np.float16).reshape(cap, N, N, N)
    nq = B - retain
    colors = np.zeros((nq, 65536, 3), np.float16)
    qmap = np.zeros((nq, flat.shape[0]), np.uint16)
    for j in range(nq):
        k = j + retain
        tri = np.stack([flat[live, c * B + k] for c in range(3)], 1)
        if tri.shape[0]:
            pal, ids = median_cut(tri, bits)
            colors[j, :1 << bits] = pal
            qmap[j, live] = ids
    out["quant_colors"] = colors
    out["quant_map"] = qmap.reshape(nq, cap, N, N, N)
    if retain:
        kept = np.zeros((retain, flat.shape[0], 3), np.float16)
        for k in range(retain):
            for c in range(3):
                kept[k, live, c] = flat[live, c * B + k]
        out["data_retained"] = kept.reshape(retain, cap, N, N, N, 3)
    return out


def write_dense_tree(path, depth_limit=5, basis_dim=9, seed=5):
    """a synthetic SH tree as svox saves one: the loader's keys plus svox's five bookkeeping keys; -> the dict written"""
    from rt_octree_amd import synth
    t = synth.make_tree(depth_limit=depth_limit, basis_dim=basis_dim, seed=seed)
    z = dict(data_dim=np.int64(t.data_dim), data_format=np.array(t.data_format), invradius3=t.scale.astype(np.float32),
             offset=t.offset.astype(np.float32), child=t.child, data=t.data,
             parent_depth=np.zeros((t.capacity, 2), np.int32), geom_resize_fact=np.float64(1.0), n_free=np.int64(0),
             n_internal=np.int64(t.capacity), depth_limit=np.int64(depth_limit))
    np.savez(path, **z)
    return z


def decoded(q):
    """the dense data [capacity,N,N,N,data_dim] a loader expands the quantised arrays q to (n3tree.cpp:279-340)"""
    qm, qc, sg = q["quant_map"], q["quant_colors"], q["sigma"]
    nq, cap, N = qm.shape[0], qm.shape[1], qm.shape[2]
    rt = q["data_retained"] if "data_retained" in q else np.zeros((0, cap, N, N, N, 3), np.float16)
    nr = rt.shape[0]
    nb, slots = nq + nr, cap * N ** 3
    data = np.zeros((slots, 3 * nb + 1), np.float16)
    for j in range(nq):
        col = qc[j][qm[j].reshape(slots)]
        for c in range(3):
            data[:, (j + nr) + c * nb] = col[:, c]
    for j in range(nr):
        for c in range(3):
            data[:, j + c * nb] = rt[j].reshape(slots, 3)[:, c]
    data[:, 3 * nb] = sg.reshape(-1)
    return data.reshape(cap, N, N, N, 3 * nb + 1)


def fnv1a64(b):
    h = 1469598103934665603
    for x in np.frombuffer(b, np.uint8).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h
