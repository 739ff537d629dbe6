"""Helpers of tests/test_depth.py: the depth outputs' expectation, reconstructed from the unchanged CPU oracle.

orc_trace_ray returns no distances, but it takes tmax_bg: for a fixed ray and RNG its alpha as a function of t_max = T is a step
function.  Hit k of the ray (include/rto.h "depth outputs") is present exactly when fl(T / delta_scale) > t_k, and its step has
height cnt_k / SPP.  Bisecting the bit pattern of T between the smallest positive normal float and 1e9f (the value a ray
without t_max gets) finds every step: its boundary b_k -- the least float T that keeps the hit -- and its height.  Alpha that
is non-zero already at the smallest T is a hit at distance 0."""
import functools

import numpy as np

import orc
from test_rays import _mixed_rays, _small, ray_oracle

f32 = np.float32
T_LO = int(np.array([np.finfo(f32).tiny], f32).view(np.uint32)[0])  # the smallest positive normal float
T_HI = int(np.array([1e9], f32).view(np.uint32)[0])
N_RAYS = 1000  # (a partial workgroup of 256)


def _flt(bits):
    return np.array([bits], np.uint32).view(f32)[0]


def reconstruct(ht, origins, dirs, spp, ndc=None, first_ray=0):
    """-> (hits, calls): hits[i] = [(b_k, cnt_k), ...] of ray i in hit order, b in float64 (0.0: a hit at distance 0), from the
    oracle's alpha alone; calls = the number of oracle calls spent"""
    n = origins.shape[0]
    calls = [0]

    def alpha(i, bits):
        calls[0] += 1
        return float(ray_oracle(ht, origins[i:i + 1], dirs[i:i + 1], spp, t_max=np.array([_flt(bits)], f32), first_ray=first_ray + i,
                                ndc=ndc)[0, 3])

    def count(a_lo, a_hi):
        c = (a_hi - a_lo) * spp
        k = int(round(c))
        assert k >= 1 and abs(c - k) < 1e-3, ("a step of the oracle's alpha is no multiple of 1 / SPP", a_lo, a_hi, spp)
        return k

    def steps(i, lo, hi, a_lo, a_hi, out):
        if a_lo == a_hi:
            return
        if hi - lo == 1:
            out.append((float(_flt(hi)), count(a_lo, a_hi)))
            return
        mid = (lo + hi) // 2
        a_mid = alpha(i, mid)
        steps(i, lo, mid, a_lo, a_mid, out)
        steps(i, mid, hi, a_mid, a_hi, out)

    hits = []
    for i in range(n):
        a_lo, a_hi = alpha(i, T_LO), alpha(i, T_HI)
        out = []
        if a_lo > 0:
            out.append((0.0, count(0.0, a_lo)))
        steps(i, T_LO, T_HI, a_lo, a_hi, out)
        hits.append(out)
    return hits, calls[0]


def expectation(hits, spp):
    """-> (depth [n], t_near [n]) in float64: sum_k (cnt_k / SPP) * b_k and b_0 (+inf without a hit)"""
    depth = np.array([sum(c / spp * b for b, c in h) for h in hits], np.float64)
    t_near = np.array([h[0][0] if h else np.inf for h in hits], np.float64)
    return depth, t_near


def alpha_of(hits, spp):
    return np.array([sum(c for _, c in h) for h in hits], np.float64) / spp


@functools.lru_cache(maxsize=None)
def scene():
    """the tree of the ray tests (depth 6, SH9, seed 7) and N_RAYS of test_rays' 4000 mixed rays: 700 of those that start inside
    the box (they are the ones that meet density often, some at distance 0) and every tenth of the others -- origins anywhere,
    axis-aligned / zero-component directions, rays that graze the faces"""
    t = _small()
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    o, d = _mixed_rays(t, 4000, seed=1)
    idx = np.concatenate([np.arange(0, 700), np.arange(1000, 4000, 10)])
    assert idx.size == N_RAYS
    return t, ht, np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])


@functools.lru_cache(maxsize=None)
def reference(spp):
    """the reconstruction of scene()'s rays at this SPP, computed once per session and shared: (hits, depth, t_near, calls)"""
    _, ht, o, d = scene()
    hits, calls = reconstruct(ht, o, d, spp)
    depth, t_near = expectation(hits, spp)
    return hits, depth, t_near, calls


def check_inputs(hits, spp):
    """the conditions on the inputs, from the reconstruction alone: a test on these rays cannot pass on empty ones.  (A ray
    with one sample has one hit at most: the share of rays with two or more distinct hits is asked for above SPP 1.)"""
    with_hit = [h for h in hits if h]
    assert len(with_hit) >= 100, len(with_hit)
    if spp > 1:
        assert 4 * sum(1 for h in with_hit if len(h) >= 2) >= len(with_hit), (sum(1 for h in with_hit if len(h) >= 2), len(with_hit))
    assert any(h[0][0] == 0.0 for h in with_hit)


def ulp(x):
    """the float32 ulp at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(f32)).astype(np.float64)
