"""The numpy float32 restatement of the sparse step of the tree fit (include/rto.h "tree fit": the touched bitmap, its list,
rto_fit_step_sparse).

touched: fit_rays_ref.restate with one more output.  Its backward march adds the density's contribution of every dense sample
with np.add.at(gflat, slot * D + (D - 1), .) -- the place where rto_fit_march.h calls add with k == D - 1 -- before the colour
contributions; restate_touched runs it with a numpy whose add.at also notes those indices, whether or not the fixed-point value
is zero.  The list is np.flatnonzero; the three step formulas are restated with explicit np.float32 temporaries, every
operation rounded once.  Does not read the product library."""
import numpy as np

import fit_rays_ref as RR
import fit_ref as FR

F = np.float32
D64 = np.float64
SGD, RMSPROP, ADAM = 0, 1, 2


class _NotingAdd:
    """numpy's add, whose .at also notes the indices congruent to D - 1 modulo D: the density's contributions"""

    def __init__(self, D, noted):
        self.D, self.noted = D, noted

    def at(self, a, idx, vals):
        idx = np.asarray(idx)
        dens = idx[idx % self.D == self.D - 1]
        self.noted.append(dens // self.D)
        np.add.at(a, idx, vals)

    def __call__(self, *a, **kw):
        return np.add(*a, **kw)


class _Numpy:
    """numpy with a noting add, for the time of one restate"""

    def __init__(self, add):
        self.add = add

    def __getattr__(self, name):
        return getattr(np, name)


def restate_touched(ht, params, origins, dirs, targets, touched=None, **kw):
    """fit_rays_ref.restate -> (out, grad, stats, touched): touched a bool array [slots], accumulated into when given"""
    slots = ht.capacity * ht.N ** 3
    noted = []
    saved = RR.np
    RR.np = _Numpy(_NotingAdd(params.shape[-1], noted))
    try:
        out, grad, stats = RR.restate(ht, params, origins, dirs, targets, **kw)
    finally:
        RR.np = saved
    touched = np.zeros(slots, bool) if touched is None else touched
    for s in noted:
        touched[s] = True
    return out, grad, stats, touched


def bitmap_of(touched):
    """bool [slots] -> uint32 [(slots + 31) // 32]: slot s is bit s & 31 of word s >> 5"""
    slots = touched.shape[0]
    words = np.zeros((slots + 31) // 32, np.uint32)
    s = np.flatnonzero(touched)
    np.bitwise_or.at(words, s >> 5, (np.uint32(1) << (s & 31).astype(np.uint32)).astype(np.uint32))
    return words


def bits_of(words, slots):
    """uint32 words -> bool [slots] (bits at or beyond slots are dropped)"""
    b = (words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)
    return b.reshape(-1)[:slots].astype(bool)


def list_of(words, slots):
    """the set slots in ascending order, uint32"""
    return np.flatnonzero(bits_of(words, slots)).astype(np.uint32)


def bias(beta, t):
    """the caller's float of step t: float32(1 - float32(beta)^t), the power and the difference in double"""
    return F(1.0 - float(F(beta)) ** int(t))


def step(kind, params, grad, lst, lr, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, t=1, m=None, v=None):
    """the step over the rows `lst` of params / grad / m / v (arrays [..., D], changed in place); every operation float32"""
    D = params.shape[-1]
    P, G = params.reshape(-1, D), grad.reshape(-1, D)
    lr, gs, b1, b2, eps = F(lr), F(grad_scale), F(beta1), F(beta2), F(eps)
    rows = np.asarray(lst, np.int64)
    rows = rows[rows < P.shape[0]]
    with np.errstate(all="ignore"):
        g = (G[rows].astype(D64) * (1.0 / FR.FIX)).astype(np.float32)
        g = (g * gs).astype(np.float32)
        G[rows] = 0
        p = P[rows]
        if kind == SGD:
            s = (lr * g).astype(np.float32)
            P[rows] = (p - s).astype(np.float32)
            return
        V = v.reshape(-1, D)
        if kind == ADAM:
            M = m.reshape(-1, D)
            a = (b1 * M[rows]).astype(np.float32)
            c1 = F(F(1) - b1)
            b = (c1 * g).astype(np.float32)
            mm = (a + b).astype(np.float32)
            M[rows] = mm
        a2 = (b2 * V[rows]).astype(np.float32)
        c2 = F(F(1) - b2)
        b2g = (c2 * g).astype(np.float32)
        b3 = (b2g * g).astype(np.float32)
        vv = (a2 + b3).astype(np.float32)
        V[rows] = vv
        if kind == ADAM:
            num = (mm / bias(beta1, t)).astype(np.float32)
            vh = (vv / bias(beta2, t)).astype(np.float32)
            root = np.sqrt(vh).astype(np.float32)
        else:
            num = g
            root = np.sqrt(vv).astype(np.float32)
        den = (root + eps).astype(np.float32)
        r = (num / den).astype(np.float32)
        s = (lr * r).astype(np.float32)
        P[rows] = (p - s).astype(np.float32)
