"""Two reference statements of the tree fit (include/rto.h "tree fit").

(a) restate(): both marches and the fixed-point sums restated in numpy float32, bit for bit, in the style of
    leaf_weights_ref.restate -- every operation an IEEE float32 operation rounded once, the double sub-expressions (entry into
    the volume, SH basis, det_expf) in float64, the descent through the oracle's orc_query.  The rays of a camera advance
    together, one march step per pass; the sums are integers, so nothing depends on their order.  sgd_step() restates the step.
(b) model64(): the float64 composited image built from expected_render (ray_segments, view_basis: the model whose
    expected_frame IS the composited image) written with torch float64 tensors, and its gradient by torch.autograd.

Neither reads the product library."""
import ctypes as C

import numpy as np

import expected_render as ER
import leaf_weights_ref as LR
import orc

F = np.float32
D64 = np.float64
FIX = 2.0 ** 36


def det_expf(x):
    """lm::det_expf (= orc_det_expf) on a float32 array, operation by operation in float64"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        xd = x.astype(D64)
        xs = np.where(np.isfinite(xd), np.clip(xd, -104.0, 89.0), 0.0)
        z = xs * 1.4426950408889634
        kd = (z + 6755399441055744.0) - 6755399441055744.0
        r = (xs - kd * 0.693147180558298016) - kd * 1.6465949582897082e-12
        p = np.full_like(r, 1.0 / 39916800.0)
        for c in (1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5,
                  1.0, 1.0):
            p = p * r + c
        out = (p * np.ldexp(1.0, kd.astype(np.int64))).astype(np.float32)
    out = np.where(x > F(88.72283935546875), F(np.inf), out)
    out = np.where(x < F(-103.97208404541016), F(0), out)
    return np.where(np.isnan(x), x, out).astype(np.float32)


def sh_basis32(B, d):
    """sh_basis (lumisphere.hpp:38-80) for unit vectors d [3][n] float32 -> [B][n] float32: double literals, the products with
    them in float64, one rounding per assignment"""
    x, y, z = d[0], d[1], d[2]
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    d_ = lambda a: a.astype(D64)  # noqa: E731
    f_ = lambda a: a.astype(np.float32)  # noqa: E731
    out = [None] * 25
    out[0] = np.full_like(x, F(0.28209479177387814))
    out[1] = f_(-0.4886025119029199 * d_(y))
    out[2] = f_(0.4886025119029199 * d_(z))
    out[3] = f_(-0.4886025119029199 * d_(x))
    out[4] = f_(1.0925484305920792 * d_(xy))
    out[5] = f_(-1.0925484305920792 * d_(yz))
    out[6] = f_(0.31539156525252005 * ((2.0 * d_(zz) - d_(xx)) - d_(yy)))
    out[7] = f_(-1.0925484305920792 * d_(xz))
    out[8] = f_(0.5462742152960396 * d_(xx - yy))
    out[9] = f_(-0.5900435899266435 * d_(y) * d_(F(3) * xx - yy))
    out[10] = f_(2.890611442640554 * d_(xy) * d_(z))
    out[11] = f_(-0.4570457994644658 * d_(y) * d_((F(4) * zz - xx) - yy))
    out[12] = f_(0.3731763325901154 * d_(z) * d_((F(2) * zz - F(3) * xx) - F(3) * yy))
    out[13] = f_(-0.4570457994644658 * d_(x) * d_((F(4) * zz - xx) - yy))
    out[14] = f_(1.445305721320277 * d_(z) * d_(xx - yy))
    out[15] = f_(-0.5900435899266435 * d_(x) * d_(xx - F(3) * yy))
    out[16] = f_(2.5033429417967046 * d_(xy) * d_(xx - yy))
    out[17] = f_(-1.7701307697799304 * d_(yz) * d_(F(3) * xx - yy))
    out[18] = f_(0.9461746957575601 * d_(xy) * d_(F(7) * zz - F(1)))
    out[19] = f_(-0.6690465435572892 * d_(yz) * d_(F(7) * zz - F(3)))
    out[20] = f_(0.10578554691520431 * d_(zz * (F(35) * zz - F(30)) + F(3)))
    out[21] = f_(-0.6690465435572892 * d_(xz) * d_(F(7) * zz - F(3)))
    out[22] = f_(0.47308734787878004 * d_(xx - yy) * d_(F(7) * zz - F(1)))
    out[23] = f_(-1.7701307697799304 * d_(xz) * d_(xx - F(3) * yy))
    out[24] = f_(0.6258357354491761 * d_(xx * (xx - F(3) * yy) - yy * (F(3) * xx - yy)))
    return np.stack(out[:B]).astype(np.float32)


def to_fixed(g):
    """float32 array -> int64: 0 for a NaN, clamped to +-2^16, times 2^36, to nearest even"""
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(g), F(0), np.clip(g, F(-65536), F(65536)))
        return np.rint(c.astype(D64) * FIX).astype(np.int64)


def sgd_step(params, grad, lr):
    """-> the stepped params (float32): g = (float)((double)q * 2^-36), p - lr * g with two float roundings"""
    g = (grad.astype(D64) * (1.0 / FIX)).astype(np.float32)
    return (params - F(lr) * g).astype(np.float32)


def _colour(B, p, Y):
    """p [k][D] float32, Y [B][k] -> c [k][3]"""
    if B == 0:
        return p[:, :3].copy()
    c = np.empty((p.shape[0], 3), np.float32)
    for ch in range(3):
        z = Y[0] * p[:, ch * B]
        for k in range(1, B):
            z = z + Y[k] * p[:, ch * B + k]
        c[:, ch] = F(1) / (F(1) + det_expf(-z))
    return c


def restate(ht, params, cams, targets=None, want_grad=True, step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2,
            render_bbox=(0, 0, 0, 1, 1, 1), bg=1.0, ndc=None, grad=None, stats=None):
    """ht: an orc.HostTree (the support); params float32 [capacity,N,N,N,D]; cams: objects with width, height, fx, fy,
    transform; targets: per camera float32 [H,W,3] or None -> (images, grad int64 like params or None, stats int64 [2]);
    grad / stats given are accumulated into"""
    L = orc.lib()
    N = ht.N
    n_slots = ht.capacity * N ** 3
    Dd = params.shape[-1]
    B = 0 if ht.data_format.upper().startswith("RGBA") else (Dd - 1) // 3
    P = np.ascontiguousarray(params, np.float32).reshape(n_slots, Dd)
    sig16 = ht.data.reshape(n_slots, -1)[:, -1].view(np.float16)
    if want_grad and grad is None:
        grad = np.zeros(params.shape, np.int64)
    gflat = grad.reshape(-1) if want_grad else None
    stats = np.zeros(2, np.int64) if stats is None else stats
    step_size, sigma_thresh, stop_thresh, bg = F(step_size), F(sigma_thresh), F(stop_thresh), F(bg)
    bbox = LR._f(render_bbox)
    sc = LR._f(ht.scale)
    xyz = (C.c_float * 3)()
    cube = C.c_float()
    images = []
    with np.errstate(all="ignore"):
        for f, cam in enumerate(cams):
            d, c = LR.camera_rays32(cam, ht.scale, ht.offset, ndc)
            vdir = LR.camera_rays32(cam, ht.scale, ht.offset, None)[0]
            n = d.shape[1]
            tg = None if targets is None else np.asarray(targets[f], np.float32).reshape(n, 3)
            unmasked = np.ones(n, bool) if tg is None else ~np.isnan(tg).any(1)
            ok = np.isfinite(d).all(0) & np.isfinite(c).all(0)
            Y = sh_basis32(B, vdir) if B else None
            d = np.stack([d[i] * sc[i] for i in range(3)])
            ds = F(1.0) / LR._norm3(d)
            d = np.stack([d[i] * ds for i in range(3)])
            tmax_bg = F(1e9) / ds
            invd = (1.0 / (d.astype(D64) + 1e-9)).astype(np.float32)
            tmin = np.zeros_like(ds)
            tmax = np.full_like(ds, F(1e4))
            for i in range(3):
                t1 = (((D64(bbox[i]) + 1e-6) - c[i].astype(D64)) * invd[i].astype(D64)).astype(np.float32)
                t2 = (((D64(bbox[i + 3]) - 1e-6) - c[i].astype(D64)) * invd[i].astype(D64)).astype(np.float32)
                tmin = LR._fmax(tmin, LR._fmin(t1, t2))
                tmax = LR._fmin(tmax, LR._fmax(t1, t2))
            tmax = LR._fmin(tmax, tmax_bg)
            ok &= ~((tmax < 0) | (tmin > tmax))

            def march(out, res):
                """out None: the forward march -> (acc, T); else the backward march, adding into gflat"""
                T = np.ones_like(ds)
                acc = np.zeros((n, 3), np.float32)
                t = tmin.copy()
                live = np.nonzero(ok & unmasked & (t < tmax))[0]
                while live.size:
                    pos = c[:, live] + t[live] * d[:, live]
                    k = live.size
                    slot = np.empty(k, np.int64)
                    cs = np.empty(k, np.float32)
                    local = np.empty((3, k), np.float32)
                    for j in range(k):
                        xyz[0], xyz[1], xyz[2] = pos[0, j], pos[1, j], pos[2, j]
                        slot[j] = L.orc_query(C.byref(ht.c), xyz, C.byref(cube), None)
                        cs[j] = cube.value
                        local[0, j], local[1, j], local[2, j] = xyz[0], xyz[1], xyz[2]
                    tm = np.full(k, F(1e4))
                    for i in range(3):
                        t1 = -local[i] * invd[i, live]
                        t2 = t1 + invd[i, live]
                        tm = LR._fmin(tm, LR._fmax(t1, t2))
                    dt = tm / cs + step_size
                    p = P[slot]
                    sigma = p[:, Dd - 1]
                    dense = (sig16[slot].astype(np.float32) > sigma_thresh) & (sigma > sigma_thresh)
                    delta = dt * ds[live]
                    e = np.where(dense, det_expf(-(delta * sigma)), F(1))
                    att = np.where(e < F(1), e, F(1)).astype(np.float32)
                    Tl = T[live]
                    w = Tl * (F(1) - att)
                    col = _colour(B, p, None if Y is None else Y[:, live])
                    acc_new = acc[live] + w[:, None] * col
                    acc[live] = np.where(dense[:, None], acc_new, acc[live])
                    if out is not None and dense.any():
                        dn = np.nonzero(dense)[0]
                        rl, a_after = res[live][dn], acc[live][dn]
                        Ta = (Tl * att)[dn]
                        x = Ta[:, None] * col[dn] - (out[live][dn] - a_after)
                        s = rl[:, 0] * x[:, 0]
                        s = s + rl[:, 1] * x[:, 1]
                        s = s + rl[:, 2] * x[:, 2]
                        base = slot[dn] * Dd
                        np.add.at(gflat, base + (Dd - 1), to_fixed(delta[dn] * s))
                        gc = rl * w[dn, None]
                        if B == 0:
                            for ch in range(3):
                                np.add.at(gflat, base + ch, to_fixed(gc[:, ch]))
                        else:
                            cd = col[dn]
                            gz = gc * (cd * (F(1) - cd))
                            Yl = Y[:, live][:, dn]
                            for ch in range(3):
                                for kk in range(B):
                                    np.add.at(gflat, base + ch * B + kk, to_fixed(gz[:, ch] * Yl[kk]))
                    Tn = np.where(dense, Tl * att, Tl).astype(np.float32)
                    T[live] = Tn
                    stop = dense & (Tn < stop_thresh)
                    tn = t[live] + dt
                    adv = tn > t[live]
                    t[live] = np.where(adv, tn, t[live])
                    live = live[~stop & adv & (tn < tmax[live])]
                return acc, T

            acc, T = march(None, None)
            out = (acc + (T * bg)[:, None]).astype(np.float32)
            images.append(np.where(unmasked[:, None], out, F(0)).reshape(int(cam.height), int(cam.width), 3))
            if tg is None:
                continue
            res = (out - tg).astype(np.float32)
            loss = (res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + res[:, 2] * res[:, 2]
            stats[0] += to_fixed(loss)[unmasked].sum()
            stats[1] += int(unmasked.sum())
            if want_grad:
                march(out, res)
    return images, grad, stats


# ------------------------------------------------------------------ the float64 model
class Model64:
    """The composited images of a SynthTree (N = 2) over poses in torch float64, differentiable with respect to the leaf values
    `values` [capacity * 8, D]: the rays' segments come once from expected_render.ray_segments (the support: the tree's own
    densities), the field from `values`."""

    def __init__(self, tree, poses, W, H, fx, fy, step_size=1e-4, sigma_thresh=1e-2, render_bbox=(0, 0, 0, 1, 1, 1), bg=1.0, ndc=None):
        import torch
        self.torch = torch
        self.scene = ER.Scene.of(tree)
        self.W, self.H, self.n = W, H, len(poses)
        self.bg, self.sigma_thresh = bg, sigma_thresh
        self.rays = []  # per ray: (slots int64 [m], lengths float64 [m], Y float64 [B] or None)
        for c2w in poses:
            for y in range(H):
                for x in range(W):
                    o, dw = ER.pinhole_ray(c2w, W, H, fx, fy, x, y)
                    Y = ER.view_basis(self.scene, dw)
                    if ndc is not None:
                        o, dw = ER.ndc_warp(o, dw, ndc)
                    segs = ER.ray_segments(self.scene, o, dw, step_size=step_size, sigma_thresh=sigma_thresh, bbox=render_bbox)
                    slots = torch.tensor([nd * 8 + ci for nd, ci, _, _ in segs], dtype=torch.int64)
                    lens = torch.tensor([ln for _, _, ln, _ in segs], dtype=torch.float64)
                    self.rays.append((slots, lens, None if Y is None else torch.tensor(Y, dtype=torch.float64)))

    def values_of(self, params):
        return self.torch.tensor(np.asarray(params, np.float64).reshape(self.scene.child.size, -1), dtype=self.torch.float64)

    def images(self, values):
        """values: torch float64 [capacity * 8, D] -> [n, H, W, 3]"""
        torch = self.torch
        B = self.scene.basis_dim
        outs = []
        for slots, lens, Y in self.rays:
            if slots.numel() == 0:
                outs.append(torch.full((3,), self.bg, dtype=torch.float64))
                continue
            v = values[slots]
            sigma = v[:, -1]
            keep = (sigma > self.sigma_thresh).to(torch.float64)  # the second test of the support, a constant of the gradient
            att = torch.exp(-(sigma * lens) * keep)
            Tc = torch.cumprod(att, 0)
            T = torch.cat([torch.ones(1, dtype=torch.float64), Tc[:-1]])
            w = T * (1.0 - att)
            col = v[:, :3] if self.scene.rgba else torch.sigmoid(v[:, :3 * B].reshape(-1, 3, B) @ Y)
            outs.append((w[:, None] * col).sum(0) + Tc[-1] * self.bg)
        return torch.stack(outs).reshape(self.n, self.H, self.W, 3)

    def loss(self, values, targets):
        """1/2 sum |out - target|^2 over the pixels whose target holds no NaN"""
        torch = self.torch
        tg = torch.tensor(np.asarray(targets, np.float64))
        mask = ~torch.isnan(tg).any(-1, keepdim=True)
        r = torch.where(mask, self.images(values) - torch.nan_to_num(tg), torch.zeros((), dtype=torch.float64))
        return 0.5 * (r * r).sum()

    def grad(self, params, targets):
        """-> (images float64 [n,H,W,3], gradient float64 with the shape of params)"""
        v = self.values_of(params).requires_grad_(True)
        loss = self.loss(v, targets)
        loss.backward()
        with self.torch.no_grad():
            img = self.images(v).numpy()
        return img, v.grad.numpy().reshape(np.asarray(params).shape)
