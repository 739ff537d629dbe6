"""The numpy float32 restatement of the tree fit on rays the caller supplies (include/rto.h "tree fit", rto_tree_fit_grad_rays):
ray_begin_ray of csrc/rto_fit_march.h restated operation by operation -- normalize3 of the direction, the NDC warp, offset +
scale * cen -- and after it the entry and the two marches of fit_ref.restate, whose helpers (det_expf, sh_basis32, to_fixed,
_colour) are imported.  The rays advance together, one march step per pass; the sums are integers.  Does not read the product
library."""
import ctypes as C

import numpy as np

import fit_ref as FR
import leaf_weights_ref as LR
import orc

F = np.float32
D64 = np.float64


def ray_setup32(origins, dirs, scale, offset, ndc=None):
    """ray_begin_ray's set-up for rays [n][3] float32 -> (dir [3][n], cen [3][n], vdir [3][n]) float32 in tree space"""
    d = [np.asarray(dirs, np.float32)[:, i].copy() for i in range(3)]
    c = [np.asarray(origins, np.float32)[:, i].copy() for i in range(3)]
    inv = F(1.0) / LR._norm3(d)
    d = [d[i] * inv for i in range(3)]
    vdir = np.stack(d).astype(np.float32)
    if ndc is not None and ndc[0] > 0:
        nw, nh, nf = F(ndc[0]), F(ndc[1]), F(ndc[2])
        t = -(F(1.0) + c[2]) / d[2]
        c = [c[i] + t * d[i] for i in range(3)]
        ax, ay = (F(2) * nf) / nw, (F(2) * nf) / nh
        d0 = -ax * (d[0] / d[2] - c[0] / c[2])
        d1 = -ay * (d[1] / d[2] - c[1] / c[2])
        d2 = F(-2) / c[2]
        c0 = -ax * (c[0] / c[2])
        c1 = -ay * (c[1] / c[2])
        c2 = F(1) + F(2) / c[2]
        d, c = [d0, d1, d2], [c0, c1, c2]
        inv = F(1.0) / LR._norm3(d)
        d = [d[i] * inv for i in range(3)]
    sc, of = LR._f(scale), LR._f(offset)
    c = [of[i] + sc[i] * c[i] for i in range(3)]
    return np.stack(d).astype(np.float32), np.stack(c).astype(np.float32), vdir


def restate(ht, params, origins, dirs, targets=None, want_grad=True, step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2,
            render_bbox=(0, 0, 0, 1, 1, 1), bg=1.0, ndc=None, grad=None, stats=None, out=None):
    """ht: an orc.HostTree (the support); params float32 [capacity,N,N,N,D]; origins, dirs, targets float32 [n,3] (targets may be
    None) -> (out float32 [n,3], grad int64 like params or None, stats int64 [2]); grad / stats given are accumulated into; `out`
    given keeps the rows of masked rays"""
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
    n = int(np.asarray(origins).shape[0])
    out = np.zeros((n, 3), np.float32) if out is None else out
    with np.errstate(all="ignore"):
        d, c, vdir = ray_setup32(origins, dirs, ht.scale, ht.offset, ndc)
        tg = None if targets is None else np.asarray(targets, np.float32).reshape(n, 3)
        unmasked = np.ones(n, bool) if tg is None else ~np.isnan(tg).any(1)
        ok = np.isfinite(d).all(0) & np.isfinite(c).all(0)
        Y = FR.sh_basis32(B, vdir) if B else None
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

        def march(col_out, res):
            """col_out None: the forward march -> (acc, T); else the backward march, adding into gflat"""
            T = np.ones(n, np.float32)
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
                e = np.where(dense, FR.det_expf(-(delta * sigma)), F(1))
                att = np.where(e < F(1), e, F(1)).astype(np.float32)
                Tl = T[live]
                w = Tl * (F(1) - att)
                col = FR._colour(B, p, None if Y is None else Y[:, live])
                acc_new = acc[live] + w[:, None] * col
                acc[live] = np.where(dense[:, None], acc_new, acc[live])
                if col_out is not None and dense.any():
                    dn = np.nonzero(dense)[0]
                    rl, a_after = res[live][dn], acc[live][dn]
                    Ta = (Tl * att)[dn]
                    x = Ta[:, None] * col[dn] - (col_out[live][dn] - a_after)
                    s = rl[:, 0] * x[:, 0]
                    s = s + rl[:, 1] * x[:, 1]
                    s = s + rl[:, 2] * x[:, 2]
                    base = slot[dn] * Dd
                    np.add.at(gflat, base + (Dd - 1), FR.to_fixed(delta[dn] * s))
                    gc = rl * w[dn, None]
                    if B == 0:
                        for ch in range(3):
                            np.add.at(gflat, base + ch, FR.to_fixed(gc[:, ch]))
                    else:
                        cd = col[dn]
                        gz = gc * (cd * (F(1) - cd))
                        Yl = Y[:, live][:, dn]
                        for ch in range(3):
                            for kk in range(B):
                                np.add.at(gflat, base + ch * B + kk, FR.to_fixed(gz[:, ch] * Yl[kk]))
                Tn = np.where(dense, Tl * att, Tl).astype(np.float32)
                T[live] = Tn
                stop = dense & (Tn < stop_thresh)
                tn = t[live] + dt
                adv = tn > t[live]
                t[live] = np.where(adv, tn, t[live])
                live = live[~stop & adv & (tn < tmax[live])]
            return acc, T

        acc, T = march(None, None)
        colour = (acc + (T * bg)[:, None]).astype(np.float32)
        out[unmasked] = colour[unmasked]
        if tg is not None:
            res = (colour - tg).astype(np.float32)
            loss = (res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + res[:, 2] * res[:, 2]
            stats[0] += FR.to_fixed(loss)[unmasked].sum()
            stats[1] += int(unmasked.sum())
            if want_grad:
                march(colour, res)
    return out, grad, stats
