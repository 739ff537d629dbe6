"""Two reference statements of the per-leaf peak weights (include/rto.h "leaf weights").

(a) restate(): the definition restated in numpy float32, bit for bit -- every operation an IEEE float32 operation rounded
    once (numpy's elementwise +, -, *, /, sqrt on float32 arrays), the double sub-expressions of the entry into the volume in
    float64, the descent through the oracle's orc_query, the exponential through orc_det_expf.  The rays of a camera advance
    together, one march step per pass; nothing depends on their order (the update is a max).
(b) model64(): a float64 model built from expected_render.ray_segments, the suite's own statement of which leaves a ray
    crosses and for how long: p_j = T_j (1 - exp(-tau_j)), the peak per (node, child), the ray stops when T < stop_thresh.

Neither reads the product library."""
import ctypes as C

import numpy as np

import expected_render as ER
import orc

F = np.float32


def _f(v):
    return np.asarray(v, np.float32)


def _norm3(d):
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def _fmin(a, b):
    return np.where(a < b, a, b)


def _fmax(a, b):
    return np.where(a > b, a, b)


def camera_rays32(cam, scale, offset, ndc=None):
    """ray_setup for every pixel of `cam` (an object with width, height, fx, fy and transform, 12 floats column-major):
    (dir [3][n], cen [3][n]) float32 in tree space, row-major pixels"""
    W, H = int(cam.width), int(cam.height)
    m = _f(np.asarray(cam.transform, np.float32).reshape(-1))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = xs.reshape(-1).astype(np.float32)
    y = ys.reshape(-1).astype(np.float32)
    v0 = (x - F(0.5) * F(W)) / F(cam.fx)
    v1 = -(y - F(0.5) * F(H)) / F(cam.fy)
    v2 = np.full_like(v0, F(-1.0))
    d = [(m[0 + i] * v0 + m[3 + i] * v1) + m[6 + i] * v2 for i in range(3)]
    inv = F(1.0) / _norm3(d)
    d = [d[i] * inv for i in range(3)]
    c = [np.full_like(v0, m[9 + i]) for i in range(3)]
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
        inv = F(1.0) / _norm3(d)
        d = [d[i] * inv for i in range(3)]
    sc, of = _f(scale), _f(offset)
    c = [of[i] + sc[i] * c[i] for i in range(3)]
    return np.stack(d).astype(np.float32), np.stack(c).astype(np.float32)


def restate(ht, cams, step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2, render_bbox=(0, 0, 0, 1, 1, 1), ndc=None, out=None):
    """ht: an orc.HostTree; cams: objects with width, height, fx, fy, transform -> float32 [capacity, N, N, N]"""
    L = orc.lib()
    N = ht.N
    n_slots = ht.capacity * N ** 3
    sig16 = ht.data.reshape(n_slots, -1)[:, -1].view(np.float16)
    bits = np.zeros(n_slots, np.uint32) if out is None else out.reshape(-1).view(np.uint32)
    step_size, sigma_thresh, stop_thresh = F(step_size), F(sigma_thresh), F(stop_thresh)
    bbox = _f(render_bbox)
    sc = _f(ht.scale)
    xyz = (C.c_float * 3)()
    cube = C.c_float()
    with np.errstate(all="ignore"):
        for cam in cams:
            d, c = camera_rays32(cam, ht.scale, ht.offset, ndc)
            ok = np.isfinite(d).all(0) & np.isfinite(c).all(0)
            # ray_enter
            d = np.stack([d[i] * sc[i] for i in range(3)])
            ds = F(1.0) / _norm3(d)
            d = np.stack([d[i] * ds for i in range(3)])
            tmax_bg = F(1e9) / ds
            invd = (1.0 / (d.astype(np.float64) + 1e-9)).astype(np.float32)
            tmin = np.zeros_like(ds)
            tmax = np.full_like(ds, F(1e4))
            for i in range(3):
                t1 = (((np.float64(bbox[i]) + 1e-6) - c[i].astype(np.float64)) * invd[i].astype(np.float64)).astype(np.float32)
                t2 = (((np.float64(bbox[i + 3]) - 1e-6) - c[i].astype(np.float64)) * invd[i].astype(np.float64)).astype(np.float32)
                tmin = _fmax(tmin, _fmin(t1, t2))
                tmax = _fmin(tmax, _fmax(t1, t2))
            tmax = _fmin(tmax, tmax_bg)
            ok &= ~((tmax < 0) | (tmin > tmax))
            T = np.ones_like(ds)
            t = tmin.copy()
            live = np.nonzero(ok & (t < tmax))[0]
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
                    tm = _fmin(tm, _fmax(t1, t2))
                dt = tm / cs + step_size
                sigma = sig16[slot].astype(np.float32)
                dense = sigma > sigma_thresh
                arg = -((dt * ds[live]) * sigma)
                e = np.ones(k, np.float32)
                for j in np.nonzero(dense)[0]:
                    e[j] = L.orc_det_expf(float(arg[j]))
                att = np.where(e < F(1), e, F(1)).astype(np.float32)
                w = T[live] * (F(1) - att)
                np.maximum.at(bits, slot[dense], w[dense].view(np.uint32))
                Tn = np.where(dense, T[live] * att, T[live]).astype(np.float32)
                T[live] = Tn
                stop = dense & (Tn < stop_thresh)
                tn = t[live] + dt
                adv = tn > t[live]
                t[live] = np.where(adv, tn, t[live])
                go = ~stop & adv & (tn < tmax[live])
                live = live[go]
    return bits.view(np.float32).reshape(ht.capacity, N, N, N)


def model64(tree, poses, W, H, fx, fy, step_size=1e-4, sigma_thresh=1e-2, stop_thresh=1e-2, render_bbox=(0, 0, 0, 1, 1, 1)):
    """tree: a SynthTree (N = 2); poses: row-major c2w matrices -> float64 [capacity, 2, 2, 2]: per leaf the largest
    T_j (1 - exp(-tau_j)) over the pixels' rays, tau_j = sigma * world length (expected_render.ray_segments)"""
    scene = ER.Scene.of(tree)
    peak = np.zeros((scene.child.shape[0], 8))
    for c2w in poses:
        for y in range(H):
            for x in range(W):
                o, dw = ER.pinhole_ray(c2w, W, H, fx, fy, x, y)
                T = 1.0
                for node, ci, length, sigma in ER.ray_segments(scene, o, dw, step_size=step_size, sigma_thresh=sigma_thresh, bbox=render_bbox):
                    a = np.exp(-sigma * length)
                    p = T * (1.0 - a)
                    if p > peak[node, ci]:
                        peak[node, ci] = p
                    T *= a
                    if T < stop_thresh:
                        break
    return peak.reshape(-1, 2, 2, 2)
