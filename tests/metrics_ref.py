"""The model the metric kernels are held to (include/rto.h "image metrics"), in numpy.

Formats and the background composite are float32, operation by operation; everything after is float64.  The window comes from
np.exp in float64; the separable passes run along H, then along W, each a sum over the 11 taps in tap order.  The formulas are
restated from denoiser/metrics.py:7-9 (SMAPE), :61-62 (PSNR), :78-79 (SSIM = pytorch_msssim.ssim(X, Y, data_range=1)) and
denoiser/dataset.py:76,82-84 (8-bit conversion, white background)."""
import numpy as np

C1, C2 = 1e-4, 9e-4  # (0.01 * data_range)^2, (0.03 * data_range)^2


def window():
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    return g / g.sum()


def to_float32(img):
    """[...,4] uint8 or float32 -> float32 as the kernels convert it"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255.0)
    assert img.dtype == np.float32
    return img


def composite(truth, bg):
    """rgb * a + bg * (1 - a) in float32, every product and sum rounded"""
    t = to_float32(truth).copy()
    a = t[..., 3:4]
    t[..., :3] = t[..., :3] * a + np.float32(bg) * (np.float32(1.0) - a)
    assert t.dtype == np.float32
    return t


def _filter(x, g):
    """[H,W] float64 -> [H-10,W-10]: along H, then along W, taps added in order"""
    H, W = x.shape
    v = np.zeros((H - 10, W), np.float64)
    for k in range(11):
        v += g[k] * x[k:k + H - 10]
    o = np.zeros((H - 10, W - 10), np.float64)
    for k in range(11):
        o += g[k] * v[:, k:k + W - 10]
    return o


def ssim(p, t):
    """p, t: [H,W,>=3] float32 -> float64 scalar; NaN when the image is smaller than the window"""
    H, W = p.shape[:2]
    if H < 11 or W < 11:
        return float("nan")
    g = window()
    means = []
    for c in range(3):
        x, y = p[..., c].astype(np.float64), t[..., c].astype(np.float64)
        mx, my = _filter(x, g), _filter(y, g)
        vxx = _filter(x * x, g) - mx * mx
        vyy = _filter(y * y, g) - my * my
        vxy = _filter(x * y, g) - mx * my
        m = (2.0 * (mx * my) + C1) / (mx * mx + my * my + C1) * ((2.0 * vxy + C2) / (vxx + vyy + C2))
        means.append(m.mean())
    return float(np.mean(means))


def frame_metrics(pred, truth, over_background=None):
    """one frame, [H,W,4] each, uint8 or float32 -> dict(mse, psnr, smape, ssim) of float64"""
    p = to_float32(pred)
    t = composite(truth, over_background) if over_background is not None else to_float32(truth)
    if not (np.isfinite(p[..., :3]).all() and np.isfinite(t[..., :3]).all()):
        nan = float("nan")
        return {"mse": nan, "psnr": nan, "smape": nan, "ssim": nan}
    pd, td = p[..., :3].astype(np.float64), t[..., :3].astype(np.float64)
    d = pd - td
    mse = float((d * d).mean())
    with np.errstate(divide="ignore"):
        psnr = float(-10.0 * np.log10(mse))
    smape = float((np.abs(d) / (np.abs(pd) + np.abs(td) + 1e-5)).mean())
    return {"mse": mse, "psnr": psnr, "smape": smape, "ssim": ssim(p, t)}


def batch_metrics(pred, truth, over_background=None):
    return [frame_metrics(pred[i], truth[i], over_background) for i in range(len(pred))]


def assert_close(got, want, where=""):
    """the tolerances of the issue: ssim absolute 1e-9, mse and smape relative 1e-10, psnr absolute 1e-9 dB; NaN and inf
    must match as such"""
    for name, tol, rel in (("mse", 1e-10, True), ("psnr", 1e-9, False), ("smape", 1e-10, True), ("ssim", 1e-9, False)):
        g, w = float(getattr(got, name)), float(want[name])
        print("%s %s: got %.17g model %.17g" % (where, name, g, w))
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (where, name, g, w)
        else:
            assert abs(g - w) <= (tol * abs(w) if rel else tol), (where, name, g, w, abs(g - w))
