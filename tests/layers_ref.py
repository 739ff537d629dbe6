"""Helpers of tests/test_layers.py: the layer fixture and the layered expectation.

A layered frame (rto_ctx_set_layers) is defined through rto_launch_rays: pixel (x, y) is ray y * W + x of the camera's rays with
t_max = its depth and background = its colour's rgb.  The CPU expectation is therefore test_rays.ray_oracle -- orc_trace_ray plus
the numpy restatement pinned there to the pixel oracle -- on volrend.camera_rays."""
import numpy as np

import rt_octree_amd as R
from test_rays import ray_oracle

f32 = np.float32


def volume_centre(t):
    """world-space centre of the tree's volume (tree space (0.5, 0.5, 0.5))"""
    return ((0.5 - t.offset.astype(np.float64)) / t.scale.astype(np.float64))


def make_layers(t, cams):
    """depth [F, H, W] and colour [F, H, W, 4] float32 for the cameras of one context.  Depth: the distance along each pixel's
    unit ray to the plane through the volume centre that faces the camera (it cuts the object in half), pushed a little further
    per frame; rows 0..5 are +inf (no limit), rows 20..25 lie in front of the whole volume, and a sprinkle of 0, negative and NaN
    entries sits inside the object's silhouette and outside it.  Colour: a gradient that differs per channel and per frame;
    alpha holds a poison the kernels must not read."""
    F = len(cams)
    H, W = cams[0].height, cams[0].width
    depth = np.empty((F, H, W), f32)
    color = np.empty((F, H, W, 4), f32)
    c = volume_centre(t)
    for f, cam in enumerate(cams):
        o, d = R.camera_rays(cam)
        d = d.astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        m = np.asarray(cam.transform, np.float64)
        axis = -m[2]  # the viewing direction
        along = float(np.dot(c - m[3], axis))
        t_plane = (along * (1.0 + 0.02 * f)) / (d @ axis)
        dp = t_plane.reshape(H, W).astype(f32)
        dp[0:6, :] = np.inf
        dp[20:26, :] = f32(0.1 * along)  # (the volume starts at least half its diagonal before the centre: far behind this)
        yy, xx = np.mgrid[0:H, 0:W]
        k = (yy * 7 + xx * 13 + f) % 97
        dp[k == 0] = 0.0
        dp[k == 1] = -2.5
        dp[k == 2] = np.nan
        depth[f] = dp
        u, v = xx / f32(W - 1), yy / f32(H - 1)
        color[f, ..., 0] = 0.1 + 0.8 * u
        color[f, ..., 1] = 0.9 - 0.7 * v + 0.01 * f
        color[f, ..., 2] = 0.2 + 0.3 * u * v + 0.05 * f
        color[f, ..., 3] = -123.0
    return depth, color


def expected_rgba(ht, cam, spp, depth=None, color=None, rng_base=None, bg=1.0, ndc=None, **optkw):
    """[H * W, 4]: (r, g, b, alpha) of a layered frame, ray by ray on the CPU"""
    o, d = R.camera_rays(cam)
    tm = None if depth is None else np.ascontiguousarray(depth, f32).reshape(-1)
    back = None if color is None else np.ascontiguousarray(color, f32).reshape(-1, 4)[:, :3]
    return ray_oracle(ht, o, d, spp, t_max=tm, background=back, bg=bg, rng_base=rng_base, ndc=ndc, **optkw)


def frame_outputs(rgba, H, W):
    """the reference's frame outputs (volrend.cu:186-212) from [H * W, 4] (r, g, b, alpha): aux [8, H, W] = the values and their
    float32 squares, image [H, W, 4] = (r, g, b, 1)"""
    p = np.ascontiguousarray(rgba.T.reshape(4, H, W), f32)
    aux = np.concatenate([p, p * p], 0)
    image = np.concatenate([rgba[:, :3], np.ones((H * W, 1), f32)], 1).reshape(H, W, 4)
    return aux, image
