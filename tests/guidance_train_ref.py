"""The GuidanceNet under training as a model in torch on the CPU, parametrised by dtype: forward, backward given ReLU6 masks, and
the forward error bound of a float32 evaluation.  tests/test_guidance_train.py holds the HIP training kernels to it.

    z_l = conv3x3(x_{l-1}, W_l, zero padding) + b_l,   x_l = min(max(z_l, 0), 6)
    weight_map = softmax(x_N[:levels]),  guidance_map = x_N[levels:]

Error bound of float32 arithmetic with float32 accumulation, per element and layer (tau_0 = 0):
    A_l   = conv(|x_{l-1}|, |W_l|) + |b_l|
    tau_l = 2 (9 cin_l + 1) 2^-24 A_l + conv(tau_{l-1}, |W_l|)
(9 cin + 1 roundings of relative size 2^-24 on partial sums bounded by A_l, with a factor 2 for their second-order terms and the
order of summation; the clamp is 1-Lipschitz, so the bound holds for x_l too.)  An activation is DECIDED when its float64 z lies
farther than tau from both 0 and 6: every correct float32 evaluation then agrees on its ReLU6 mask."""
import numpy as np
import torch
import torch.nn.functional as F


def make_net(c1, levels, layers, seed=1, scale=3.0):
    """GuidanceNet(8, c1, 5, layers, levels) under torch.manual_seed(seed); its effective float32 kernels and biases x scale"""
    from rt_octree_amd import denoiser
    torch.manual_seed(seed)
    model = denoiser.GuidanceNet(8, c1, 5, layers, levels)
    with torch.no_grad():
        return [((w * scale).contiguous(), (b * scale).contiguous()) for w, b in denoiser.effective_layers(model)]


def make_aux(n, H, W, seed=1):
    """uniform [0, 1) r, g, b, a with their squares as planes 4..7"""
    rgba = np.random.RandomState(seed).rand(n, 4, H, W).astype(np.float32)
    return torch.from_numpy(np.concatenate([rgba, rgba * rgba], 1))


def forward(aux, layers, levels, dtype=torch.float64):
    """-> dict(z = [z_l], x = [x_l], weight_map, guidance_map)"""
    x, zs, xs = aux.to(dtype), [], []
    for w, b in layers:
        z = F.conv2d(x, w.to(dtype), b.to(dtype), padding=1)
        x = z.clamp(0, 6)
        zs.append(z)
        xs.append(x)
    return {"z": zs, "x": xs, "weight_map": F.softmax(x[:, :levels], 1), "guidance_map": x[:, levels:]}


def masks_of(xs):
    """torch's hardtanh_backward rule from post-activation values"""
    return [(x > 0) & (x < 6) for x in xs]


def backward(aux, layers, levels, masks, grad_wm, grad_gm, dtype=torch.float64):
    """[(dW_l, db_l)] with the given ReLU6 masks; activations are the model's own in `dtype`"""
    fw = forward(aux, layers, levels, dtype)
    xs = [aux.to(dtype)] + fw["x"]
    w = fw["weight_map"]
    g = grad_wm.to(dtype)
    dx = torch.cat([w * (g - (g * w).sum(1, keepdim=True)), grad_gm.to(dtype)], 1)
    out = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        dz = dx * masks[l].to(dtype)
        W = layers[l][0].to(dtype)
        out[l] = (torch.nn.grad.conv2d_weight(xs[l], W.shape, dz, padding=1), dz.sum((0, 2, 3)))
        if l:
            dx = torch.nn.grad.conv2d_input(xs[l].shape, W, dz, padding=1)
    return out


def forward_bound(aux, layers, levels):
    """[tau_l], float64, from the float64 activations"""
    fw = forward(aux, layers, levels, torch.float64)
    xs = [aux.double()] + fw["x"]
    tau, out = torch.zeros_like(xs[0]), []
    for l, (w, b) in enumerate(layers):
        aw = w.double().abs()
        A = F.conv2d(xs[l].abs(), aw, b.double().abs(), padding=1)
        tau = 2 * (9 * w.shape[1] + 1) * 2.0 ** -24 * A + F.conv2d(tau, aw, None, padding=1)
        out.append(tau)
    return out


def decided(zs, taus):
    return [((z.abs() > t) & ((z - 6).abs() > t)) for z, t in zip(zs, taus)]


# ---- the loss (denoiser/metrics.py:7-9) and its gradient, float64 numpy
def loss_and_grad(pred, truth, kind):
    p, t = pred[..., :3].astype(np.float64), truth[..., :3].astype(np.float64)
    d = p - t
    if kind == "mse":
        terms, g = d * d, 2 * d
    else:
        D = np.abs(p) + np.abs(t) + 1e-5
        terms = np.abs(d) / D
        g = np.sign(d) / D - np.abs(d) * np.sign(p) / (D * D)
    grad = np.zeros(pred.shape, np.float64)
    grad[..., :3] = g / terms.size
    return terms.sum() / terms.size, grad
