"""The GuidanceNet under training on the device (csrc/guidance_train_kernels.hip; include/rto.h "GuidanceNet under training"):
effective layers, forward with saved activations, backward, the loss -- against the model of tests/guidance_train_ref.py.

The forward is held to the float32 error bound of the model (tau, per element).  The gradients are held to
16 e32 + 2^-20 max|g64|, where e32 is the largest difference between the model run in float32 and in float64 on the same masks:
the margin of 16 is for a summation order and an exponential that differ from torch's; a missing tap, a wrong edge or a dropped
tile moves a gradient by whole terms, orders of magnitude above it.  e32 is printed for every tensor."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guidance_train_ref as G

NETS = [(32, 4, 2), (5, 1, 2), (8, 4, 2), (1, 6, 2), (64, 1, 2), (20, 2, 3), (64, 6, 3)]
CASES = [net + (2, 19, 23) for net in NETS] + [(32, 4, 2, 3, 40, 70)]


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("c1,levels,layers", [(8, 4, 2), (20, 2, 3), (5, 1, 2)])  # identity in the last block; three layers; none
def test_effective_layers_equal_the_full_model_float64(c1, levels, layers):
    from rt_octree_amd import denoiser
    torch.manual_seed(3)
    model = denoiser.GuidanceNet(8, c1, 5, layers, levels).double()
    has_identity = [b.in_channels == b.out_channels for b in model.layers]
    assert any(has_identity) == ((c1, levels, layers) != (5, 1, 2))
    aux = G.make_aux(2, 11, 13, seed=5).double()
    up_w, up_g = torch.randn(2, levels, 11, 13, dtype=torch.float64), torch.randn(2, levels, 11, 13, dtype=torch.float64)

    feat = model.features(aux)  # every branch, float64 (on the CPU the model does not autocast; its split() would round to float32)
    wm, gm = F.softmax(feat[:, :levels], 1), feat[:, levels:]
    (wm * up_w).sum().add((gm * up_g).sum()).backward()
    full = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()

    eff = denoiser.effective_layers(model)
    fw = G.forward(aux, eff, levels)
    assert float((fw["weight_map"] - wm).detach().abs().max()) <= 1e-12 and float((fw["guidance_map"] - gm).detach().abs().max()) <= 1e-12
    (fw["weight_map"] * up_w).sum().add((fw["guidance_map"] * up_g).sum()).backward()
    for p, ref in zip(model.parameters(), full):
        assert p.grad is not None
        assert float((p.grad - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))
    # and in float32 the sums are those of the compact module, bit for bit (from_full accumulates in float32)
    model = model.float()
    compact = denoiser.GuidanceNetCompact.from_full(model)
    for (w, b), blk in zip(denoiser.effective_layers(model), compact.layers):
        assert torch.equal(w.detach(), blk.conv.weight) and torch.equal(b.detach(), blk.conv.bias)


def test_model_backward_equals_autograd_float64():
    layers = [(w.double(), b.double()) for w, b in G.make_net(20, 2, 3)]
    aux = G.make_aux(2, 9, 10).double()
    params = [t.clone().requires_grad_(True) for wb in layers for t in wb]
    x = aux
    for l in range(3):
        z = F.conv2d(x, params[2 * l], params[2 * l + 1], padding=1)
        assert float(torch.minimum(z.abs(), (z - 6).abs()).min().detach()) > 1e-9
        x = F.relu6(z)
    gw, gg = torch.randn(2, 2, 9, 10, dtype=torch.float64), torch.randn(2, 2, 9, 10, dtype=torch.float64)
    (F.softmax(x[:, :2], 1) * gw).sum().add((x[:, 2:] * gg).sum()).backward()
    fw = G.forward(aux, layers, 2)
    ours = G.backward(aux, layers, 2, G.masks_of(fw["x"]), gw, gg)
    for l in range(3):
        for mine, ref in zip(ours[l], (params[2 * l].grad, params[2 * l + 1].grad)):
            assert float((mine - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("kind", ["smape", "mse"])
def test_loss_gradient_formula_equals_autograd_float64(kind):
    rs = np.random.RandomState(4)
    pred, truth = rs.randn(2, 5, 7, 4).astype(np.float32), rs.randn(2, 5, 7, 4).astype(np.float32)
    pred[0, 0, :3] = truth[0, 0, :3]  # p == t
    pred[0, 1, :2] = truth[0, 1, :2] = 0  # p == t == 0
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(truth, dtype=torch.float64)
    d = p[..., :3] - t[..., :3]
    loss = (d.abs() / (p[..., :3].abs() + t[..., :3].abs() + 1e-5)).mean() if kind == "smape" else (d ** 2).mean()
    loss.backward()
    ref_loss, ref_grad = G.loss_and_grad(pred, truth, kind)
    assert abs(ref_loss - float(loss)) <= 1e-14 * abs(float(loss))
    # (the two terms of the SMAPE derivative cancel where p and t have opposite signs: a few digits of the 16 go)
    assert np.allclose(ref_grad, p.grad.numpy(), rtol=1e-9, atol=1e-18)
    assert np.all(ref_grad[0, 0, :3] == 0) and np.all(ref_grad[0, 1, :2] == 0) and np.all(ref_grad[..., 3] == 0)


# ---------------------------------------------------------------- GPU helpers
class Net:
    """one case's inputs on the device and the raw ABI calls"""

    def __init__(self, c1, levels, layers, n, H, W):
        from rt_octree_amd import _lib
        self.levels, self.n, self.H, self.W = levels, n, H, W
        self.host_layers = G.make_net(c1, levels, layers)
        self.host_aux = G.make_aux(n, H, W)
        self.dev = [(w.cuda(), b.cuda()) for w, b in self.host_layers]
        self.aux = self.host_aux.cuda()
        self.grads = [(torch.full_like(w, 7.0), torch.full_like(b, 7.0)) for w, b in self.dev]  # (overwritten, not accumulated)
        self.c_layers = (_lib.CGuidanceTrainLayer * layers)()
        for c, (w, b), (gw, gb) in zip(self.c_layers, self.dev, self.grads):
            c.weight, c.bias, c.grad_weight, c.grad_bias = w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr()
            c.cin, c.cout = w.shape[1], w.shape[0]
        self.h = C.c_void_p(0)
        _lib.check(_lib.lib().rto_guidance_train_create(0, C.byref(self.h)))

    def acts_floats(self):
        from rt_octree_amd import _lib
        nbytes = C.c_size_t(0)
        _lib.check(_lib.lib().rto_guidance_train_acts_bytes(self.c_layers, len(self.dev), self.levels, self.n, self.H, self.W, C.byref(nbytes)))
        assert nbytes.value == 4 * self.n * self.H * self.W * sum(w.shape[0] for w, _ in self.dev)
        return nbytes.value // 4

    def forward(self, aux=None):
        from rt_octree_amd import _lib
        aux = self.aux if aux is None else aux
        acts = torch.empty(self.acts_floats(), device="cuda")
        wm = torch.empty((self.n, self.levels, self.H, self.W), device="cuda")
        gm = torch.empty_like(wm)
        _lib.check(_lib.lib().rto_guidance_train_forward(self.h, None, aux.data_ptr(), self.c_layers, len(self.dev), self.levels, self.n,
                                                         self.H, self.W, acts.data_ptr(), wm.data_ptr(), gm.data_ptr()))
        return acts, wm, gm

    def split(self, acts):
        out, o = [], 0
        for w, _ in self.dev:
            k = self.n * w.shape[0] * self.H * self.W
            out.append(acts[o:o + k].reshape(self.n, w.shape[0], self.H, self.W))
            o += k
        return out

    def backward(self, acts, gw, gg, aux=None):
        from rt_octree_amd import _lib
        aux = self.aux if aux is None else aux
        _lib.check(_lib.lib().rto_guidance_train_backward(self.h, None, gw.data_ptr(), gg.data_ptr(), aux.data_ptr(), acts.data_ptr(),
                                                          self.c_layers, len(self.dev), self.levels, self.n, self.H, self.W))
        torch.cuda.synchronize()
        return [(a.cpu().clone(), b.cpu().clone()) for a, b in self.grads]

    def close(self):
        from rt_octree_amd import _lib
        torch.cuda.synchronize()
        _lib.lib().rto_guidance_train_free(self.h)


def _upstream(net, seed=2):
    rs = np.random.RandomState(seed)
    shape = (net.n, net.levels, net.H, net.W)
    return torch.from_numpy(rs.randn(*shape).astype(np.float32)), torch.from_numpy(rs.randn(*shape).astype(np.float32))


# ---------------------------------------------------------------- GPU: forward and backward against the model
@pytest.mark.gpu
@pytest.mark.parametrize("c1,levels,layers,n,H,W", CASES)
def test_forward_and_backward_against_the_model(c1, levels, layers, n, H, W):
    net = Net(c1, levels, layers, n, H, W)
    try:
        fw = G.forward(net.host_aux, net.host_layers, levels)
        taus = G.forward_bound(net.host_aux, net.host_layers, levels)
        dec = G.decided(fw["z"], taus)
        # preconditions, on the float64 model (met by every net at seed 1)
        for l, x in enumerate(fw["x"]):
            assert float((x == 0).double().mean()) >= 1e-3 and float((x == 6).double().mean()) >= 1e-3, "layer %d does not saturate" % l
        undecided = sum(int((~d).sum()) for d in dec) / sum(d.numel() for d in dec)
        assert undecided <= 0.02

        acts, wm, gm = net.forward()
        torch.cuda.synchronize()
        xs = [a.cpu() for a in net.split(acts)]
        for l, (x, ref, tau) in enumerate(zip(xs, fw["x"], taus)):
            err = (x.double() - ref).abs()
            print("layer %d: max |x - x64| %.3e, max tau %.3e" % (l, float(err.max()), float(tau.max())))
            assert bool((err <= tau).all()), "layer %d activations leave the float32 bound" % l
        assert bool(((gm.cpu().double() - fw["guidance_map"]).abs() <= taus[-1][:, levels:]).all())
        assert torch.equal(gm.cpu(), xs[-1][:, levels:])
        wtol = 2 * taus[-1][:, :levels].max(1, keepdim=True)[0] + 2.0 ** -20
        assert bool(((wm.cpu().double() - fw["weight_map"]).abs() <= wtol).all())
        masks = G.masks_of(xs)
        for l, (m, ref, d) in enumerate(zip(masks, G.masks_of(fw["x"]), dec)):
            assert bool((m == ref)[d].all()), "layer %d: a decided activation has the wrong ReLU6 mask" % l

        gw, gg = _upstream(net)
        ours = net.backward(acts, gw.cuda(), gg.cuda())
        g64 = G.backward(net.host_aux, net.host_layers, levels, masks, gw, gg, torch.float64)
        g32 = G.backward(net.host_aux, net.host_layers, levels, masks, gw, gg, torch.float32)
        for l in range(layers):
            for name, mine, r64, r32 in zip(("dW", "db"), ours[l], g64[l], g32[l]):
                e32 = float((r32.double() - r64).abs().max())
                err = float((mine.double() - r64).abs().max())
                scale = float(r64.abs().max())
                print("%s_%d: e32 %.3e, kernel error %.3e, max |g64| %.3e" % (name, l, e32, err, scale))
                assert err <= 16 * e32 + 2.0 ** -20 * scale, "%s_%d" % (name, l)
    finally:
        net.close()


# ---------------------------------------------------------------- GPU: further checks
@pytest.mark.gpu
@pytest.mark.parametrize("c1,levels,layers", [(32, 4, 2), (20, 2, 3)])
def test_same_bits_every_run_and_in_any_order(c1, levels, layers):
    net = Net(c1, levels, layers, 3, 40, 70)
    try:
        aux_b = G.make_aux(3, 40, 70, seed=9).cuda()
        ga, gb = [t.cuda() for t in _upstream(net, 2)], [t.cuda() for t in _upstream(net, 3)]

        def alone(aux, g):
            acts, wm, gm = net.forward(aux)
            return [t.cpu().clone() for t in (acts, wm, gm)] + [t for wb in net.backward(acts, g[0], g[1], aux) for t in wb]

        a1, a2, b1 = alone(net.aux, ga), alone(net.aux, ga), alone(aux_b, gb)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a1, a2)), "two runs differ"
        # forward A, forward B, backward B, backward A
        fa, fb = net.forward(net.aux), net.forward(aux_b)
        gB = [t for wb in net.backward(fb[0], gb[0], gb[1], aux_b) for t in wb]
        gA = [t for wb in net.backward(fa[0], ga[0], ga[1], net.aux) for t in wb]
        mixed_a = [t.cpu() for t in fa] + gA
        mixed_b = [t.cpu() for t in fb] + gB
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a1, mixed_a))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b1, mixed_b))
    finally:
        net.close()


@pytest.mark.gpu
def test_refusals_return_their_codes_and_leave_outputs_untouched():
    from rt_octree_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -3
    net = Net(8, 4, 2, 1, 8, 8)
    try:
        acts = torch.full((net.acts_floats(),), 5.0, device="cuda")
        wm = torch.full((1, 4, 8, 8), 5.0, device="cuda")
        gm = torch.full_like(wm, 5.0)
        up = torch.ones_like(wm)

        def layers_of(chain):
            arr = (_lib.CGuidanceTrainLayer * len(chain))()
            keep = []
            for c, (cin, cout) in zip(arr, chain):
                w, b = torch.zeros(cout, cin, 3, 3, device="cuda"), torch.zeros(cout, device="cuda")
                gw, gb = torch.full_like(w, 5.0), torch.full_like(b, 5.0)
                keep += [w, b, gw, gb]
                c.weight, c.bias, c.grad_weight, c.grad_bias, c.cin, c.cout = w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr(), cin, cout
            return arr, keep

        def fwd(arr, nl, levels, n=1, H=8, W=8, aux=None, h=None):
            return L.rto_guidance_train_forward(net.h if h is None else h, None, net.aux.data_ptr() if aux is None else aux, arr, nl, levels,
                                                n, H, W, acts.data_ptr(), wm.data_ptr(), gm.data_ptr())

        def bwd(arr, nl, levels, n=1, H=8, W=8):
            return L.rto_guidance_train_backward(net.h, None, up.data_ptr(), up.data_ptr(), net.aux.data_ptr(), acts.data_ptr(), arr, nl,
                                                 levels, n, H, W)

        good, keep_good = layers_of([(8, 8), (8, 8)])
        assert fwd(good, 2, 4, aux=C.c_void_p(0)) == INVALID and fwd(None, 2, 4) == INVALID
        assert fwd(good, 2, 4, n=0) == INVALID and fwd(good, 2, 4, H=0) == INVALID and fwd(good, 2, 4, W=-1) == INVALID
        assert fwd(good, 1, 4) == INVALID and fwd(good, 4, 4) == INVALID
        assert b"num_layers" in L.rto_last_error()
        for chain in ([(7, 8), (8, 8)], [(8, 8), (9, 8)], [(8, 8), (8, 6)]):  # does not link up (twice); last cout != 2 levels
            arr, _keep = layers_of(chain)
            assert fwd(arr, 2, 4) == INVALID and bwd(arr, 2, 4) == INVALID
        for chain in ([(8, 65), (65, 8)], [(8, 8), (8, 14)], [(8, 8), (8, 16), (16, 8)]):  # c1 65; levels 7; middle not c1 -> c1
            arr, _keep = layers_of(chain)
            lv = chain[-1][1] // 2
            assert fwd(arr, len(chain), lv) == UNSUPPORTED and bwd(arr, len(chain), lv) == UNSUPPORTED
        nograd, _k = layers_of([(8, 8), (8, 8)])
        nograd[1].grad_bias = None
        assert bwd(nograd, 2, 4) == INVALID
        nbytes = C.c_size_t(123)
        assert L.rto_guidance_train_acts_bytes(good, 5, 4, 1, 8, 8, C.byref(nbytes)) == INVALID and nbytes.value == 123
        loss = torch.full((), 5.0, dtype=torch.float64, device="cuda")
        img = torch.zeros(1, 8, 8, 4, device="cuda")
        grad = torch.full_like(img, 5.0)
        assert L.rto_loss_forward_backward(net.h, None, img.data_ptr(), img.data_ptr(), 1, 8, 8, 2, loss.data_ptr(), grad.data_ptr()) == INVALID
        assert L.rto_loss_forward_backward(net.h, None, img.data_ptr(), img.data_ptr(), 1, 0, 8, 0, loss.data_ptr(), grad.data_ptr()) == INVALID
        assert L.rto_loss_forward_backward(net.h, None, img.data_ptr(), None, 1, 8, 8, 0, loss.data_ptr(), grad.data_ptr()) == INVALID
        assert L.rto_loss_forward_backward(net.h, None, img.data_ptr() + 4, img.data_ptr(), 1, 4, 4, 0, loss.data_ptr(), grad.data_ptr()) == INVALID
        torch.cuda.synchronize()
        assert float(loss) == 5.0 and bool((grad == 5).all())
        assert bool((gm == 5).all()) and bool((wm == 5).all()) and bool((acts == 5).all())
        for t in keep_good[2::4] + keep_good[3::4]:
            assert bool((t == 5).all())
        assert fwd(nograd, 2, 4) == 0  # (the forward does not read the gradient pointers)
    finally:
        net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["smape", "mse"])
def test_image_loss_on_the_device(kind):
    from rt_octree_amd import denoiser
    rs = np.random.RandomState(6)
    pred, truth = rs.rand(2, 19, 23, 4).astype(np.float32), rs.rand(2, 19, 23, 4).astype(np.float32)
    pred[:, ::3, ::2, :3] *= -1  # both signs of p
    pred[0, 3, 4:9] = truth[0, 3, 4:9]  # p == t
    pred[1, 5, 5, :3] = truth[1, 5, 5, :3] = 0  # p == t == 0
    ref_loss, ref_grad = G.loss_and_grad(pred, truth, kind)
    p = torch.tensor(pred, device="cuda", requires_grad=True)
    loss = denoiser.image_loss(p, torch.tensor(truth, device="cuda"), kind)
    loss.backward()
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - ref_loss) <= 1e-10 * abs(ref_loss)
    g = p.grad.cpu().numpy()
    r32 = ref_grad.astype(np.float32)
    ulp = np.spacing(np.abs(r32))
    assert np.all(np.abs(g.astype(np.float64) - r32.astype(np.float64)) <= ulp)
    assert np.all(g[0, 3, 4:9] == 0) and np.all(g[1, 5, 5] == 0) and np.all(g[..., 3] == 0)
    bad = pred.copy()
    bad[1, 2, 3, 1] = np.nan
    q = torch.tensor(bad, device="cuda", requires_grad=True)
    loss = denoiser.image_loss(q, torch.tensor(truth, device="cuda"), kind)
    loss.backward()
    assert np.isnan(float(loss)) and np.isnan(float(q.grad[1, 2, 3, 1])) and bool(torch.isfinite(q.grad[0]).all())
    with pytest.raises(NotImplementedError):
        denoiser.image_loss(p, p, "lpips_alex")


@pytest.mark.gpu
def test_fused_filtering_end_to_end_and_a_short_training():
    from rt_octree_amd import denoiser
    torch.manual_seed(1)
    model = denoiser.GuidanceNet(8, 32, 5, 2, 4).cuda()
    aux = G.make_aux(2, 40, 40, seed=3).cuda()
    img = aux[:, :4].permute(0, 2, 3, 1).contiguous()
    truth = torch.tensor(np.random.RandomState(8).rand(2, 40, 40, 4).astype(np.float32), device="cuda") * 0.5 + 0.25 * img
    out = denoiser.filtering(model, aux, img, requires_grad=True, fused=True)
    with torch.no_grad():  # the unfused model in float32, without autocast
        wm, gm = model.split(model.features(aux))
        ref = denoiser.filtering_autograd(wm, gm, img)
    assert float((out - ref).abs().max()) <= 1e-5
    denoiser.image_loss(out, truth).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert sum(float(p.grad.abs().sum()) for p in model.parameters()) > 0
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        loss = denoiser.image_loss(denoiser.filtering(model, aux, img, requires_grad=True, fused=True), truth)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("loss %.5f -> %.5f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
