"""The sparse step of the tree fit on the host (include/rto.h "tree fit": rto_fit_grad_rays_touched_host,
rto_fit_touched_list_host, rto_fit_step_sparse_host; no GPU).  Bit for bit unless said: the marking twin's out, grad and stats
against the old twin's and its bitmap against the numpy restatement (tests/fit_sparse_ref.py) in every format, on an NDC and a
re-laid tree, in any order, split and thread count; the list on synthetic bitmaps; the SGD identity with rto_fit_sgd_step_host;
ten RMSProp and Adam steps against the restatement; their meaning against torch.optim in float64 (a bound); the refusals by
their texts; optimize_octree --optimizer / --sparse_step on the cpu backend."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as FR
import fit_sparse_ref as SR
import orc
import rt_octree_amd as R
import test_fit_rays_host as TH
from helpers import rcam
from rt_octree_amd import optimize_octree, synth
from rt_octree_amd._lib import CFitOptim, lib

E_INVALID = -1
W, H = TH.W, TH.H
BLOCK_WORDS = 2048  # RTO_FIT_TOUCHED_BLOCK_WORDS of include/rto.h (asserted against the library below)
# rates of the ten-step runs, chosen on the host so that the second epoch's loss word is below the first's
LR_RMSPROP, LR_ADAM = 0.01, 0.01
GRAD_SCALE = 2.0 / (3.0 * TH.BATCH)
# max |p32 - p64| / max |p64 - p0| after ten steps of the twin beside torch.optim in float64, measured on the host (DESIGN.md
# 7r), and the bound the test holds: twice that
MEANING_MEASURED = {"rmsprop": 1.72e-5, "adam": 6.94e-4}


def n_slots(t):
    return int(t.child.size)


def call_touched(t, params, o, d, tg, ndc=None, threads=8, grad=None, stats=None, out=None, touched=None, **optkw):
    """one rto_fit_grad_rays_touched_host call -> (out, grad, stats, touched words)"""
    grad = np.zeros(params.shape, np.int64) if grad is None else grad
    stats = np.zeros(2, np.int64) if stats is None else stats
    out = np.full((o.shape[0], 3), TH.SENTINEL, np.float32) if out is None else out
    touched = np.zeros(R.touched_words(n_slots(t)), np.uint32) if touched is None else touched
    R.fit_grad_rays_host(t.child, t.data, params, t.scale, t.offset, t.data_format, o, d, tg, R.RenderOptions(**optkw), ndc=ndc,
                         threads=threads, grad=grad, stats=stats, out=out, touched=touched)
    return out, grad, stats, touched


def check_marks(t, params, grad, words, floor=500):
    """the properties of a touched set: every non-zero grad row is marked, only leaves are, at least `floor` bits are set, and at
    least one leaf of the support stays clear"""
    bits = SR.bits_of(words, n_slots(t))
    D = params.shape[-1]
    rows = grad.reshape(-1, D).any(1)
    assert not (rows & ~bits).any(), "a slot with a non-zero grad word is not marked"
    assert not bits[t.child.reshape(-1) != 0].any(), "an internal slot is marked"
    support = (t.child.reshape(-1) == 0) & (t.data.reshape(-1, D)[:, -1].astype(np.float32) > np.float32(1e-2)) \
        & (params.reshape(-1, D)[:, -1] > np.float32(1e-2))
    assert not (bits & ~support).any(), "a slot outside the support is marked"
    assert bits.sum() >= floor, "only %d bits are set" % bits.sum()
    assert (support & ~bits).any(), "every leaf of the support is marked: the test cannot tell a full set"
    assert not SR.bits_of(words, words.size * 32)[n_slots(t):].any()
    return bits


# ------------------------------------------------------------------ 1. the marking twin
@pytest.mark.parametrize("fmt", TH.FORMATS)
def test_marking_twin_in_every_format(fmt):
    t = TH.make5(fmt)
    o, d = TH.rays_of(TH.cams3())
    params = TH.perturbed_params(t)
    tg = TH.noisy(TH.host_fit(t).render_rays(o, d))
    tg[400, 1] = np.nan  # one masked ray
    got = call_touched(t, params, o, d, tg)
    TH.same(got[:3], TH.call_rays(t, params, o, d, tg), fmt + " against the old twin")
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    want = SR.restate_touched(ht, params, o, d, tg, out=np.full((o.shape[0], 3), TH.SENTINEL, np.float32))
    TH.same(got[:3], want[:3], fmt + " against the restatement")
    assert np.array_equal(got[3], SR.bitmap_of(want[3])), fmt + ": the bitmap differs from the restatement's"
    check_marks(t, params, got[1], got[3])


@pytest.mark.parametrize("name", ["ndc", "shuffled"])
def test_marking_twin_on_an_ndc_and_a_relaid_tree(name):
    t = synth.make_tree(5, 9, seed=7)
    ndc, kw = None, {}
    if name == "ndc":
        ndc = (64.0, 48.0, 50.0)
        pose = [synth.look_at_c2w(p, target=(0, 0, -1), up=(0, 1, 0)) for p in ((0.1, 0.05, 0.3), (-0.2, 0.1, 0.2), (0.0, -0.1, 0.4))]
        cams = [rcam(W, H, p, fx=18.0) for p in pose]  # (23 pixels at fx 18 span the 64 of the NDC frame at focal 50: the whole volume)
    else:
        t = synth.shuffle_nodes(t, seed=3)
        cams = TH.cams3()
    o, d = TH.rays_of(cams)
    params = TH.perturbed_params(t)
    tg = TH.noisy(TH.host_fit(t, ndc=ndc, **kw).render_rays(o, d))
    got = call_touched(t, params, o, d, tg, ndc=ndc, **kw)
    TH.same(got[:3], TH.call_rays(t, params, o, d, tg, ndc=ndc, **kw), name)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format, ndc=ndc)
    want = SR.restate_touched(ht, params, o, d, tg, ndc=ndc)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], SR.bitmap_of(want[3])), name
    check_marks(t, params, got[1], got[3])


@pytest.fixture(scope="module")
def cam_case():
    """(tree, params, origins, dirs, targets, the marking twin's (out, grad, stats, touched) in raster order) -- read only"""
    t = TH.make5("SH9")
    o, d = TH.rays_of(TH.cams3())
    params = TH.perturbed_params(t)
    tg = TH.noisy(TH.host_fit(t).render_rays(o, d))
    tg[W * H + 3 * W + 4, 1] = np.nan
    want = call_touched(t, params, o, d, tg)
    for a in (params, o, d, tg) + want:
        a.setflags(write=False)
    return t, params, o, d, tg, want


def test_the_set_does_not_depend_on_order_splits_or_threads(cam_case):
    t, params, o, d, tg, want = cam_case
    n = o.shape[0]
    check_marks(t, params, want[1], want[3])
    for threads in (1, 3, 8):
        got = call_touched(t, params, o, d, tg, threads=threads)
        TH.same(got[:3], want[:3], "threads %d" % threads)
        assert np.array_equal(got[3], want[3]), "threads %d: the bitmap differs" % threads
    perm = np.random.default_rng(5).permutation(n)
    po, pg, ps, pt = call_touched(t, params, o[perm], d[perm], tg[perm], threads=3)
    back = np.empty_like(po)
    back[perm] = po
    TH.same((back, pg, ps), want[:3], "permuted")
    assert np.array_equal(pt, want[3]), "permuted: the bitmap differs"
    # split into calls of 1, 63, 64, 65 rays and the rest: the call accumulates into the bitmap as into grad
    grad, stats, out = np.zeros(params.shape, np.int64), np.zeros(2, np.int64), np.full((n, 3), TH.SENTINEL, np.float32)
    touched = np.zeros(want[3].size, np.uint32)
    at, sizes = 0, []
    for k in (1, 63, 64, 65, n - 193):
        s = slice(at, at + k)
        call_touched(t, params, o[s], d[s], tg[s], grad=grad, stats=stats, out=out[s], touched=touched, threads=3)
        sizes.append(int(SR.bits_of(touched, n_slots(t)).sum()))
        at += k
    assert at == n and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    TH.same((out, grad, stats), want[:3], "split")
    assert np.array_equal(touched, want[3]), "split: the bitmap differs"


def test_masked_missing_and_unmarched_rays_mark_nothing():
    t = TH.make5("SH9")
    o, d, tg, bad = TH.degenerate_rays(t)
    params = TH.perturbed_params(t)
    # the three rays that are not marched, a masked ray, and a ray that misses the box
    away = np.array([[0.0, 0.0, 9.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    oo = np.concatenate([o[bad], o[9:10], away[0]])
    dd = np.concatenate([d[bad], d[9:10], away[1]])
    tt = np.concatenate([tg[bad], tg[9:10], np.full((1, 3), 0.5, np.float32)])
    out, grad, stats, touched = call_touched(t, params, oo, dd, tt)
    assert stats[1] == 4 and not touched.any() and not grad.any()
    # and with them among rays that do march, the set is that of the others
    full = call_touched(t, params, o, d, tg)
    keep = np.setdiff1d(np.arange(64), bad + [9])
    rest = call_touched(t, params, o[keep], d[keep], tg[keep])
    assert np.array_equal(full[3], rest[3]) and np.array_equal(full[1], rest[1]) and SR.bits_of(full[3], n_slots(t)).sum() > 20


# ------------------------------------------------------------------ 2. the list
LIST_SLOTS = (2 * BLOCK_WORDS + 37) * 32 - 5


def list_patterns():
    """name -> the words of a bitmap of LIST_SLOTS slots (two scan blocks plus 37 words, minus 5 bits)"""
    words = LIST_SLOTS // 32 + 1
    assert words == 2 * BLOCK_WORDS + 37 and LIST_SLOTS % 32 == 27
    rng = np.random.default_rng(17)
    last = np.zeros(words, np.uint32)
    last[-1] = np.uint32(1) << np.uint32((LIST_SLOTS - 1) % 32)
    beyond = np.zeros(words, np.uint32)
    beyond[-1] = np.uint32(0xF8000000)  # the five bits at and beyond slots
    sparse = rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
    sparse[rng.random(words) < 0.5] = 0
    sparse[-1] |= np.uint32(0xC0000000)  # and two bits beyond slots
    return {"all clear": np.zeros(words, np.uint32), "all set": np.full(words, 0xFFFFFFFF, np.uint32), "last valid slot": last,
            "only bits beyond slots": beyond, "random": sparse}


def check_list(run, name, words):
    """run(words, clear, capacity) -> (list, count, words after): the list entry under test, on one pattern"""
    want = SR.list_of(words, LIST_SLOTS)
    for clear in (False, True):
        caps = sorted({0, 1, max(want.size - 1, 0), want.size, want.size + 3})
        for cap in caps:
            lst, count, after = run(words.copy(), clear, cap)
            assert count == want.size, "%s: count %d, not %d" % (name, count, want.size)
            k = min(cap, want.size)
            assert np.array_equal(lst[:k], want[:k]), "%s: the list differs (capacity %d)" % (name, cap)
            assert (lst[k:] == 0xFFFFFFFF).all(), "%s: written past min(count, capacity)" % name
            assert (np.diff(lst[:k].astype(np.int64)) > 0).all()
            assert np.array_equal(after, np.zeros_like(words) if clear else words), "%s: clear = %s" % (name, clear)


def host_list(words, clear, cap):
    lst = np.full(cap, 0xFFFFFFFF, np.uint32)
    count = np.full(1, 99, np.uint64)
    R.touched_list_host(words, LIST_SLOTS, lst, count, clear=clear)
    return lst, int(count[0]), words


@pytest.mark.parametrize("name", ["all clear", "all set", "last valid slot", "only bits beyond slots", "random"])
def test_list_on_synthetic_bitmaps(name):
    assert lib().rto_fit_touched_block_words() == BLOCK_WORDS
    words = list_patterns()[name]
    check_list(host_list, name, words)
    want = SR.list_of(words, LIST_SLOTS)
    assert want.size == {"all clear": 0, "all set": LIST_SLOTS, "last valid slot": 1, "only bits beyond slots": 0}.get(name, want.size)
    if name == "last valid slot":
        assert want[0] == LIST_SLOTS - 1
    if name == "random":
        assert 1000 < want.size < LIST_SLOTS // 2


# ------------------------------------------------------------------ 3. the SGD identity
def test_sparse_sgd_step_leaves_the_dense_steps_bytes(cam_case):
    t, params, o, d, tg, want = cam_case
    dense_p, dense_g = params.copy(), want[1].copy()
    R.sgd_step_host(dense_p, dense_g, TH.LR10)
    p, g, touched = params.copy(), want[1].copy(), want[3].copy()
    lst, count = np.zeros(n_slots(t), np.uint32), np.zeros(1, np.uint64)
    R.touched_list_host(touched, n_slots(t), lst, count)
    assert not touched.any() and count[0] == SR.bits_of(want[3], n_slots(t)).sum()
    R.step_sparse_host(p, g, lst, count, R.fit_optim("sgd", TH.LR10))
    assert np.array_equal(p.view(np.uint32), dense_p.view(np.uint32)) and not g.any() and not dense_g.any()
    assert np.count_nonzero(p != params) > 1000
    # the restatement's step gives them too
    rp, rg = params.copy(), want[1].copy()
    SR.step(SR.SGD, rp, rg, lst[:int(count[0])], TH.LR10)
    assert np.array_equal(rp.view(np.uint32), dense_p.view(np.uint32)) and not rg.any()
    # an entry >= slots is skipped, a count beyond the capacity is cut, count == 0 does nothing
    p2, g2 = params.copy(), want[1].copy()
    R.step_sparse_host(p2, g2, np.array([n_slots(t), 0xFFFFFFFF], np.uint32), np.array([7], np.uint64), R.fit_optim("sgd", TH.LR10))
    R.step_sparse_host(p2, g2, lst, np.zeros(1, np.uint64), R.fit_optim("sgd", TH.LR10))
    assert np.array_equal(p2.view(np.uint32), params.view(np.uint32)) and np.array_equal(g2, want[1])


# ------------------------------------------------------------------ 4. ten RMSProp and Adam steps
def ten_steps_sparse_host(kind, lr, t, o, d, tg, batches, **kw):
    """-> (the loss word of each epoch, the HostTreeFit after the ten steps, the slots ever listed as a bool array)"""
    hf = R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, options=R.RenderOptions(), threads=8, optimizer=kind, **kw)
    hf.params[...] = TH.start_params(t)
    words, ever = [], np.zeros(n_slots(t), bool)
    for epoch in batches:
        for idx in epoch:
            hf.accumulate_rays(o[idx], d[idx], tg[idx])
            ever |= SR.bits_of(hf.touched, n_slots(t))
            hf.step(lr, grad_scale=GRAD_SCALE)
            assert not hf.grad.any() and not hf.touched.any()
        words.append(int(hf.stats[0]))
        assert hf.loss()[1] == 5 * TH.BATCH
    assert hf.t == 10
    return words, hf, ever


@pytest.mark.parametrize("kind,lr", [("rmsprop", LR_RMSPROP), ("adam", LR_ADAM)])
def test_ten_steps_equal_the_restatement_and_lower_the_loss(kind, lr):
    t, o, d, tg, batches = TH.sgd_rays()
    words, hf, ever = ten_steps_sparse_host(kind, lr, t, o, d, tg, batches)
    ht = orc.HostTree(t.child, t.data, t.scale, t.offset, t.data_format)
    p = TH.start_params(t)
    m, v = np.zeros_like(p), np.zeros_like(p)
    want, step = [], 0
    for epoch in batches:
        stats = np.zeros(2, np.int64)
        for idx in epoch:
            _, g, stats, touched = SR.restate_touched(ht, p, o[idx], d[idx], tg[idx], stats=stats)
            step += 1
            SR.step(SR.ADAM if kind == "adam" else SR.RMSPROP, p, g, np.flatnonzero(touched), lr, GRAD_SCALE, t=step, m=m, v=v)
            assert not g.any()
        want.append(int(stats[0]))
    print(kind, "loss words", words, [round(w / FR.FIX, 4) for w in words])
    assert words == want
    assert np.array_equal(hf.params.view(np.uint32), p.view(np.uint32))
    assert np.array_equal(hf.v.view(np.uint32), v.view(np.uint32))
    if kind == "adam":
        assert np.array_equal(hf.m.view(np.uint32), m.view(np.uint32))
    else:
        assert hf.m is None
    # rows never listed keep their bits in all three arrays
    D = p.shape[-1]
    never = ~ever
    assert never.sum() > 100 and ever.sum() > 500
    assert np.array_equal(hf.params.reshape(-1, D)[never].view(np.uint32), TH.start_params(t).reshape(-1, D)[never].view(np.uint32))
    assert not hf.v.reshape(-1, D)[never].view(np.uint32).any()
    assert hf.v.reshape(-1, D)[ever].any(1).sum() > 500
    if kind == "adam":
        assert not hf.m.reshape(-1, D)[never].view(np.uint32).any()
    assert words[1] < words[0], "the second epoch's loss word is not below the first's"


# ------------------------------------------------------------------ 5. meaning: torch.optim in float64
def meaning_case():
    """a case where every leaf of the support is touched at every step: a depth-3 tree, all rays of three cameras per step, no
    early stop"""
    t = synth.make_tree(3, 4, seed=7)
    o, d = TH.rays_of(TH.cams3())
    tg = TH.host_fit(t, stop_thresh=0.0).render_rays(o, d)
    return t, o, d, tg


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_ten_steps_beside_torch_optim_in_float64(kind):
    import torch
    t, o, d, tg = meaning_case()
    lr, gs, b1, b2, eps = 0.01, 2.0 / (3.0 * o.shape[0]), 0.9, 0.999, 1e-8
    hf = R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, options=R.RenderOptions(stop_thresh=0.0), threads=8,
                       optimizer=kind, beta1=b1, beta2=b2, eps=eps)
    hf.params[...] = TH.start_params(t)
    p0 = hf.params.astype(np.float64)
    p64 = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    if kind == "adam":
        opt = torch.optim.Adam([p64], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps))
    else:
        opt = torch.optim.RMSprop([p64], lr=f32(lr), alpha=f32(b2), eps=f32(eps))
    D = hf.params.shape[-1]
    support = (t.child.reshape(-1) == 0) & (t.data.reshape(-1, D)[:, -1].astype(np.float32) > np.float32(1e-2))
    for _ in range(10):
        hf.accumulate_rays(o, d, tg)
        bits = SR.bits_of(hf.touched, n_slots(t))
        dense = support & (hf.params.reshape(-1, D)[:, -1] > np.float32(1e-2))
        assert np.array_equal(bits, dense) and bits.sum() > 50, "not every dense leaf is touched at this step"
        g32 = (hf.grad.astype(np.float64) * (1.0 / FR.FIX)).astype(np.float32)  # from_fixed
        p64.grad = torch.tensor(g32.astype(np.float64) * f32(gs), dtype=torch.float64)
        opt.step()
        hf.step(lr, grad_scale=gs)
    got = hf.params.astype(np.float64)
    ref = p64.detach().numpy()
    moved = np.abs(ref - p0).max()
    err = np.abs(got - ref).max() / moved
    print("%s: max |p32 - p64| / max |p64 - p0| = %.3g (moved %.3g), bound %.3g" % (kind, err, moved, 2 * MEANING_MEASURED[kind]))
    assert moved > 0.05
    assert err <= 2 * MEANING_MEASURED[kind]


# ------------------------------------------------------------------ 6. refusals, the tool
def test_refusal_texts():
    t = synth.make_tree(4, 4, seed=7)
    params = t.data.astype(np.float32)
    slots, D = n_slots(t), params.shape[-1]
    grad, stats = np.zeros(params.shape, np.int64), np.zeros(2, np.int64)
    touched = np.zeros(R.touched_words(slots) + 1, np.uint32)
    n = 8
    buf = np.zeros((4, n + 1, 3), np.float32)
    buf[1] = 1.0
    pp, gp, sp, tp_ = params.ctypes.data, grad.ctypes.data, stats.ctypes.data, touched.ctypes.data
    op, dp, tp, up = (buf[k].ctypes.data for k in range(4))
    sc = (C.c_float * 3)(*[float(v) for v in t.scale])
    of = (C.c_float * 3)(*[float(v) for v in t.offset])
    data = t.data.view(np.uint16)
    co = R.RenderOptions().to_c()

    def raw(params=pp, origins=op, dirs=dp, targets=tp, out=up, n=n, grad=gp, stats=sp, touched=tp_):
        return lib().rto_fit_grad_rays_touched_host(C.c_void_p(t.child.ctypes.data), C.c_void_p(data.ctypes.data), params, t.child.shape[0],
                                                    2, D, t.data_format.encode(), sc, of, None, origins, dirs, targets, out, n,
                                                    C.byref(co), 0, grad, stats, touched)

    def refused(call, prefix, text, **kw):
        rc = call(**kw)
        msg = lib().rto_last_error().decode()
        assert rc == E_INVALID and text in msg and msg.startswith(prefix), (rc, msg, text)

    assert raw() == 0
    grad[...] = 0
    stats[...] = 0
    touched[...] = 0
    buf[3] = 0
    w = "rto_fit_grad_rays_touched_host: "
    refused(raw, w, "null grad: a forward-only call uses the entry without the bitmap", grad=None)
    refused(raw, w, "null grad", grad=None, stats=None, targets=None)
    refused(raw, w, "null touched", touched=None)
    refused(raw, w, "touched must be 4-byte aligned", touched=tp_ + 2)
    refused(raw, w, "touched overlaps params", touched=pp + 64)
    refused(raw, w, "touched overlaps grad", touched=gp + 8 * (grad.size - 1))
    refused(raw, w, "touched overlaps stats", touched=sp + 8)
    refused(raw, w, "touched overlaps origins", touched=op)
    refused(raw, w, "touched overlaps dirs", touched=dp + 4)
    refused(raw, w, "touched overlaps targets", touched=tp + 12 * (n - 1))
    refused(raw, w, "touched overlaps out", touched=up)
    refused(raw, w, "null params", params=None)  # and what the old entry refuses
    refused(raw, w, "n must be >= 0", n=-1)
    refused(raw, w, "null targets with grad or stats set", targets=None)
    assert not grad.any() and not stats.any() and not touched.any() and not buf[3].any(), "a refused call wrote"

    # the list
    lst, count = np.zeros(16, np.uint32), np.zeros(2, np.uint64)
    lp, cp = lst.ctypes.data, count.ctypes.data

    def raw_list(touched=tp_, slots=slots, list_=lp, cap=16, count=cp):
        return lib().rto_fit_touched_list_host(touched, slots, 0, list_, cap, count)

    w = "rto_fit_touched_list_host: "
    assert raw_list() == 0 and count[0] == 0
    refused(raw_list, w, "null touched", touched=None)
    refused(raw_list, w, "null count", count=None)
    refused(raw_list, w, "slots must be in [0, 2^31)", slots=-1)
    refused(raw_list, w, "slots must be in [0, 2^31)", slots=2 ** 31)
    refused(raw_list, w, "list_capacity must be >= 0", cap=-1)
    refused(raw_list, w, "null list with list_capacity > 0", list_=None)
    assert raw_list(list_=None, cap=0) == 0
    refused(raw_list, w, "touched must be 4-byte aligned", touched=tp_ + 1)
    refused(raw_list, w, "list must be 4-byte aligned", list_=lp + 2)
    refused(raw_list, w, "count must be 8-byte aligned", count=cp + 4)
    assert lib().rto_fit_touched_scratch_bytes(-1) == -1 and lib().rto_fit_touched_scratch_bytes(2 ** 31) == -1
    assert lib().rto_fit_touched_scratch_bytes(0) == 4 and lib().rto_fit_touched_scratch_bytes(LIST_SLOTS) == 12

    # the step
    m, v = np.zeros_like(params), np.zeros_like(params)
    mp, vp = m.ctypes.data, v.ctypes.data

    def raw_step(params=pp, grad=gp, m=mp, v=vp, slots=slots, row=D, list_=lp, count=cp, cap=16, kind=2, opt=True):
        o = CFitOptim(kind, 0.1, 1.0, 0.9, 0.999, 1e-8, 0.1, 0.001)
        return lib().rto_fit_step_sparse_host(params, grad, m, v, slots, row, list_, count, cap, C.byref(o) if opt else None)

    w = "rto_fit_step_sparse_host: "
    count[0] = 0
    assert raw_step() == 0
    for name, key in (("params", "params"), ("grad", "grad"), ("list", "list_"), ("count", "count")):
        refused(raw_step, w, "null " + name, **{key: None})
    refused(raw_step, w, "null options", opt=False)
    refused(raw_step, w, "row must be >= 1", row=0)
    refused(raw_step, w, "slots must be in [0, 2^31)", slots=-1)
    refused(raw_step, w, "list_capacity must be >= 0", cap=-1)
    refused(raw_step, w, "unknown kind 3", kind=3)
    refused(raw_step, w, "unknown kind -1", kind=-1)
    refused(raw_step, w, "null m: RTO_FIT_ADAM keeps a first moment", m=None)
    refused(raw_step, w, "null v: RTO_FIT_RMSPROP and RTO_FIT_ADAM keep a second moment", v=None)
    refused(raw_step, w, "null v", v=None, kind=1)
    assert raw_step(m=None, kind=1) == 0 and raw_step(m=None, v=None, kind=0) == 0
    refused(raw_step, w, "params must be 4-byte aligned", params=pp + 2)
    refused(raw_step, w, "grad must be 8-byte aligned", grad=gp + 4)
    refused(raw_step, w, "m must be 4-byte aligned", m=mp + 1)
    refused(raw_step, w, "v must be 4-byte aligned", v=vp + 2)
    refused(raw_step, w, "list must be 4-byte aligned", list_=lp + 1)
    refused(raw_step, w, "count must be 8-byte aligned", count=cp + 4)
    # the Python layer's own
    with pytest.raises(R.RtoError):
        R.fit_optim("lion")
    with pytest.raises(R.RtoError):
        R.HostTreeFit(t.child, t.data, t.scale, t.offset, t.data_format, optimizer="lion")
    with pytest.raises(R.RtoError):
        R.fit_grad_rays_host(t.child, t.data, params, t.scale, t.offset, t.data_format, buf[0][:n], buf[1][:n], buf[2][:n], grad=grad,
                             touched=np.zeros(3, np.uint32))
    with pytest.raises(R.RtoError):
        TH.host_fit(t).step(1.0, grad_scale=0.5)


def test_bias_floats_are_those_of_the_restatement():
    for t in (1, 2, 10, 1000):
        o = R.fit_optim("adam", 0.1, t=t)
        assert np.float32(o.bias1) == SR.bias(0.9, t) and np.float32(o.bias2) == SR.bias(0.999, t)


def test_optimize_octree_sparse_step_and_optimizers_on_the_cpu(tmp_path, capsys):
    tree = TH.make5("SH9")
    js, pert = TH.write_dataset(tmp_path, tree)
    run = lambda name, *flags: TH.run_tool(tmp_path, name, pert, js, "cpu", *flags)  # noqa: E731
    # --optimizer sgd --sparse_step writes the bytes of the default run: image batches, and shuffled ray batches
    plain = run("plain", "--batch_imgs", "2")
    assert run("sparse", "--batch_imgs", "2", "--optimizer", "sgd", "--sparse_step") == plain
    rays = run("rays", "--batch_rays", str(TH.BATCH), "--seed", "1")
    assert run("rays_sparse", "--batch_rays", str(TH.BATCH), "--seed", "1", "--sparse_step") == rays
    assert rays != plain
    # the default command line (no --lr: 1000) is unchanged by the new default of the parser
    base = [pert, "--poses", js, "--epochs", "1", "--backend", "cpu"]
    assert optimize_octree.main(base + ["--out_dir", str(tmp_path / "d0")]) == 0
    assert optimize_octree.main(base + ["--out_dir", str(tmp_path / "d1"), "--lr", "1000"]) == 0
    assert (tmp_path / "d0" / "pert.npz").read_bytes() == (tmp_path / "d1" / "pert.npz").read_bytes()
    # adam and rmsprop need --lr, run, and change the tree
    capsys.readouterr()
    for kind in ("adam", "rmsprop"):
        assert optimize_octree.main(base + ["--out_dir", str(tmp_path / "bad"), "--optimizer", kind]) == 2
        assert "needs an explicit --lr" in capsys.readouterr().err
    out = {}
    for kind in ("adam", "rmsprop"):
        d = tmp_path / kind
        assert optimize_octree.main([pert, "--poses", js, "--epochs", "2", "--backend", "cpu", "--out_dir", str(d), "--optimizer", kind,
                                     "--lr", "0.01", "--batch_rays", str(TH.BATCH)]) == 0
        out[kind] = (d / "pert.npz").read_bytes()
        with np.load(d / "pert.npz") as f, np.load(pert) as z:
            assert f["data"].dtype == np.float16 and np.array_equal(f["child"], z["child"])
            assert np.count_nonzero(f["data"].view(np.uint16) != z["data"].view(np.uint16)) > 1000
    assert out["adam"] != out["rmsprop"] and out["adam"] != rays
    assert optimize_octree.main(base + ["--out_dir", str(tmp_path / "bad"), "--optimizer", "adam", "--lr", "0.01", "--beta2", "1.0"]) == 2
