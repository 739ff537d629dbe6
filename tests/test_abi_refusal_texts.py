"""What the C ABI answers to a bad call -- the returned code and the whole rto_last_error() text -- for the entries whose host
code sits on rto_abi_common.h: the fused GuidanceNet, the image metrics, the training step, the plain filter entries and the
two *_create of the render side.  EXPECTED was recorded from a librto.so built from the commit BEFORE that header existed
(PYTHONPATH=. RTO_LIB=<that build> python tests/test_abi_refusal_texts.py host, and ... gpu on a machine with a device): the texts and codes
are that build's, and this file holds the library to them.  The host half needs no device; the gpu half needs live handles."""
import ctypes as C
import sys

import numpy as np
import pytest

from rt_octree_amd import _lib

P = 0x1000  # a non-null pointer: no refused call reads through it
BIG = (2, 32768, 32768)  # n x H x W = 2^31 pixels

# label -> (code, rto_last_error())
EXPECTED = {
    # ---- decided on the host
    'acts_bytes/null bytes': (-1, 'rto_guidance_train_acts_bytes: null argument'),
    'acts_bytes/null layers': (-1, 'rto_guidance_train_acts_bytes: null argument'),
    'acts_bytes/n 0': (-1, 'rto_guidance_train_acts_bytes: n, H and W must be at least 1, not 0, 8, 8'),
    'acts_bytes/H 0': (-1, 'rto_guidance_train_acts_bytes: n, H and W must be at least 1, not 1, 0, 8'),
    'acts_bytes/W -1': (-1, 'rto_guidance_train_acts_bytes: n, H and W must be at least 1, not 1, 8, -1'),
    'acts_bytes/one layer': (-1, 'rto_guidance_train_acts_bytes: num_layers must be 2 or 3, not 1'),
    'acts_bytes/four layers': (-1, 'rto_guidance_train_acts_bytes: num_layers must be 2 or 3, not 4'),
    'acts_bytes/null weight': (-1, 'rto_guidance_train_acts_bytes: null pointer in layer 1'),
    'acts_bytes/null bias': (-1, 'rto_guidance_train_acts_bytes: null pointer in layer 0'),
    'acts_bytes/no channels': (-1, 'rto_guidance_train_acts_bytes: layer 0 has no channels'),
    'acts_bytes/first cin 7': (-1, 'rto_guidance_train_acts_bytes: layer 0 takes 7 channels but is given 8'),
    'acts_bytes/broken chain': (-1, 'rto_guidance_train_acts_bytes: layer 1 takes 9 channels but is given 8'),
    'acts_bytes/last cout': (-1, 'rto_guidance_train_acts_bytes: the last layer writes 6 channels, not 2 * levels = 8'),
    'acts_bytes/2^31 pixels': (-1, 'rto_guidance_train_acts_bytes: 2 x 32768 x 32768 pixels exceed the 2^31 - 1 the index arithmetic takes'),
    'acts_bytes/c1 65': (-3, 'rto_guidance_train_acts_bytes: 8 -> c1 [-> c1] -> 2 * levels with c1 in 1..64 and levels in 1..6 only (c1 65, levels 4)'),
    'acts_bytes/levels 7': (-3, 'rto_guidance_train_acts_bytes: 8 -> c1 [-> c1] -> 2 * levels with c1 in 1..64 and levels in 1..6 only (c1 8, levels 7)'),
    'acts_bytes/middle widens': (-3, 'rto_guidance_train_acts_bytes: 8 -> c1 [-> c1] -> 2 * levels with c1 in 1..64 and levels in 1..6 only (c1 8, levels 4)'),
    'create_layers/null layers': (-1, 'rto_guidance_net_create_layers: null argument'),
    'create_layers/null out': (-1, 'rto_guidance_net_create_layers: null argument'),
    'create_layers/no layers': (-1, 'rto_guidance_net_create_layers: null argument'),
    'create_layers/null bias': (-1, 'rto_guidance_net_create_layers: layer 1 has a null pointer or no channels'),
    'create_layers/no channels': (-1, 'rto_guidance_net_create_layers: layer 0 has a null pointer or no channels'),
    'create_layers/first cin 7': (-1, 'rto_guidance_net_create_layers: the first layer reads the 8 aux channels, not 7'),
    'create_layers/broken chain': (-1, 'rto_guidance_net_create_layers: layer 2 reads 12 channels, the layer before it writes 8'),
    'create_layers/last cout': (-1, 'rto_guidance_net_create_layers: the last layer writes 6 channels, kernel_levels = 4 needs twice that number'),
    'create_layers/levels 0': (-1, 'rto_guidance_net_create_layers: the last layer writes 8 channels, kernel_levels = 0 needs twice that number'),
    'create_layers/one layer': (-3, 'fused GuidanceNet: two or three layers, not 1'),
    'create_layers/four layers': (-3, 'fused GuidanceNet: two or three layers, not 4'),
    'create_layers/c1 65': (-3, 'fused GuidanceNet: mid_channels 1..64 (8 -> 65 x 1 -> 2 x 4)'),
    'create_layers/middle widens': (-3, 'fused GuidanceNet: the middle layer keeps mid_channels (8 -> 8 x 2 -> 2 x 4)'),
    'create_layers/levels 7': (-3, 'fused GuidanceNet: kernel_levels 1..6 (8 -> 8 x 1 -> 2 x 7)'),
    'create_layers/nan weight': (-1, 'rto_guidance_net_create_layers: layer 1 has a non-finite weight'),
    'create_layers/inf bias': (-1, 'rto_guidance_net_create_layers: layer 0 has a non-finite bias'),
    'net_create/null': (-1, 'rto_guidance_net_create: null argument'),
    'net_create/c1 65': (-3, 'fused GuidanceNet supports mid_channels 1..64, kernel_levels 1..6'),
    'filtering_batch/null': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch/H 0': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch/n 0': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch/L 7': (-1, 'Kernel size == 15 not supported.'),
    'filtering_batch/L 0': (-1, 'Kernel size == 1 not supported.'),
    'filtering_batch/in == out': (-1, 'rto_filtering: img_in and img_out must differ'),
    'filtering/null': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch_mode/unknown mode': (-1, 'rto_filtering_batch_mode: unknown mode'),
    'filtering_batch_mode/unknown mode before null': (-1, 'rto_filtering_batch_mode: unknown mode'),
    'filtering_batch_mode/exact null': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch_mode/fast null': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch_mode/fast H 0': (-1, 'rto_filtering: null pointer or bad size'),
    'filtering_batch_mode/fast L 7': (-1, 'Kernel size == 15 not supported.'),
    'filtering_batch_mode/fast in == out': (-1, 'rto_filtering: img_in and img_out must differ'),
    'filtering_train_forward/null': (-1, 'rto_filtering_train_forward: null pointer or bad size'),
    'filtering_train_forward/W 0': (-1, 'rto_filtering_train_forward: null pointer or bad size'),
    'filtering_train_forward/L 7': (-1, 'Kernel size == 15 not supported.'),
    'filtering_train_forward/in == out': (-1, 'rto_filtering_train_forward: img_in and img_out must differ'),
    'filtering_backward/null': (-1, 'rto_filtering_backward: null pointer or bad size'),
    'filtering_backward/n 0': (-1, 'rto_filtering_backward: null pointer or bad size'),
    'filtering_backward/L 7': (-1, 'Kernel size == 15 not supported.'),
    'launch_strips/n 0': (-1, 'rto_denoise_launch_strips: bad argument'),
    'launch_strips/null out': (-1, 'rto_denoise_launch_strips: bad argument'),
    'null/net_get_info': (-1, 'rto_guidance_net_get_info: null argument'),
    'null/net_forward': (-1, 'rto_guidance_net_forward: bad argument'),
    'null/net_forward_ex': (-1, 'rto_guidance_net_forward: bad argument'),
    'null/net_forward_culled': (-1, 'rto_guidance_net_forward_culled: bad argument'),
    'null/net_forward_culled no marks': (-1, 'rto_guidance_net_forward: bad argument'),
    'null/net_forward_packed': (-1, 'rto_guidance_net_forward_packed: bad argument'),
    'null/net_forward_packed_culled': (-1, 'rto_guidance_net_forward_packed: bad argument'),
    'null/filtering_packed': (-1, 'rto_filtering_packed: bad argument'),
    'null/filtering_packed_culled': (-1, 'rto_filtering_packed_culled: bad argument'),
    'null/filtering_packed_culled no marks': (-1, 'rto_filtering_packed: bad argument'),
    'null/filtering_culled': (-1, 'rto_filtering_culled: null network handle'),
    'null/denoise': (-1, 'rto_denoise: bad argument'),
    'null/net_reserve': (-1, 'rto_guidance_net_reserve: bad argument'),
    'null/metrics_create': (-1, 'rto_metrics_create: null argument'),
    'null/metrics_compute': (-1, 'rto_metrics_compute: null argument'),
    'null/metrics_compute_async': (-1, 'rto_metrics_compute_async: null argument'),
    'null/image_read_png': (-1, 'rto_image_read_png: null argument'),
    'null/train_create': (-1, 'rto_guidance_train_create: null argument'),
    'null/train_forward': (-1, 'rto_guidance_train_forward: null argument'),
    'null/train_backward': (-1, 'rto_guidance_train_backward: null argument'),
    'null/loss': (-1, 'rto_loss_forward_backward: null argument'),
    'null/image_write_png': (-1, 'rto_image_write_png: a null argument or an empty image'),
    'create/net, no device': (-4, 'no HIP device available'),
    'create/metrics, no device': (-4, 'no HIP device available'),
    'create/train, no device': (-4, 'no HIP device available'),
    'create/ctx, no device': (-4, 'no HIP device available (librto has no CPU fallback)'),
    # (on a machine with a device: the index one past the last)
    'create/net, device index': (-1, 'device index out of range'),
    'create/metrics, device index': (-1, 'device index out of range'),
    'create/train, device index': (-1, 'device index out of range'),
    'create/ctx, device index': (-1, 'device index out of range'),
    # ---- live handles, in the order of the checks
    'metrics/null pred': (-1, 'rto_metrics_compute: null argument'),
    'metrics/null out': (-1, 'rto_metrics_compute: null argument'),
    'metrics/n 0': (-1, 'rto_metrics_compute: n, H and W must be at least 1, not 0, 11, 11'),
    'metrics/pred format 5': (-1, 'rto_metrics_compute: unknown image format 5 (RTO_IMAGE_RGBA32F or RTO_IMAGE_RGBA8)'),
    'metrics/truth format 7': (-1, 'rto_metrics_compute: unknown image format 7 (RTO_IMAGE_RGBA32F or RTO_IMAGE_RGBA8)'),
    'metrics/flag bits 6': (-1, 'rto_metrics_compute: unknown flag bits 6'),
    'metrics/nan background': (-1, 'rto_metrics_compute: the background is not finite'),
    'metrics/2^31 pixels': (-1, 'rto_metrics_compute: 2 x 32768 x 32768 pixels exceed the 2^31 - 1 the index arithmetic takes'),
    'metrics/pred misaligned': (-1, 'rto_metrics_compute: an image is not aligned to its pixel size (16 bytes RGBA32F, 4 bytes RGBA8)'),
    'metrics/truth misaligned for bytes': (-1, 'rto_metrics_compute: an image is not aligned to its pixel size (16 bytes RGBA32F, 4 bytes RGBA8)'),
    'metrics/pred on the host': (-1, "rto_metrics_compute: pred is not memory of the handle's device"),
    'metrics/truth on the host': (-1, "rto_metrics_compute: truth is not memory of the handle's device"),
    'metrics_async/n 0': (-1, 'rto_metrics_compute_async: n, H and W must be at least 1, not 0, 8, 8'),
    'metrics_async/out misaligned': (-1, 'rto_metrics_compute_async: device_out is not aligned to 8 bytes'),
    'metrics_async/out on the host': (-1, "rto_metrics_compute_async: device_out is not memory of the handle's device"),
    'metrics/ok': (0, ''),
    'loss/null truth': (-1, 'rto_loss_forward_backward: null argument'),
    'loss/H 0': (-1, 'rto_loss_forward_backward: n, H and W must be at least 1, not 1, 0, 8'),
    'loss/kind 2': (-1, 'rto_loss_forward_backward: unknown loss 2 (RTO_LOSS_SMAPE or RTO_LOSS_MSE)'),
    'loss/2^31 pixels': (-1, 'rto_loss_forward_backward: 2 x 32768 x 32768 pixels exceed the 2^31 - 1 the index arithmetic takes'),
    'loss/pred misaligned': (-1, 'rto_loss_forward_backward: an image is not aligned to 16 bytes, or device_loss not to 8'),
    'loss/loss misaligned': (-1, 'rto_loss_forward_backward: an image is not aligned to 16 bytes, or device_loss not to 8'),
    'loss/ok': (0, ''),
    'train_forward/n 0': (-1, 'rto_guidance_train_forward: n, H and W must be at least 1, not 0, 8, 8'),
    'train_forward/levels 3': (-1, 'rto_guidance_train_forward: the last layer writes 8 channels, not 2 * levels = 6'),
    'train_backward/five layers': (-1, 'rto_guidance_train_backward: num_layers must be 2 or 3, not 5'),
    'train_backward/null grad_bias': (-1, 'rto_guidance_train_backward: null pointer in layer 1'),
    'general/reserve': (-3, 'rto_guidance_net_reserve: the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'general/forward_packed': (-3, 'rto_guidance_net_forward_packed: the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'general/filtering_packed': (-3, 'rto_filtering_packed: the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'general/filtering_packed_culled': (-3, 'rto_filtering_packed_culled: the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'general/forward_ex sparse': (-3, 'rto_guidance_net_forward_ex(RTO_NET_INPUT_SPARSE): the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'general/forward_culled sparse': (-3, 'rto_guidance_net_forward_culled(RTO_NET_INPUT_SPARSE): the packed / sparse route serves mid_channels = 32, kernel_levels = 4, two layers only; this net is 8 -> 8 -> 2 x 4 (2 layers): use the fp32 planes (rto_guidance_net_forward*, rto_filtering_culled, rto_denoise)'),
    'packed/in == out': (-1, 'rto_filtering_packed: bad argument'),
    'packed/no maps yet': (-1, 'rto_filtering_packed: no packed maps (call rto_guidance_net_forward_packed first)'),
    'packed_culled/no maps yet': (-1, 'rto_filtering_packed_culled: no packed maps (call rto_guidance_net_forward_packed first)'),
    'forward_packed/n 0': (-1, 'rto_guidance_net_forward_packed: bad argument'),
    'forward_packed/sparse without marks': (-1, 'rto_guidance_net_forward_packed_culled: RTO_NET_INPUT_SPARSE needs the tile marks of the launch and RTO_NET_INPUT_RGBA'),
    'forward_packed_culled/words': (-1, 'rto_guidance_net_forward_packed_culled: the tile marks are not those of a 8 x 8 frame (rto_ctx_tile_marks)'),
    'forward_packed_culled/sparse without rgba': (-1, 'rto_guidance_net_forward_packed_culled: RTO_NET_INPUT_SPARSE needs the tile marks of the launch and RTO_NET_INPUT_RGBA'),
    'forward_packed/ok': (0, ''),
    'packed/two images': (-1, 'rto_filtering_packed: 2 x 8 x 8 images, but the packed maps hold 1 x 8 x 8'),
    'packed/another height': (-1, 'rto_filtering_packed: 1 x 16 x 8 images, but the packed maps hold 1 x 8 x 8'),
    'packed_culled/another width': (-1, 'rto_filtering_packed_culled: 1 x 8 x 16 images, but the packed maps hold 1 x 8 x 8'),
    'packed_culled/words': (-1, 'rto_filtering_packed_culled: the tile marks are not those of a 8 x 8 frame (rto_ctx_tile_marks)'),
    'forward_culled/n 0': (-1, 'rto_guidance_net_forward_culled: bad argument'),
    'forward_culled/words': (-1, 'rto_guidance_net_forward_culled: the tile marks are not those of a 8 x 8 frame (rto_ctx_tile_marks)'),
    'filtering_culled/H 0': (-1, 'rto_filtering_culled: bad argument'),
    'filtering_culled/in == out': (-1, 'rto_filtering_culled: bad argument'),
    'filtering_culled/mode 3': (-1, 'rto_filtering_culled: unknown mode'),
    'filtering_culled/words': (-1, 'rto_filtering_culled: the tile marks are not those of a 8 x 8 frame (rto_ctx_tile_marks)'),
    'filtering_culled/no marks, mode 3': (-1, 'rto_filtering_batch_mode: unknown mode'),
    'reserve/same size': (0, ''),
    'packed/still there': (0, ''),
    'reserve/grows': (0, ''),
    'packed/gone after the growing reserve': (-1, 'rto_filtering_packed: no packed maps (call rto_guidance_net_forward_packed first)'),
    'packed_culled/gone after the growing reserve': (-1, 'rto_filtering_packed_culled: no packed maps (call rto_guidance_net_forward_packed first)'),
}


def _train_layers(chain, ptr=P):
    """[(cin, cout)] -> rto_guidance_train_layer array whose pointers are `ptr` (never read by a refused call)"""
    arr = (_lib.CGuidanceTrainLayer * len(chain))()
    for l, (cin, cout) in zip(arr, chain):
        l.weight, l.bias, l.grad_weight, l.grad_bias, l.cin, l.cout = ptr, ptr, ptr, ptr, cin, cout
    return arr


def _net_layers(chain):
    """[(cin, cout)] -> rto_guidance_layer array over host weights (arr.backing = [w0, b0, w1, b1, ...] keeps them alive)"""
    arr = (_lib.CGuidanceLayer * len(chain))()
    arr.backing = []
    for l, (cin, cout) in zip(arr, chain):
        w = np.full((max(cout, 1), max(cin, 1), 3, 3), 0.125, np.float32)
        b = np.zeros(max(cout, 1), np.float32)
        arr.backing += [w, b]
        l.weight, l.bias, l.cin, l.cout = w.ctypes.data, b.ctypes.data, cin, cout
    return arr


def host_cases(L):
    """[(label, call -> code)] of the refusals that are decided before any device is used"""
    cases = []
    add = lambda label, call: cases.append((label, call))  # noqa: E731

    # ---- rto_guidance_train_acts_bytes: every branch of the training unit's check_shape
    nbytes = C.c_size_t(0)

    def acts(chain, levels=4, n=1, H=8, W=8, nl=None, out=True, edit=None):
        arr = _train_layers(chain) if chain is not None else None
        if edit:
            edit(arr)
        return lambda: L.rto_guidance_train_acts_bytes(arr, len(chain) if nl is None else nl, levels, n, H, W, C.byref(nbytes) if out else None)

    good = [(8, 8), (8, 8)]
    add("acts_bytes/null bytes", acts(good, out=False))
    add("acts_bytes/null layers", acts(None, nl=2))
    add("acts_bytes/n 0", acts(good, n=0))
    add("acts_bytes/H 0", acts(good, H=0))
    add("acts_bytes/W -1", acts(good, W=-1))
    add("acts_bytes/one layer", acts(good, nl=1))
    add("acts_bytes/four layers", acts(good + good, nl=4))
    add("acts_bytes/null weight", acts(good, edit=lambda a: setattr(a[1], "weight", None)))
    add("acts_bytes/null bias", acts(good, edit=lambda a: setattr(a[0], "bias", None)))
    add("acts_bytes/no channels", acts([(8, 0), (0, 8)]))
    add("acts_bytes/first cin 7", acts([(7, 8), (8, 8)]))
    add("acts_bytes/broken chain", acts([(8, 8), (9, 8)]))
    add("acts_bytes/last cout", acts([(8, 8), (8, 6)]))
    add("acts_bytes/2^31 pixels", acts(good, n=BIG[0], H=BIG[1], W=BIG[2]))
    add("acts_bytes/c1 65", acts([(8, 65), (65, 8)]))
    add("acts_bytes/levels 7", acts([(8, 8), (8, 14)], levels=7))
    add("acts_bytes/middle widens", acts([(8, 8), (8, 16), (16, 8)]))

    # ---- rto_guidance_net_create_layers / rto_guidance_net_create
    h = C.c_void_p(0)

    def create(chain, levels, nl=None, out=True, edit=None):
        arr = _net_layers(chain) if chain is not None else None
        if edit:
            edit(arr)
        return lambda: L.rto_guidance_net_create_layers(arr, len(chain) if nl is None else nl, levels, 0, C.byref(h) if out else None)

    def poison(index, value):
        def edit(arr):
            arr.backing[index].reshape(-1)[3] = value
        return edit

    add("create_layers/null layers", create(None, 4, nl=2))
    add("create_layers/null out", create([(8, 8), (8, 8)], 4, out=False))
    add("create_layers/no layers", create([(8, 8), (8, 8)], 4, nl=0))
    add("create_layers/null bias", create([(8, 8), (8, 8)], 4, edit=lambda a: setattr(a[1], "bias", None)))
    add("create_layers/no channels", create([(8, 0), (0, 8)], 4))
    add("create_layers/first cin 7", create([(7, 8), (8, 8)], 4))
    add("create_layers/broken chain", create([(8, 8), (8, 8), (12, 8)], 4))
    add("create_layers/last cout", create([(8, 8), (8, 6)], 4))
    add("create_layers/levels 0", create([(8, 8), (8, 8)], 0))
    add("create_layers/one layer", create([(8, 8)], 4))
    add("create_layers/four layers", create([(8, 8), (8, 8), (8, 8), (8, 8)], 4))
    add("create_layers/c1 65", create([(8, 65), (65, 8)], 4))
    add("create_layers/middle widens", create([(8, 8), (8, 16), (16, 8)], 4))
    add("create_layers/levels 7", create([(8, 8), (8, 14)], 7))
    add("create_layers/nan weight", create([(8, 8), (8, 8)], 4, edit=poison(2, np.nan)))
    add("create_layers/inf bias", create([(8, 8), (8, 8)], 4, edit=poison(1, np.inf)))
    add("net_create/null", lambda: L.rto_guidance_net_create(None, P, P, P, 8, 4, 0, C.byref(h)))
    add("net_create/c1 65", lambda: L.rto_guidance_net_create(P, P, P, P, 65, 4, 0, C.byref(h)))

    # ---- the four plain filter entries
    def batch(w=P, L_=4, H=8, W=8, n=1, i=P, o=P + 16):
        return lambda: L.rto_filtering_batch(None, w, P, L_, H, W, n, i, o)

    def mode(m, w=P, L_=4, H=8, i=P, o=P + 16):
        return lambda: L.rto_filtering_batch_mode(None, w, P, L_, H, 8, 1, i, o, m)

    def train(w=P, L_=4, W=8, i=P, o=P + 16, inv=P):
        return lambda: L.rto_filtering_train_forward(None, w, P, L_, 8, W, 1, i, o, P, P, inv)

    def back(go=P, L_=4, n=1, gg=P):
        return lambda: L.rto_filtering_backward(None, go, P, P, P, P, P, P, L_, 8, 8, n, P, gg)

    add("filtering_batch/null", batch(w=None))
    add("filtering_batch/H 0", batch(H=0))
    add("filtering_batch/n 0", batch(n=0))
    add("filtering_batch/L 7", batch(L_=7))
    add("filtering_batch/L 0", batch(L_=0))
    add("filtering_batch/in == out", batch(o=P))
    add("filtering/null", lambda: L.rto_filtering(None, P, None, 4, 8, 8, P, P + 16))
    add("filtering_batch_mode/unknown mode", mode(7))
    add("filtering_batch_mode/unknown mode before null", mode(7, w=None))
    add("filtering_batch_mode/exact null", mode(0, w=None))
    add("filtering_batch_mode/fast null", mode(1, w=None))
    add("filtering_batch_mode/fast H 0", mode(1, H=0))
    add("filtering_batch_mode/fast L 7", mode(1, L_=7))
    add("filtering_batch_mode/fast in == out", mode(1, o=P))
    add("filtering_train_forward/null", train(inv=None))
    add("filtering_train_forward/W 0", train(W=0))
    add("filtering_train_forward/L 7", train(L_=7))
    add("filtering_train_forward/in == out", train(o=P))
    add("filtering_backward/null", back(gg=None))
    add("filtering_backward/n 0", back(n=0))
    add("filtering_backward/L 7", back(L_=7))

    # ---- rto_denoise_launch_strips
    a, b = C.c_int(0), C.c_int(0)
    add("launch_strips/n 0", lambda: L.rto_denoise_launch_strips(0, 8, 8, C.byref(a), C.byref(b)))
    add("launch_strips/null out", lambda: L.rto_denoise_launch_strips(1, 8, 8, C.byref(a), None))

    # ---- a null handle, for every other entry of the three units
    info = _lib.CGuidanceNetInfo()
    two = _train_layers([(8, 8), (8, 8)])
    add("null/net_get_info", lambda: L.rto_guidance_net_get_info(None, C.byref(info)))
    add("null/net_forward", lambda: L.rto_guidance_net_forward(None, None, P, 1, 8, 8, P, P))
    add("null/net_forward_ex", lambda: L.rto_guidance_net_forward_ex(None, None, P, 1, 8, 8, P, P, 0))
    add("null/net_forward_culled", lambda: L.rto_guidance_net_forward_culled(None, None, P, 1, 8, 8, P, P, 0, P, 2, 0.0))
    add("null/net_forward_culled no marks", lambda: L.rto_guidance_net_forward_culled(None, None, P, 1, 8, 8, P, P, 0, None, 0, 0.0))
    add("null/net_forward_packed", lambda: L.rto_guidance_net_forward_packed(None, None, P, 1, 8, 8, 0))
    add("null/net_forward_packed_culled", lambda: L.rto_guidance_net_forward_packed_culled(None, None, P, 1, 8, 8, 0, P, 2, 0.0))
    add("null/filtering_packed", lambda: L.rto_filtering_packed(None, None, P, P + 16, 1, 8, 8))
    add("null/filtering_packed_culled", lambda: L.rto_filtering_packed_culled(None, None, P, P + 16, 1, 8, 8, P, 2, 0.0))
    add("null/filtering_packed_culled no marks", lambda: L.rto_filtering_packed_culled(None, None, P, P + 16, 1, 8, 8, None, 0, 0.0))
    add("null/filtering_culled", lambda: L.rto_filtering_culled(None, None, P, P, 8, 8, 1, P, P + 16, 0, P, 2, 0.0))
    add("null/denoise", lambda: L.rto_denoise(None, None, 1, 0, None))
    add("null/net_reserve", lambda: L.rto_guidance_net_reserve(None, 1, 8, 8))
    add("null/metrics_create", lambda: L.rto_metrics_create(0, None))
    add("null/metrics_compute", lambda: L.rto_metrics_compute(None, None, P, 0, P, 0, 1, 8, 8, 0, 0.0, P))
    add("null/metrics_compute_async", lambda: L.rto_metrics_compute_async(None, None, P, 0, P, 0, 1, 8, 8, 0, 0.0, P))
    add("null/image_read_png", lambda: L.rto_image_read_png(None, None, None, None, 0))
    add("null/train_create", lambda: L.rto_guidance_train_create(0, None))
    add("null/train_forward", lambda: L.rto_guidance_train_forward(None, None, P, two, 2, 4, 1, 8, 8, P, P, P))
    add("null/train_backward", lambda: L.rto_guidance_train_backward(None, None, P, P, P, P, two, 2, 4, 1, 8, 8))
    add("null/loss", lambda: L.rto_loss_forward_backward(None, None, P, P, 1, 8, 8, 0, P, P))
    add("null/image_write_png", lambda: L.rto_image_write_png(None, None, 8, 8))

    # ---- the *_create calls: without a device they say so; with one, a device index past the last is refused
    count = L.rto_device_count()
    dev, why = (0, "no device") if count <= 0 else (count, "device index")
    hh = C.c_void_p(0)
    net_ok = _net_layers([(8, 8), (8, 8)])
    add("create/net, " + why, lambda: L.rto_guidance_net_create_layers(net_ok, 2, 4, dev, C.byref(hh)))
    add("create/metrics, " + why, lambda: L.rto_metrics_create(dev, C.byref(hh)))
    add("create/train, " + why, lambda: L.rto_guidance_train_create(dev, C.byref(hh)))
    add("create/ctx, " + why, lambda: L.rto_ctx_create_batch(8, 8, 1, dev, C.byref(hh)))
    return cases


def gpu_cases(L):
    """[(label, call -> code)] of the refusals that need a live handle, in the order of the checks; the calls share the
    handles, so they run in this order.  A plain host pointer is offered to the metrics only: the library this table was recorded
    from told one from device memory there and nowhere else.  Shapes: 1 x 8 x 8 images, a 8 -> 8 -> 8 net with 4 levels (a "general" net, whose
    packed route is refused) and a 8 -> 32 -> 8 one (the reference shape, which has the packed route)."""
    import torch
    cases, keep = [], []
    add = lambda label, call: cases.append((label, call))  # noqa: E731
    dev = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731

    def host_ptr(nbytes):  # a 16-byte aligned plain host pointer
        a = np.zeros(nbytes + 16, np.uint8)
        keep.append(a)
        return a.ctypes.data + (-a.ctypes.data) % 16

    img, img2, out4 = dev(1, 11, 11, 4), dev(1, 11, 11, 4), dev(1, 4, dtype=torch.float64)  # (11: the smallest side with an SSIM window)
    ip, ip2, op = img.data_ptr(), img2.data_ptr(), out4.data_ptr()

    # ---- the metrics' validate chain
    m = C.c_void_p(0)
    assert L.rto_metrics_create(0, C.byref(m)) == 0
    res = np.zeros(4, np.float64)

    def compute(pred=ip, pf=0, truth=ip2, tf=0, n=1, H=11, W=11, flags=0, bg=0.0, out=res.ctypes.data):
        return lambda: L.rto_metrics_compute(m, None, pred, pf, truth, tf, n, H, W, flags, bg, out)

    def compute_async(out, pred=ip):
        return lambda: L.rto_metrics_compute_async(m, None, pred, 0, ip2, 0, 1, 11, 11, 0, 0.0, out)

    add("metrics/null pred", compute(pred=None))
    add("metrics/null out", compute(out=None))
    add("metrics/n 0", compute(n=0))
    add("metrics/pred format 5", compute(pf=5))
    add("metrics/truth format 7", compute(tf=7))
    add("metrics/flag bits 6", compute(flags=6))
    add("metrics/nan background", compute(flags=1, bg=float("nan")))
    add("metrics/2^31 pixels", compute(n=BIG[0], H=BIG[1], W=BIG[2]))
    add("metrics/pred misaligned", compute(pred=ip + 4))
    add("metrics/truth misaligned for bytes", compute(truth=ip2 + 2, tf=1))
    add("metrics/pred on the host", compute(pred=host_ptr(1024)))
    add("metrics/truth on the host", compute(truth=host_ptr(1024)))
    add("metrics_async/n 0", lambda: L.rto_metrics_compute_async(m, None, ip, 0, ip2, 0, 0, 8, 8, 0, 0.0, op))
    add("metrics_async/out misaligned", compute_async(op + 4))
    add("metrics_async/out on the host", compute_async(host_ptr(64)))
    add("metrics/ok", compute())

    # ---- the loss
    t = C.c_void_p(0)
    assert L.rto_guidance_train_create(0, C.byref(t)) == 0
    loss, grad = dev((), dtype=torch.float64), dev(1, 8, 8, 4)

    def lossf(pred=ip, truth=ip2, n=1, H=8, W=8, kind=0, lp=loss.data_ptr(), gp=grad.data_ptr()):
        return lambda: L.rto_loss_forward_backward(t, None, pred, truth, n, H, W, kind, lp, gp)

    add("loss/null truth", lossf(truth=None))
    add("loss/H 0", lossf(H=0))
    add("loss/kind 2", lossf(kind=2))
    add("loss/2^31 pixels", lossf(n=BIG[0], H=BIG[1], W=BIG[2]))
    add("loss/pred misaligned", lossf(pred=ip + 4))
    add("loss/loss misaligned", lossf(lp=loss.data_ptr() + 4))
    add("loss/ok", lossf())

    # ---- the training handle's forward and backward reach check_shape under their own names
    arr = (_lib.CGuidanceTrainLayer * 2)()
    for l in arr:
        w, b = dev(8, 8, 3, 3), dev(8)
        gw, gb = dev(8, 8, 3, 3), dev(8)
        keep.extend([w, b, gw, gb])
        l.weight, l.bias, l.grad_weight, l.grad_bias, l.cin, l.cout = w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr(), 8, 8
    aux, maps, acts = dev(1, 8, 8, 8), dev(1, 4, 8, 8), dev(1 << 16)
    ap, mp, cp = aux.data_ptr(), maps.data_ptr(), acts.data_ptr()
    add("train_forward/n 0", lambda: L.rto_guidance_train_forward(t, None, ap, arr, 2, 4, 0, 8, 8, cp, mp, mp))
    add("train_forward/levels 3", lambda: L.rto_guidance_train_forward(t, None, ap, arr, 2, 3, 1, 8, 8, cp, mp, mp))
    add("train_backward/five layers", lambda: L.rto_guidance_train_backward(t, None, mp, mp, ap, cp, arr, 5, 4, 1, 8, 8))

    def no_grad():
        saved, arr[1].grad_bias = arr[1].grad_bias, None
        rc = L.rto_guidance_train_backward(t, None, mp, mp, ap, cp, arr, 2, 4, 1, 8, 8)
        arr[1].grad_bias = saved
        return rc
    add("train_backward/null grad_bias", no_grad)

    # ---- the packed route: a general net refuses it; the reference shape checks extents, marks and devices
    general, net = C.c_void_p(0), C.c_void_p(0)
    assert L.rto_guidance_net_create_layers(_net_layers([(8, 8), (8, 8)]), 2, 4, 0, C.byref(general)) == 0
    assert L.rto_guidance_net_create_layers(_net_layers([(8, 32), (32, 8)]), 2, 4, 0, C.byref(net)) == 0
    marks = dev(8, dtype=torch.int32)  # an 8 x 8 frame has one tile: one word of marks and the keep-all word
    kp = marks.data_ptr()
    add("general/reserve", lambda: L.rto_guidance_net_reserve(general, 1, 8, 8))
    add("general/forward_packed", lambda: L.rto_guidance_net_forward_packed(general, None, ap, 1, 8, 8, 0))
    add("general/filtering_packed", lambda: L.rto_filtering_packed(general, None, ip, ip2, 1, 8, 8))
    add("general/filtering_packed_culled", lambda: L.rto_filtering_packed_culled(general, None, ip, ip2, 1, 8, 8, kp, 2, 0.0))
    add("general/forward_ex sparse", lambda: L.rto_guidance_net_forward_ex(general, None, ap, 1, 8, 8, mp, mp, 4))
    add("general/forward_culled sparse", lambda: L.rto_guidance_net_forward_culled(general, None, ap, 1, 8, 8, mp, mp, 4, kp, 2, 0.0))

    def packed(n=1, H=8, W=8, i=ip, o=ip2, h=net):
        return lambda: L.rto_filtering_packed(h, None, i, o, n, H, W)

    def packed_culled(n=1, H=8, W=8, i=ip, o=ip2, k=kp, words=2):
        return lambda: L.rto_filtering_packed_culled(net, None, i, o, n, H, W, k, words, 0.0)

    add("packed/in == out", packed(o=ip))
    add("packed/no maps yet", packed())
    add("packed_culled/no maps yet", packed_culled())
    add("forward_packed/n 0", lambda: L.rto_guidance_net_forward_packed(net, None, ap, 0, 8, 8, 0))
    add("forward_packed/sparse without marks", lambda: L.rto_guidance_net_forward_packed(net, None, ap, 1, 8, 8, 4 | 2))
    add("forward_packed_culled/words", lambda: L.rto_guidance_net_forward_packed_culled(net, None, ap, 1, 8, 8, 0, kp, 3, 0.0))
    add("forward_packed_culled/sparse without rgba", lambda: L.rto_guidance_net_forward_packed_culled(net, None, ap, 1, 8, 8, 4, kp, 2, 0.0))
    add("forward_packed/ok", lambda: L.rto_guidance_net_forward_packed(net, None, ap, 1, 8, 8, 0))
    add("packed/two images", packed(n=2))
    add("packed/another height", packed(H=16))
    add("packed_culled/another width", packed_culled(W=16))
    add("packed_culled/words", packed_culled(words=1))

    # ---- the marks of the fp32-plane entries
    def fwd_culled(k=kp, words=2, h=net, n=1):
        return lambda: L.rto_guidance_net_forward_culled(h, None, ap, n, 8, 8, mp, mp, 0, k, words, 0.0)

    maps2 = dev(1, 4, 8, 8)
    mp2 = maps2.data_ptr()

    def filt_culled(k=kp, words=2, mode=0, i=ip, o=ip2, H=8):
        return lambda: L.rto_filtering_culled(net, None, mp, mp2, H, 8, 1, i, o, mode, k, words, 0.0)

    add("forward_culled/n 0", fwd_culled(n=0))
    add("forward_culled/words", fwd_culled(words=5))
    add("filtering_culled/H 0", filt_culled(H=0))
    add("filtering_culled/in == out", filt_culled(o=ip))
    add("filtering_culled/mode 3", filt_culled(mode=3))
    add("filtering_culled/words", filt_culled(words=0))
    add("filtering_culled/no marks, mode 3", filt_culled(k=None, mode=3))

    # ---- a reserve that grows the packed scratch leaves no maps behind
    add("reserve/same size", lambda: L.rto_guidance_net_reserve(net, 1, 8, 8))
    add("packed/still there", packed())
    add("reserve/grows", lambda: L.rto_guidance_net_reserve(net, 2, 16, 16))
    add("packed/gone after the growing reserve", packed())
    add("packed_culled/gone after the growing reserve", packed_culled())

    def free():
        torch.cuda.synchronize()
        L.rto_metrics_free(m)
        L.rto_guidance_train_free(t)
        L.rto_guidance_net_free(general)
        L.rto_guidance_net_free(net)
        keep.extend([img, img2, out4, loss, grad, aux, maps, acts, marks, maps2])
    return cases, free


def _run(L, cases):
    got = []
    for label, call in cases:
        rc = call()
        got.append((label, rc, L.rto_last_error().decode() if rc != 0 else ""))
    return got


def _check(got):
    wrong = ["%s: (%d, %r), recorded (%d, %r)" % ((label, rc, text) + EXPECTED[label]) for label, rc, text in got
             if label not in EXPECTED or EXPECTED[label] != (rc, text)]
    assert not wrong, "\n".join(wrong)


def test_refusals_decided_on_the_host_keep_their_codes_and_texts():
    L = _lib.lib()
    got = _run(L, host_cases(L))
    assert all(rc != 0 for _label, rc, _text in got)
    _check(got)


@pytest.mark.gpu
def test_refusals_of_live_handles_keep_their_codes_and_texts():
    L = _lib.lib()
    cases, free = gpu_cases(L)
    try:
        got = _run(L, cases)
    finally:
        free()
    assert all((rc == 0) == label.endswith(("/ok", "/same size", "/still there", "/grows")) for label, rc, _text in got), got
    _check(got)


if __name__ == "__main__":  # record: print the table entries of the library RTO_LIB names
    L = _lib.lib()
    if sys.argv[1:] == ["gpu"]:
        cases, free = gpu_cases(L)
        rows = _run(L, cases)
        free()
    else:
        rows = _run(L, host_cases(L))
    for label, rc, text in rows:
        print("    %r: (%d, %r)," % (label, rc, text))
