"""Host-side mirror of the reference's render operator interface, over the C ABI (include/rto.h).

Same names, argument meaning and error behaviour as the reference (paths relative to
/root/reference):
    RenderOptions    renderer/include/volrend/render_options.hpp:13-78
    N3Tree           renderer/include/volrend/n3tree.hpp, src/n3tree.cpp:111-362
    Camera           renderer/include/volrend/camera.hpp (transform = glm::mat4x3, column-major)
    RenderContext    renderer/include/volrend/render_context.hpp:14-214 (rng, aux, images, Timer)
    launch_renderer  renderer/include/volrend/cuda/renderer_kernel.hpp:11-16
    filtering        denoiser/extension/filtering.h:7-13

All pixel work runs in the HIP kernels behind librto.so; this module only marshals arguments.
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from ._lib import CCamera, CGridParams, COptions, LayerParams, CQueryOut, CRays, CRaysOut, CTreeInfo, RtoError, check, lib

SUPPORTED_SPP = (1, 2, 3, 4, 6, 8, 16, 32)  # volrend.cu:266-278
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_FAST = 0, 1, 2
GRID_MERGE = 1  # RTO_GRID_MERGE (draw_grid_layers(merge=True))
DEPTH_BATCHED = 2  # RTO_DEPTH_BATCHED (RenderContext.enable_depth(batched=True))
AUX_CHANNELS = 8  # render_context.hpp:23
_FORMAT_NAMES = {0: "RGBA", 1: "SH", 2: "SG", 3: "ASG"}


def _stream_ptr(stream):
    """None -> default stream; int -> raw hipStream_t; torch.cuda.Stream -> its handle."""
    if stream is None:
        return C.c_void_p(0)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    raise TypeError("stream must be None, an int handle or a torch.cuda.Stream")


class RenderOptions:
    """render_options.hpp:13-78.  Field names and defaults are the reference's."""

    _JSON_KEYS = ("step_size", "sigma_thresh", "stop_thresh", "background_brightness", "show_grid",
                  "grid_max_depth", "enable_probe", "probe", "probe_disp_size", "denoise", "spp")
    SPP_DEFAULT = 4  # render_options.hpp:57

    def __init__(self, **kw):
        c = COptions()
        lib().rto_options_default(C.byref(c))
        self._load(c)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError("RenderOptions has no field '%s'" % k)
            setattr(self, k, v)

    def _load(self, c):
        self.step_size = c.step_size
        self.sigma_thresh = c.sigma_thresh
        self.stop_thresh = c.stop_thresh
        self.background_brightness = c.background_brightness
        self.render_bbox = list(c.render_bbox)
        self.basis_minmax = list(c.basis_minmax)
        self.rot_dirs = list(c.rot_dirs)
        self.show_grid = bool(c.show_grid)
        self.grid_max_depth = c.grid_max_depth
        self.render_depth = bool(c.render_depth)
        self.enable_probe = bool(c.enable_probe)
        self.probe = list(c.probe)
        self.probe_disp_size = c.probe_disp_size
        self.denoise = bool(c.denoise)
        self.spp = c.spp

    @classmethod
    def from_json(cls, path):
        """`options = json::parse(f)` (main_headless.cpp:459-464): all 11 keys are required."""
        c = COptions()
        check(lib().rto_options_from_json_file(os.fsencode(path), C.byref(c)))
        o = cls.__new__(cls)
        o._load(c)
        return o

    @classmethod
    def from_json_text(cls, text):
        c = COptions()
        check(lib().rto_options_from_json(text.encode("utf-8"), C.byref(c)))
        o = cls.__new__(cls)
        o._load(c)
        return o

    def to_json(self):
        return json.dumps({k: getattr(self, k) for k in self._JSON_KEYS}, indent=2, sort_keys=True)

    def to_c(self):
        c = COptions()
        c.step_size, c.sigma_thresh, c.stop_thresh = self.step_size, self.sigma_thresh, self.stop_thresh
        c.background_brightness = self.background_brightness
        for i in range(6):
            c.render_bbox[i] = self.render_bbox[i]
        for i in range(2):
            c.basis_minmax[i] = int(self.basis_minmax[i])
        for i in range(3):
            c.rot_dirs[i] = self.rot_dirs[i]
            c.probe[i] = self.probe[i]
        c.show_grid, c.grid_max_depth = int(self.show_grid), int(self.grid_max_depth)
        c.render_depth, c.enable_probe = int(self.render_depth), int(self.enable_probe)
        c.probe_disp_size = int(self.probe_disp_size)
        c.denoise, c.spp = int(self.denoise), int(self.spp)
        return c


class N3Tree:
    """Device-resident PlenOctree.  `N3Tree(path)` = N3Tree::open + load_cuda
    (n3tree.cpp:111-154, n3tree.cu:9-41)."""

    def __init__(self, path=None, device=0, quant_direct=False, compact=False, keep_reference=False, compact_records=False,
                 no_culling=False):
        self._h = C.c_void_p(0)
        self.device = device
        self.quant_direct = bool(quant_direct)  # render a quantised tree from its codebooks (no expansion)
        self.compact = bool(compact)            # RTO_TREE_COMPACT: no aligned copy of the SH coefficients for shading
        self.keep_reference = bool(keep_reference)  # RTO_TREE_KEEP_REFERENCE: child[] / data[] stay resident
        self.compact_records = bool(compact_records)  # RTO_TREE_COMPACT_RECORDS: coefficient records for hittable leaves only
        self.no_culling = bool(no_culling)  # RTO_TREE_NO_CULLING: no empty-space culling cells
        if path is not None:
            self.open(path)

    def _flags(self):
        return ((1 if self.quant_direct else 0) | (2 if self.compact else 0) | (4 if self.keep_reference else 0)
                | (8 if self.compact_records else 0) | (16 if self.no_culling else 0))

    def open(self, path):
        self.free()
        h = C.c_void_p(0)
        check(lib().rto_tree_load_npz_ex(os.fsencode(path), self.device, self._flags(), C.byref(h)))
        self._h = h
        self._refresh()

    @classmethod
    def from_arrays(cls, child, data, scale, offset, data_format="", device=0, compact=False, keep_reference=False,
                    compact_records=False, no_culling=False, extra_data=None):
        """child int32 [capacity,N,N,N]; data float16 (or uint16 bits) [capacity,N,N,N,data_dim];
        scale = invradius3, offset (n3tree.cpp:257-267).  extra_data: the lobes of an SG / ASG tree, float32
        [basis_dim, 4] (SG) / [basis_dim, 11] (ASG) or flat (n3tree.cpp:350-353); ignored for SH / RGBA trees."""
        child = np.ascontiguousarray(child, dtype=np.int32)
        data = np.ascontiguousarray(data)
        if data.dtype == np.float16:
            data = data.view(np.uint16)
        if data.dtype != np.uint16:
            raise RtoError(-6, "data must be stored in half precision")  # n3tree.cpp:345
        if child.ndim != 4 or data.ndim != 5:
            raise RtoError(-1, "child must be [capacity,N,N,N] and data [capacity,N,N,N,data_dim]")
        cap, N, dd = child.shape[0], child.shape[1], data.shape[-1]
        sc = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(scale, np.float32), (3,))])
        of = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(offset, np.float32), (3,))])
        t = cls(device=device, compact=compact, keep_reference=keep_reference, compact_records=compact_records,
                no_culling=no_culling)
        extra_ptr, extra_n = None, 0
        if extra_data is not None:
            extra_data = np.asarray(extra_data)
            if extra_data.dtype != np.float32:  # (the reference reinterprets the bytes as float: n3tree.cpp:351)
                raise RtoError(-6, "extra_data must be float32")
            extra_data = np.ascontiguousarray(extra_data)
            extra_ptr, extra_n = C.c_void_p(extra_data.ctypes.data), extra_data.size
        h = C.c_void_p(0)
        check(lib().rto_tree_from_arrays_extra(C.c_void_p(child.ctypes.data), C.c_void_p(data.ctypes.data), cap, N, dd,
                                               data_format.encode("ascii"), sc, of, device, t._flags(), extra_ptr, extra_n,
                                               C.byref(h)))
        t._h = h
        t._refresh()
        return t

    def _refresh(self):
        info = CTreeInfo()
        check(lib().rto_tree_get_info(self._h, C.byref(info)))
        self.capacity, self.N, self.data_dim = info.capacity, info.N, info.data_dim
        self.basis_dim = info.basis_dim
        self.data_format = _FORMAT_NAMES.get(info.format, "UNKNOWN") + (str(info.basis_dim) if info.basis_dim != -1 else "")
        self.scale = np.array(info.scale, np.float32)
        self.offset = np.array(info.offset, np.float32)
        self.use_ndc = bool(info.use_ndc)
        self.ndc_width, self.ndc_height, self.ndc_focal = info.ndc_width, info.ndc_height, info.ndc_focal
        self.max_depth = info.max_depth
        self.device_bytes = info.device_bytes
        self.wide_nodes = info.wide_nodes

    def set_ndc(self, width, height, focal):
        """main_headless.cpp:400-405: tree.use_ndc = true; ndc_width/height/focal."""
        check(lib().rto_tree_set_ndc(self._h, float(width), float(height), float(focal)))
        self._refresh()

    def query(self, points, values=True, sigma=False, level=False, cube=False, stream=None):
        """rto_tree_query: what the tree holds at `points`, a contiguous float32 CUDA tensor [n, 3] in world space on the tree's
        device (a numpy array is copied over).  Returns a dict of torch tensors on that device with the outputs asked for:
        "values" [n, data_dim] float32 (the leaf's data[] row, last = sigma), "sigma" [n], "level" [n] int32 (-1: a point with a
        non-finite coordinate, which is not answered: zeros elsewhere), "cube" [n, 4] (the leaf's min corner in tree coordinates
        and its side).  No NDC warp is applied.  Asynchronous on `stream` (default: torch's current stream); no sync."""
        import torch
        device = torch.device("cuda", self.device)
        if not hasattr(points, "shape") or len(points.shape) != 2:
            raise RtoError(-1, "points must be a contiguous float32 tensor of shape [n, 3]")
        n = int(points.shape[0])
        pts = _ray_tensor(points, "points", 3, n, device)
        res = {}
        if values:
            res["values"] = torch.empty((n, self.data_dim), dtype=torch.float32, device=device)
        if sigma:
            res["sigma"] = torch.empty((n,), dtype=torch.float32, device=device)
        if level:
            res["level"] = torch.empty((n,), dtype=torch.int32, device=device)
        if cube:
            res["cube"] = torch.empty((n, 4), dtype=torch.float32, device=device)
        q = CQueryOut()
        for k, t in res.items():
            setattr(q, k, t.data_ptr() if n > 0 else None)
        if stream is None:
            stream = torch.cuda.current_stream(device)
        check(lib().rto_tree_query(self._h, C.c_void_p(pts.data_ptr()) if n > 0 else None, n, C.byref(q), _stream_ptr(stream)))
        return res

    def is_data_loaded(self):
        return bool(self._h)

    def free(self):
        if getattr(self, "_h", None):
            lib().rto_tree_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Camera:
    """camera.hpp: width, height, fx, fy and `transform`, a glm::mat4x3 (4 columns of 3): columns
    0..2 are the camera axes, column 3 the centre.  `transform` here is a float32 [4,3] array whose
    row c is glm column c, so `.reshape(-1)` is the 12-float column-major block the kernel reads
    (common.cuh:29-44)."""

    def __init__(self, width=800, height=800, fx=1111.11, fy=-1.0):
        self.width, self.height = int(width), int(height)
        self.fx = float(fx)
        self.fy = float(fy) if fy > 0 else float(fx)
        self.transform = np.zeros((4, 3), np.float32)
        self.transform[0, 0] = self.transform[1, 1] = self.transform[2, 2] = 1.0

    def set_c2w(self, m):
        """m: row-major 3x4 / 4x4 camera-to-world (blender `transform_matrix`); transposed into the
        column-major layout like main_headless.cpp:262-268."""
        m = np.asarray(m, np.float32)
        self.transform = np.ascontiguousarray(m[:3, :4].T)

    def to_c(self):
        c = CCamera()
        c.width, c.height, c.fx, c.fy = self.width, self.height, self.fx, self.fy
        flat = np.asarray(self.transform, np.float32).reshape(-1)
        if flat.size != 12:
            raise RtoError(-1, "Camera.transform must hold 12 floats")
        for i in range(12):
            c.transform[i] = float(flat[i])
        return c


class _DevArray:
    """Zero-copy view of a device buffer for torch.as_tensor / cupy (CUDA array interface v2)."""

    def __init__(self, ptr, shape, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


class Timer:
    """RenderContext::Timer (render_context.hpp:122-213): three event pairs on the render stream,
    FPS = 1000 / (render + torch + filter) over the recorded frames."""

    RENDER, TORCH, FILTER = 0, 1, 2

    def __init__(self, ctx):
        self._ctx = ctx

    def reset(self, stream=None):
        check(lib().rto_timer_reset(self._ctx._h, _stream_ptr(stream)))

    def render_start(self): check(lib().rto_timer_start(self._ctx._h, 0))
    def render_stop(self): check(lib().rto_timer_stop(self._ctx._h, 0))
    def torch_start(self): check(lib().rto_timer_start(self._ctx._h, 1))
    def torch_stop(self): check(lib().rto_timer_stop(self._ctx._h, 1))
    def filter_start(self): check(lib().rto_timer_start(self._ctx._h, 2))
    def filter_stop(self): check(lib().rto_timer_stop(self._ctx._h, 2))

    def record(self, denoise):
        check(lib().rto_timer_record(self._ctx._h, int(bool(denoise))))

    def stats(self):
        ms = (C.c_float * 3)()
        fps, n = C.c_float(0), C.c_int(0)
        check(lib().rto_timer_report(self._ctx._h, ms, C.byref(fps), C.byref(n)))
        return {"render_ms": ms[0], "torch_ms": ms[1], "filter_ms": ms[2],
                "all_ms": ms[0] + ms[1] + ms[2], "fps": fps.value, "frames": n.value}

    def report(self):
        s = self.stats()
        print("render: %.10f ms per frame" % s["render_ms"])
        print("torch:  %.10f ms per frame" % s["torch_ms"])
        print("filter: %.10f ms per frame" % s["filter_ms"])
        print("all:    %.10f ms per frame" % s["all_ms"])
        print("FPS:    %.10f" % s["fps"])
        return s


class RenderContext:
    """render_context.hpp:14-214 with offscreen = true: rng = pcg32(20230418), aux_buffer
    [8,H,W] f32, noisy image and final image [H,W,4] f32 (linear device memory instead of
    cudaArray + surface/texture objects)."""

    CHANNELS = AUX_CHANNELS

    def __init__(self, width, height, device=0, frames=1):
        self._h = C.c_void_p(0)
        h = C.c_void_p(0)
        check(lib().rto_ctx_create_batch(int(width), int(height), int(frames), int(device), C.byref(h)))
        self._h = h
        self.width, self.height, self.device, self.frames = int(width), int(height), int(device), int(frames)
        self.offscreen = True
        self._layers = (None, None)  # the tensors handed to set_layers: kept referenced while the context may read them
        self._timer = Timer(self)

    # rng (pcg32.h)
    def rng_seed(self, initstate=20230418, initseq=1):
        lib().rto_ctx_rng_seed(self._h, initstate, initseq)

    def rng_advance(self, delta=1 << 32):
        """ctx.rng.advance() (main_headless.cpp:478,506): default jump 2^32."""
        lib().rto_ctx_rng_advance(self._h, delta)

    def rng_set(self, state, inc):
        lib().rto_ctx_rng_set(self._h, state, inc)

    def rng_get(self):
        s, i = C.c_uint64(0), C.c_uint64(0)
        lib().rto_ctx_rng_get(self._h, C.byref(s), C.byref(i))
        return s.value, i.value

    def select_frame(self, frame):
        """frame slot the single-frame entry points, accessors and downloads refer to"""
        check(lib().rto_ctx_select_frame(self._h, int(frame)))

    def batch_views(self):
        """zero-copy views over ALL frame slots: aux [F,8,H,W], noisy [F,H,W,4], image [F,H,W,4]"""
        sel = lib().rto_ctx_selected_frame(self._h)  # (the selection is the caller's: left as found)
        self.select_frame(0)
        F, H, W = self.frames, self.height, self.width
        views = (_DevArray(self.aux_ptr, (F, AUX_CHANNELS, H, W), self), _DevArray(self.noisy_ptr, (F, H, W, 4), self),
                 _DevArray(self.image_ptr, (F, H, W, 4), self))
        self.select_frame(sel)
        return views

    def set_kernel(self, kernel):
        check(lib().rto_ctx_set_kernel(self._h, int(kernel)))

    def set_layers(self, depth=None, color=None):
        """rto_ctx_set_layers (RenderContext::offscreen = false): launch_renderer / launch_renderer_batch stop every pixel's ray at
        `depth` [frames, H, W] (world distance along the unit direction; +inf = no limit) and composite the volume over `color`
        [frames, H, W, 4] (rgb read) instead of the constant background.  Contiguous float32 torch tensors on the context's device
        (numpy arrays are copied over); either may be None, both None restores the offscreen behaviour.  Frame slot k reads plane
        k.  The tensors stay referenced by the context; they must not be the context's own buffers."""
        import torch
        device = torch.device("cuda", self.device)
        n = self.frames * self.height * self.width
        d = None if depth is None else _ray_tensor(_as_planes(depth, (self.frames, self.height, self.width)), "depth", 0, n, device)
        c = None if color is None else _ray_tensor(_as_planes(color, (self.frames, self.height, self.width, 4)), "color", 4, n, device)
        check(lib().rto_ctx_set_layers(self._h, C.c_void_p(d.data_ptr()) if d is not None else None,
                                       C.c_void_p(c.data_ptr()) if c is not None else None))
        self._layers = (d, c)
        self.offscreen = d is None and c is None

    def layers(self):
        """(depth pointer or None, colour pointer or None) the context holds (rto_ctx_layers)"""
        d, c = C.c_void_p(None), C.c_void_p(None)
        check(lib().rto_ctx_layers(self._h, C.byref(d), C.byref(c)))
        return d.value, c.value

    def _show_layers(self, name, draw, target, cams, params, refusal=None, **kw):
        """show_meshes / show_grid: draw(...) for one camera per frame slot into the depth and colour tensors the context keeps
        alive (allocated once), then bound with set_layers.  refusal: an error to raise after the camera check"""
        import torch
        if isinstance(cams, Camera):
            cams = [cams]
        if len(cams) != self.frames:
            raise RtoError(-1, "%s: %d cameras for a context of %d frame slots" % (name, len(cams), self.frames))
        if refusal is not None:
            raise refusal
        keep = getattr(self, "_grid_layers", None)
        if keep is None:
            device = torch.device("cuda", self.device)
            keep = (torch.empty((self.frames, self.height, self.width), dtype=torch.float32, device=device),
                    torch.empty((self.frames, self.height, self.width, 4), dtype=torch.float32, device=device))
            self._grid_layers = keep
        draw(target, cams, params, depth=keep[0], color=keep[1], **kw)
        self.set_layers(keep[0], keep[1])
        return keep

    def show_meshes(self, meshset, cams, options, params=None, stream=None, tree=None):
        """The reference's mesh pass for this context: draws `meshset` (meshes.draw_mesh_layers; `params`: a MeshParams instead of
        the defaults taken from `options`) for `cams` -- one Camera per frame slot -- into the depth and colour tensors the
        context keeps alive (the ones show_grid uses) and binds them with set_layers.  For meshes AND the grid call show_meshes
        first, then show_grid(..., merge=True): the reference's draw order.  `tree`: the tree the frames will be rendered from;
        meshes live in world space, so an NDC tree is refused with RTO_E_UNSUPPORTED, as the grid refuses it.  Returns (depth,
        color)."""
        from .meshes import MeshParams, draw_mesh_layers
        ndc = tree is not None and tree.use_ndc
        return self._show_layers("show_meshes", draw_mesh_layers, meshset, cams, MeshParams(options) if params is None else params,
                                 RtoError(-3, "show_meshes: meshes are in world space: over an NDC tree the depth measure differs") if ndc else None,
                                 stream=stream)

    def show_grid(self, tree, cams, options, params=None, stream=None, merge=False):
        """RenderOptions.show_grid for this context: draws the octree grid of `tree` cut off at options.grid_max_depth
        (draw_grid_layers; `params`: a GridParams instead of the defaults taken from `options`) for `cams` -- one Camera per frame
        slot, or a single Camera for a single-slot context -- into a depth and a colour tensor the context keeps alive, and binds
        them with set_layers: the launches that follow render over the grid.  Returns (depth [frames, H, W], color [frames, H, W,
        4]).  set_layers() with no arguments restores the offscreen behaviour.  merge=True (after show_meshes): the lines are depth-tested
        against what the layers hold (RTO_GRID_MERGE) instead of replacing them."""
        return self._show_layers("show_grid", draw_grid_layers, tree, cams, GridParams(options) if params is None else params,
                                 merge=merge, stream=stream)

    def enable_depth(self, on=True, batched=False):
        """rto_ctx_enable_depth: launch_renderer / launch_renderer_batch also write depth and t_near [frames, H, W] (include/rto.h
        "depth outputs").  Batches are then rendered frame by frame through the single-frame kernels -- or, with batched=True
        (RTO_DEPTH_BATCHED), through the persistent kernels like any other batch: the same bytes, tile marks and lean outputs kept.
        Calling it again on an enabled context switches between the two without touching the planes."""
        check(lib().rto_ctx_enable_depth(self._h, (DEPTH_BATCHED if batched else 1) if on else 0))

    def depth_enabled(self):
        return bool(lib().rto_ctx_depth_enabled(self._h))

    def depth_mode(self):
        """0 = no depth outputs, 1 = batches frame by frame, DEPTH_BATCHED (2) = batches through the persistent kernels"""
        return int(lib().rto_ctx_depth_enabled(self._h))

    def depth_view(self):
        """zero-copy view of the selected slot's depth plane [H, W]; None while disabled"""
        p = lib().rto_ctx_depth(self._h)
        return _DevArray(p, (self.height, self.width), self) if p else None

    def t_near_view(self):
        p = lib().rto_ctx_t_near(self._h)
        return _DevArray(p, (self.height, self.width), self) if p else None

    def download_depth(self, stream=None):
        """(depth, t_near) of the selected slot, float32 [H, W] numpy arrays"""
        d = np.empty((self.height, self.width), np.float32)
        t = np.empty((self.height, self.width), np.float32)
        check(lib().rto_ctx_download_depth(self._h, _stream_ptr(stream), C.c_void_p(d.ctypes.data), C.c_void_p(t.ctypes.data)))
        return d, t

    def timer(self):
        return self._timer

    def set_tuning(self, key, value):
        """performance knobs ("strip_rows", "refill", "tile_order", "xcd_queues", "tile_major", "tile_block", "blocks_per_cu", "cull", "cull_cubes", "cull_single");
        results never change"""
        check(lib().rto_ctx_set_tuning(self._h, key.encode("ascii"), int(value)))

    def set_lean_outputs(self, on=True):
        """rto_ctx_set_lean_outputs: batched launches with denoise on store the noisy image as (r, g, b, alpha) and no aux
        planes -- 16 instead of 48 bytes per pixel; consumers: FusedGuidanceNet(..., rgba=True) on noisy_ptr, denoise().
        on = 2 (sparse): and nothing at all for the pixels of culled tiles; consumers additionally pass sparse=True + the marks"""
        check(lib().rto_ctx_set_lean_outputs(self._h, int(on)))

    def frames_lean_level(self, first=0, n=1):
        return lib().rto_ctx_frames_lean_level(self._h, int(first), int(n))  # 0 full / 1 lean / 2 sparse; -1: a mixed range

    def frames_are_lean(self, first=0, n=1):
        return lib().rto_ctx_frames_are_lean(self._h, int(first), int(n)) == 1  # (0: all full; -1: a mixed range)

    def kernel_timing(self, on=True):
        """HIP-event timing of the traversal / shading kernels of launch_renderer_batch"""
        check(lib().rto_ctx_kernel_timing(self._h, int(bool(on))))

    def kernel_timing_read(self):
        g, t, s, n = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        check(lib().rto_ctx_kernel_timing_read3(self._h, C.byref(g), C.byref(t), C.byref(s), C.byref(n)))
        return {"raygen_ms": g.value, "traverse_ms": t.value, "shade_ms": s.value, "launches": n.value}

    def queue_stats(self):
        """(tile slots marched, tile slots in all) of the last batched launch: the rest were culled as provably empty"""
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().rto_ctx_queue_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tile_marks(self):
        """(device pointer, words per frame, first slot, frames, background) of the tile marks the last batched launch left
        (rto_ctx_tile_marks) -- what FusedGuidanceNet.filter_packed(cull=...) takes; None after a single-frame launch"""
        p, w, s0, n, bg = C.c_void_p(None), C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        if lib().rto_ctx_tile_marks(self._h, C.byref(p), C.byref(w), C.byref(s0), C.byref(n), C.byref(bg)) != 0:
            return None
        return p.value, w.value, s0.value, n.value, bg.value

    def enable_stats(self, on=True, marched=False):
        """Work counters for the roofline's algorithmic byte count (never in a timed run).  marched: also count the frame as
        the batched path works through it (get_march_stats) -- select a slot of the last batched launch and re-render its pose."""
        check(lib().rto_ctx_enable_stats(self._h, 2 if (on and marched) else int(bool(on))))

    def get_march_stats(self, reset=True, stream=None):
        out = (C.c_uint64 * 8)()
        check(lib().rto_ctx_get_march_stats(self._h, _stream_ptr(stream), out, int(bool(reset))))
        keys = ("rays", "steps", "grid_loads", "node_loads", "hit_entries", "rays_in_box", "wide_loads")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def get_stats(self, reset=True, stream=None):
        out = (C.c_uint64 * 6)()
        check(lib().rto_ctx_get_stats(self._h, _stream_ptr(stream), out, int(bool(reset))))
        keys = ("rays", "rays_in_box", "steps", "levels", "hit_leaves", "hit_rays")
        return {k: int(v) for k, v in zip(keys, out)}

    # device pointers / zero-copy views
    @property
    def aux_ptr(self): return lib().rto_ctx_aux(self._h)
    @property
    def noisy_ptr(self): return lib().rto_ctx_noisy(self._h)
    @property
    def image_ptr(self): return lib().rto_ctx_image(self._h)

    def aux_view(self): return _DevArray(self.aux_ptr, (1, AUX_CHANNELS, self.height, self.width), self)
    def noisy_view(self): return _DevArray(self.noisy_ptr, (self.height, self.width, 4), self)
    def image_view(self): return _DevArray(self.image_ptr, (self.height, self.width, 4), self)

    # host copies (main_headless.cpp:508-540)
    def download_aux(self, stream=None):
        out = np.empty((AUX_CHANNELS, self.height, self.width), np.float32)
        check(lib().rto_ctx_download_aux(self._h, _stream_ptr(stream), C.c_void_p(out.ctypes.data)))
        return out

    def download_image(self, noisy=False, stream=None):
        out = np.empty((self.height, self.width, 4), np.float32)
        check(lib().rto_ctx_download_image(self._h, _stream_ptr(stream), int(noisy), C.c_void_p(out.ctypes.data)))
        return out

    def download_rgba8(self, noisy=False, stream=None):
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().rto_ctx_download_rgba8(self._h, _stream_ptr(stream), int(noisy), C.c_void_p(out.ctypes.data)))
        return out

    def metrics(self, truth, n=1, noisy=False, over_background=None, stream=None):
        """MSE, PSNR, SMAPE and SSIM (metrics.ImageMetrics) of the image -- or the noisy image -- of the n frame slots from the
        selected one against `truth`, a device tensor [n,H,W,4] (or [H,W,4]), float32 or uint8, read in place.  Returns a list
        of n FrameMetrics; synchronises `stream`."""
        from .metrics import ImageMetrics
        sel = lib().rto_ctx_selected_frame(self._h)
        if n < 1 or sel + n > self.frames:
            raise RtoError(-1, "metrics: %d frames from slot %d of a context of %d" % (n, sel, self.frames))
        if getattr(self, "_metrics", None) is None:
            self._metrics = ImageMetrics(self.device)
        pred = _DevArray(self.noisy_ptr if noisy else self.image_ptr, (n, self.height, self.width, 4), self)
        return self._metrics.compute(pred, truth, over_background=over_background, stream=stream)

    def freeResource(self):
        if getattr(self, "_metrics", None) is not None:
            self._metrics.free()
            self._metrics = None
        if getattr(self, "_h", None):
            lib().rto_ctx_free(self._h)
            self._h = C.c_void_p(0)

    free = freeResource

    def __del__(self):
        try:
            self.freeResource()
        except Exception:
            pass


def launch_renderer(tree, cam, options, ctx, stream=None, offscreen=True):
    """volrend::launch_renderer(tree, cam, options, ctx, stream, offscreen)
    (renderer_kernel.hpp:11-16).  Asynchronous on `stream`.  Unsupported spp raises like the
    reference's std::runtime_error("spp == N not supported.") (volrend.cu:275-277).  offscreen=False renders over the
    context's depth / colour layers (RenderContext.set_layers: the reference's surf_obj_depth / surf_obj) and raises when the
    context has none; a context with layers composites over them whatever `offscreen` says (rto_ctx_set_layers)."""
    if not offscreen and ctx.layers() == (None, None):
        raise RtoError(-3, "offscreen=False needs a depth / colour layer on the context (RenderContext.set_layers); GL interop is out of scope")
    cc, co = cam.to_c(), options.to_c()
    check(lib().rto_launch_renderer(tree._h, C.byref(cc), C.byref(co), ctx._h, _stream_ptr(stream)))


def launch_renderer_batch(tree, cams, options, ctx, stream=None, rng_jumps=None):
    """n frames in one launch of the persistent ray-queue kernel (rto_launch_renderer_batch):
    cams[f] -> frame slot f, RNG = ctx.rng advanced by rng_jumps[f] (default f) jumps of 2^32.
    Bit-identical to the reference's frame loop `launch_renderer(...); ctx.rng.advance()`."""
    n = len(cams)
    arr = (CCamera * n)(*[c.to_c() for c in cams])
    jumps = None
    if rng_jumps is not None:
        jumps = (C.c_int64 * n)(*[int(j) for j in rng_jumps])
    co = options.to_c()
    check(lib().rto_launch_renderer_batch(tree._h, arr, jumps, n, C.byref(co), ctx._h, _stream_ptr(stream)))


class GridParams(LayerParams):
    """rto_grid_params: max_depth, line_px, color (the lines' rgb), background.  GridParams(options) takes max_depth =
    options.grid_max_depth and background = options.background_brightness (rto_grid_params_default)."""
    CSTRUCT, DEFAULT = CGridParams, "rto_grid_params_default"

    def _load(self, c):
        self.max_depth, self.line_px, self.color, self.background = c.max_depth, c.line_px, list(c.color), c.background

    def to_c(self, merge=False):
        c = CGridParams()
        c.max_depth, c.line_px, c.background = int(self.max_depth), float(self.line_px), float(self.background)
        for i in range(3):
            c.color[i] = float(self.color[i])
        c.flags = GRID_MERGE if merge else 0
        return c


def draw_grid_layers(tree, cams, params=None, depth=None, color=None, merge=False, stream=None):
    """rto_draw_grid_layers: the octree grid of `tree` (RenderOptions.show_grid) ray-traced for the n cameras `cams` (one size)
    into depth [n, H, W] and color [n, H, W, 4], contiguous float32 torch tensors on the tree's device -- allocated here when not
    given; pass depth=False / color=False for an output that is not wanted.  params: a GridParams (None: the defaults of the
    default options).  merge=True (RTO_GRID_MERGE): depth-test the lines against what the given tensors hold instead of
    overwriting them.  Returns (depth, color) (None for an output not asked for), the inputs of RenderContext.set_layers.
    Asynchronous on `stream` (default: torch's current stream); no sync."""
    return _draw_layers("draw_grid_layers", lib().rto_draw_grid_layers, tree, cams, GridParams() if params is None else params,
                        depth, color, merge, stream)


def _draw_layers(name, entry, target, cams, params, depth, color, merge, stream):
    """a layer pass (draw_grid_layers, meshes.draw_mesh_layers) over its C entry point: target = the N3Tree / MeshSet"""
    import torch
    device = torch.device("cuda", target.device)
    if isinstance(cams, Camera):
        cams = [cams]
    n = len(cams)
    H, W = (cams[0].height, cams[0].width) if n else (0, 0)
    if merge and (depth is None or depth is False):
        raise RtoError(-1, "%s: merge=True tests against a depth tensor of the caller's" % name)

    def plane(t, shape, name):
        if t is False:
            return None
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=device)
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape)
                or t.device != device):
            raise RtoError(-1, "%s must be a contiguous float32 tensor of shape %s on %s" % (name, list(shape), device))
        return t

    d = plane(depth, (n, H, W), "depth")
    c = plane(color, (n, H, W, 4), "color")
    if n == 0:
        return d, c
    if stream is None:
        stream = torch.cuda.current_stream(device)
    arr = (CCamera * n)(*[cam.to_c() for cam in cams])
    cp = params.to_c(merge)
    check(entry(target._h, arr, n, C.byref(cp), C.c_void_p(d.data_ptr()) if d is not None else None,
                C.c_void_p(c.data_ptr()) if c is not None else None, _stream_ptr(stream)))
    return d, c


def camera_rays(cam):
    """(origins, dirs) of a Camera's pixels, row-major: float32 [H*W, 3] numpy arrays.  dirs[i] is M xyz(x, y) as the frame
    kernels compute it before normalising (float32, left to right, no FMA; volrend.cu:23-34), so render_rays of these rays
    returns aux planes 0..3 of launch_renderer bit for bit; add t_max / background to composite the camera's view over a depth
    and colour image."""
    W, H = cam.width, cam.height
    f = np.float32
    x = np.arange(W, dtype=np.int64).astype(f)[None, :]
    y = np.arange(H, dtype=np.int64).astype(f)[:, None]
    with np.errstate(all="ignore"):
        xyz0 = np.broadcast_to((x - f(0.5) * f(W)) / f(cam.fx), (H, W))
        xyz1 = np.broadcast_to(-(y - f(0.5) * f(H)) / f(cam.fy), (H, W))
        xyz2 = f(-1.0)
        m = np.asarray(cam.transform, f).reshape(-1)
        dirs = np.empty((H, W, 3), f)
        for c in range(3):
            dirs[..., c] = m[c] * xyz0 + m[3 + c] * xyz1 + m[6 + c] * xyz2
    origins = np.broadcast_to(m[9:12], (H * W, 3)).copy()
    return origins, dirs.reshape(H * W, 3)


def _as_planes(a, shape):
    """a layer given in its frame shape [frames, H, W(, 4)] (a single-slot context also takes [H, W(, 4)]) -> the flat shape
    _ray_tensor checks; anything else is passed on for _ray_tensor to refuse"""
    got = tuple(a.shape)
    if got == tuple(shape) or (shape[0] == 1 and got == tuple(shape[1:])):
        return a.reshape((-1, 4) if len(shape) == 4 else (-1,))
    return a


def _ray_tensor(a, name, cols, n, device):
    """a contiguous float32 torch tensor [n, cols] (or [n]) on `device`: torch tensors are taken as they are, numpy arrays copied over"""
    import torch
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    if not isinstance(a, torch.Tensor):
        raise TypeError("%s must be a torch tensor or a numpy array" % name)
    want = (n, cols) if cols else (n,)
    if a.dtype != torch.float32 or not a.is_contiguous() or tuple(a.shape) != want:
        raise RtoError(-1, "%s must be a contiguous float32 tensor of shape %s" % (name, list(want)))
    if a.device != device:
        raise RtoError(-1, "%s lives on %s, the tree on %s" % (name, a.device, device))
    return a


def render_rays(tree, origins, dirs, options, ctx, t_max=None, background=None, first_ray=0, out=None, stream=None,
                depth=False, t_near=False, rgba=True):
    """rto_launch_rays: colour and opacity of n arbitrary rays.  origins / dirs [n, 3], t_max [n] (world distance along the unit
    direction; None = 1e9), background [n, 3] (None = options.background_brightness): contiguous float32 torch tensors on the
    tree's device, or numpy arrays (copied over).  Returns out, a float32 [n, 4] tensor (r, g, b composited over the backdrop,
    alpha = accumulated opacity); pass `out` to fill one.  Ray i draws its samples from ctx.rng advanced by (first_ray + i) * spp.
    depth / t_near (rto_launch_rays_ex; include/rto.h "depth outputs"): when either is asked for the result is the tuple (out,
    depth [n], t_near [n]) without the ones not asked for, in that order.  rgba=False (with depth or t_near): no colour is asked
    for -- the kernel skips the shading -- and the tuple holds the depth outputs only; `out` must then be None.
    Asynchronous on `stream` (default: torch's current stream); no sync."""
    import torch
    device = torch.device("cuda", tree.device)
    n = int(origins.shape[0])
    o = _ray_tensor(origins, "origins", 3, n, device)
    d = _ray_tensor(dirs, "dirs", 3, n, device)
    tm = None if t_max is None else _ray_tensor(t_max, "t_max", 0, n, device)
    bg = None if background is None else _ray_tensor(background, "background", 3, n, device)
    if not rgba:
        if not (depth or t_near):
            raise RtoError(-1, "render_rays: no output asked for")
        if out is not None:
            raise RtoError(-1, "render_rays: rgba=False takes no `out`")
    elif out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=device)
    else:
        out = _ray_tensor(out, "out", 4, n, device)
    extra = [torch.empty((n,), dtype=torch.float32, device=device) if want else None for want in (depth, t_near)]
    res = out if not (depth or t_near) else tuple(([out] if rgba else []) + [e for e in extra if e is not None])
    if n == 0:
        return res
    if stream is None:
        stream = torch.cuda.current_stream(device)
    r = CRays()
    r.origins, r.dirs = o.data_ptr(), d.data_ptr()
    r.t_max = tm.data_ptr() if tm is not None else None
    r.background = bg.data_ptr() if bg is not None else None
    r.n, r.first_ray = n, int(first_ray)
    co = options.to_c()
    if not (depth or t_near):
        check(lib().rto_launch_rays(tree._h, C.byref(r), C.byref(co), ctx._h, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
        return out
    ro = CRaysOut()
    ro.rgba = out.data_ptr() if rgba else None
    ro.depth = extra[0].data_ptr() if extra[0] is not None else None
    ro.t_near = extra[1].data_ptr() if extra[1] is not None else None
    check(lib().rto_launch_rays_ex(tree._h, C.byref(r), C.byref(co), ctx._h, C.byref(ro), _stream_ptr(stream)))
    return res


def _dev_ptr(t):
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    if hasattr(t, "__cuda_array_interface__"):
        return C.c_void_p(t.__cuda_array_interface__["data"][0])
    raise TypeError("expected a device tensor or pointer")


FILTER_EXACT, FILTER_FAST = 0, 1  # RTO_FILTER_EXACT / RTO_FILTER_FACTORISED (include/rto.h)


def filtering(stream, weight_map, guidance_map, img_in, img_out, mode=FILTER_EXACT):
    """denoiser::filtering(stream, weight_map[L,H,W], guidance_map[L,H,W], img_in, img_out)
    (filtering.h:7-13).  Tensors are contiguous float32 device tensors (torch) or raw pointers with
    `shape`; img_in / img_out are [H,W,4].  mode: FILTER_EXACT (bit-identical to the oracle) or
    FILTER_FAST (factorised exponentials, ~1e-6 relative)."""
    for t in (weight_map, guidance_map):
        if hasattr(t, "is_contiguous") and not t.is_contiguous():
            raise RtoError(-1, "weight_map / guidance_map must be contiguous")  # CHECK_CONTIGUOUS
    L, H, W = (int(s) for s in guidance_map.shape[-3:])
    n = int(guidance_map.shape[0]) if len(guidance_map.shape) == 4 else 1  # [n,L,H,W]: n images per launch
    check(lib().rto_filtering_batch_mode(_stream_ptr(stream), _dev_ptr(weight_map), _dev_ptr(guidance_map), L, H, W, n,
                                         _dev_ptr(img_in), _dev_ptr(img_out), int(mode)))
