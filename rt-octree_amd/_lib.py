"""Loads librto.so (the C ABI of include/rto.h) with ctypes.  No fallback: if the HIP library is
missing or does not load, importing a symbol from it raises."""
import ctypes as C
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.environ.get("RTO_LIB") or os.path.join(PKG_DIR, "lib", "librto.so")  # (RTO_LIB: another build of the same library, for same-box A/B runs)

RTO_OK = 0


class RtoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rto error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


class COptions(C.Structure):
    """rto_options (include/rto.h) == RenderOptions (render_options.hpp:13-78)."""
    _fields_ = [
        ("step_size", C.c_float), ("sigma_thresh", C.c_float), ("stop_thresh", C.c_float),
        ("background_brightness", C.c_float), ("render_bbox", C.c_float * 6),
        ("basis_minmax", C.c_int * 2), ("rot_dirs", C.c_float * 3),
        ("show_grid", C.c_int), ("grid_max_depth", C.c_int), ("render_depth", C.c_int),
        ("enable_probe", C.c_int), ("probe", C.c_float * 3), ("probe_disp_size", C.c_int),
        ("denoise", C.c_int), ("spp", C.c_int),
    ]


class CCamera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_float), ("fy", C.c_float),
                ("transform", C.c_float * 12)]


class CRays(C.Structure):
    """rto_rays (include/rto.h): device pointers to the ray buffers"""
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("t_max", C.c_void_p), ("background", C.c_void_p),
                ("n", C.c_int64), ("first_ray", C.c_int64)]


class CRaysOut(C.Structure):
    """rto_rays_out (include/rto.h): device pointers, any of them NULL"""
    _fields_ = [("rgba", C.c_void_p), ("depth", C.c_void_p), ("t_near", C.c_void_p)]


class CQueryOut(C.Structure):
    """rto_query_out (include/rto.h): device pointers, any of them NULL"""
    _fields_ = [("values", C.c_void_p), ("sigma", C.c_void_p), ("level", C.c_void_p), ("cube", C.c_void_p)]


class CGridParams(C.Structure):
    """rto_grid_params (include/rto.h)"""
    _fields_ = [("max_depth", C.c_int), ("line_px", C.c_float), ("color", C.c_float * 3), ("background", C.c_float),
                ("flags", C.c_int)]


class CMeshDesc(C.Structure):
    """rto_mesh_desc (include/rto.h): host pointers"""
    _fields_ = [("vert", C.c_void_p), ("n_verts", C.c_int64), ("faces", C.c_void_p), ("n_faces", C.c_int64),
                ("face_size", C.c_int), ("unlit", C.c_int), ("estimate_normals", C.c_int), ("rotation", C.c_float * 3),
                ("translation", C.c_float * 3), ("scale", C.c_float)]


class CMeshesInfo(C.Structure):
    """rto_meshes_info (include/rto.h)"""
    _fields_ = [("triangles", C.c_int64), ("segments", C.c_int64), ("points", C.c_int64), ("nodes", C.c_int64),
                ("device_bytes", C.c_int64), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("device", C.c_int)]


class CMeshParams(C.Structure):
    """rto_mesh_params (include/rto.h)"""
    _fields_ = [("line_px", C.c_float), ("point_px", C.c_float), ("background", C.c_float), ("flags", C.c_int)]


class CMeshRays(C.Structure):
    """rto_mesh_rays (include/rto.h): device pointers (host pointers for rto_meshes_trace_rays_host)"""
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("n", C.c_int64), ("line_spread", C.c_float),
                ("point_spread", C.c_float), ("background", C.c_float)]


class CGuidanceLayer(C.Structure):
    """rto_guidance_layer (include/rto.h): host pointers to one convolution's fp32 weights [cout][cin][3][3] and bias"""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("cin", C.c_int), ("cout", C.c_int)]


class CGuidanceTrainLayer(C.Structure):
    """rto_guidance_train_layer (include/rto.h): device pointers to one layer's effective kernel, bias and their gradients"""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p),
                ("cin", C.c_int), ("cout", C.c_int)]


class CGuidanceNetInfo(C.Structure):
    _fields_ = [("c1", C.c_int), ("levels", C.c_int), ("num_layers", C.c_int), ("halo", C.c_int), ("packed_route", C.c_int)]


class CTreeInfo(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64), ("N", C.c_int), ("data_dim", C.c_int), ("format", C.c_int),
        ("basis_dim", C.c_int), ("scale", C.c_float * 3), ("offset", C.c_float * 3),
        ("use_ndc", C.c_int), ("ndc_width", C.c_float), ("ndc_height", C.c_float),
        ("ndc_focal", C.c_float), ("max_depth", C.c_int), ("device_bytes", C.c_int64),
        ("wide_nodes", C.c_int64),
    ]


class CSimplifyStats(C.Structure):
    """rto_simplify_stats (include/rto.h)"""
    _fields_ = [("reachable", C.c_int64), ("unreachable", C.c_int64), ("killed", C.c_int64), ("merged", C.c_int64),
                ("levels", C.c_int64)]


class CGridBuildStats(C.Structure):
    """rto_grid_build_stats (include/rto.h)"""
    _fields_ = [("nodes", C.c_int64), ("killed", C.c_int64), ("levels", C.c_int64)]


class CRefineStats(C.Structure):
    """rto_refine_stats (include/rto.h)"""
    _fields_ = [("reachable", C.c_int64), ("candidates", C.c_int64), ("selected", C.c_int64), ("levels", C.c_int64),
                ("cut_key", C.c_int64)]


class CFitOptim(C.Structure):
    """rto_fit_optim (include/rto.h)"""
    _fields_ = [("kind", C.c_int), ("lr", C.c_float), ("grad_scale", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("bias1", C.c_float), ("bias2", C.c_float)]


# every symbol include/rto.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "rto_version": (C.c_char_p, []),
    "rto_last_error": (C.c_char_p, []),
    "rto_device_count": (C.c_int, []),
    "rto_options_default": (None, [C.POINTER(COptions)]),
    "rto_options_from_json_file": (C.c_int, [C.c_char_p, C.POINTER(COptions)]),
    "rto_options_from_json": (C.c_int, [C.c_char_p, C.POINTER(COptions)]),
    "rto_tree_load_npz": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "rto_tree_load_npz_ex": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_tree_from_arrays": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p,
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                       C.POINTER(_P)]),
    "rto_tree_from_arrays_ex": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p,
                                          C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                                          C.POINTER(_P)]),
    "rto_tree_from_arrays_extra": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p,
                                             C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                                             _P, C.c_int64, C.POINTER(_P)]),
    "rto_tree_set_ndc": (C.c_int, [_P, C.c_float, C.c_float, C.c_float]),
    "rto_tree_get_info": (C.c_int, [_P, C.POINTER(CTreeInfo)]),
    "rto_tree_query": (C.c_int, [_P, _P, C.c_int64, C.POINTER(CQueryOut), _P]),
    "rto_grid_params_default": (None, [C.POINTER(CGridParams), C.POINTER(COptions)]),
    "rto_draw_grid_layers": (C.c_int, [_P, C.POINTER(CCamera), C.c_int, C.POINTER(CGridParams), _P, _P, _P]),
    "rto_meshes_create": (C.c_int, [C.POINTER(CMeshDesc), C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_meshes_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "rto_meshes_load_files": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_meshes_get_info": (C.c_int, [_P, C.POINTER(CMeshesInfo)]),
    "rto_meshes_download": (C.c_int, [_P, _P, _P]),
    "rto_meshes_free": (None, [_P]),
    "rto_mesh_params_default": (None, [C.POINTER(CMeshParams), C.POINTER(COptions)]),
    "rto_draw_mesh_layers": (C.c_int, [_P, C.POINTER(CCamera), C.c_int, C.POINTER(CMeshParams), _P, _P, _P]),
    "rto_meshes_trace_rays": (C.c_int, [_P, C.POINTER(CMeshRays), _P, _P, _P]),
    "rto_meshes_trace_rays_host": (C.c_int, [_P, C.POINTER(CMeshRays), _P, _P]),
    "rto_tree_probe_npz": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "rto_tree_free": (None, [_P]),
    "rto_ctx_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_ctx_create_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_ctx_frames": (C.c_int, [_P]),
    "rto_ctx_select_frame": (C.c_int, [_P, C.c_int]),
    "rto_ctx_free": (None, [_P]),
    "rto_ctx_width": (C.c_int, [_P]),
    "rto_ctx_height": (C.c_int, [_P]),
    "rto_ctx_aux": (_P, [_P]),
    "rto_ctx_noisy": (_P, [_P]),
    "rto_ctx_image": (_P, [_P]),
    "rto_ctx_rng_seed": (None, [_P, C.c_uint64, C.c_uint64]),
    "rto_ctx_rng_advance": (None, [_P, C.c_int64]),
    "rto_ctx_rng_set": (None, [_P, C.c_uint64, C.c_uint64]),
    "rto_ctx_rng_get": (None, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rto_ctx_set_kernel": (C.c_int, [_P, C.c_int]),
    "rto_ctx_set_tuning": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "rto_ctx_set_lean_outputs": (C.c_int, [_P, C.c_int]),
    "rto_ctx_frames_are_lean": (C.c_int, [_P, C.c_int, C.c_int]),
    "rto_ctx_frames_lean_level": (C.c_int, [_P, C.c_int, C.c_int]),
    "rto_ctx_queue_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rto_ctx_set_layers": (C.c_int, [_P, _P, _P]),
    "rto_ctx_layers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "rto_ctx_tile_marks": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "rto_ctx_kernel_timing": (C.c_int, [_P, C.c_int]),
    "rto_ctx_kernel_timing_read": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "rto_ctx_kernel_timing_read3": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "rto_ctx_enable_stats": (C.c_int, [_P, C.c_int]),
    "rto_ctx_get_stats": (C.c_int, [_P, _P, C.POINTER(C.c_uint64), C.c_int]),
    "rto_ctx_get_march_stats": (C.c_int, [_P, _P, C.POINTER(C.c_uint64), C.c_int]),
    "rto_wide_image_probe": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "rto_launch_renderer": (C.c_int, [_P, C.POINTER(CCamera), C.POINTER(COptions), _P, _P]),
    "rto_launch_renderer_batch": (C.c_int, [_P, C.POINTER(CCamera), C.POINTER(C.c_int64), C.c_int, C.POINTER(COptions), _P, _P]),
    "rto_launch_rays": (C.c_int, [_P, C.POINTER(CRays), C.POINTER(COptions), _P, _P, _P]),
    "rto_launch_rays_ex": (C.c_int, [_P, C.POINTER(CRays), C.POINTER(COptions), _P, C.POINTER(CRaysOut), _P]),
    "rto_ctx_enable_depth": (C.c_int, [_P, C.c_int]),
    "rto_ctx_depth_enabled": (C.c_int, [_P]),
    "rto_ctx_depth": (_P, [_P]),
    "rto_ctx_t_near": (_P, [_P]),
    "rto_ctx_download_depth": (C.c_int, [_P, _P, _P, _P]),
    "rto_filtering_batch": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rto_filtering_batch_mode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "rto_filtering_train_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "rto_filtering_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rto_filtering": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rto_ctx_filtering": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "rto_ctx_download_rgba8": (C.c_int, [_P, _P, C.c_int, _P]),
    "rto_ctx_download_image": (C.c_int, [_P, _P, C.c_int, _P]),
    "rto_ctx_download_aux": (C.c_int, [_P, _P, _P]),
    "rto_guidance_net_create": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_guidance_net_create_layers": (C.c_int, [C.POINTER(CGuidanceLayer), C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "rto_guidance_net_get_info": (C.c_int, [_P, C.POINTER(CGuidanceNetInfo)]),
    "rto_guidance_net_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rto_guidance_net_forward_ex": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "rto_guidance_net_forward_packed": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rto_filtering_packed": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "rto_guidance_net_forward_culled": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_float]),
    "rto_filtering_culled": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_float]),
    "rto_guidance_net_forward_packed_culled": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float]),
    "rto_filtering_packed_culled": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float]),
    "rto_denoise": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "rto_denoise_launch_strips": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rto_ctx_selected_frame": (C.c_int, [_P]),
    "rto_guidance_net_reserve": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "rto_guidance_net_free": (None, [_P]),
    "rto_metrics_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_metrics_free": (None, [_P]),
    "rto_metrics_compute_async": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "rto_metrics_compute": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "rto_image_read_png": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.c_size_t]),
    "rto_image_write_png": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "rto_quantizer_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_quantizer_free": (None, [_P]),
    "rto_quantize_median_cut": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    "rto_quantize_median_cut_host": (C.c_int, [_P, C.c_int64, C.c_int, _P, _P]),
    "rto_simplifier_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_simplifier_free": (None, [_P]),
    "rto_tree_simplify": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_float, _P, _P, C.POINTER(C.c_int64), _P,
                                    C.POINTER(CSimplifyStats)]),
    "rto_tree_simplify_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_float, _P, _P, C.POINTER(C.c_int64), _P,
                                         C.POINTER(CSimplifyStats)]),
    "rto_tree_leaf_weights": (C.c_int, [_P, C.POINTER(CCamera), C.c_int, C.POINTER(COptions), _P, _P]),
    "rto_leaf_weights_host": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(C.c_float), C.POINTER(CCamera), C.c_int, C.POINTER(COptions), C.c_int, _P]),
    "rto_tree_fit_grad": (C.c_int, [_P, _P, C.POINTER(CCamera), C.POINTER(_P), C.POINTER(_P), C.c_int, C.POINTER(COptions), _P, _P, _P]),
    "rto_fit_sgd_step": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P]),
    "rto_fit_grad_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(CCamera), C.POINTER(_P), C.POINTER(_P), C.c_int,
                                    C.POINTER(COptions), C.c_int, _P, _P]),
    "rto_fit_sgd_step_host": (C.c_int, [_P, _P, C.c_int64, C.c_float]),
    "rto_tree_fit_grad_rays": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(COptions), _P, _P, _P]),
    "rto_fit_grad_rays_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64, C.POINTER(COptions), C.c_int, _P, _P]),
    "rto_tree_fit_grad_rays_touched": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(COptions), _P, _P, _P, _P]),
    "rto_fit_grad_rays_touched_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_float),
                                                 C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64,
                                                 C.POINTER(COptions), C.c_int, _P, _P, _P]),
    "rto_fit_touched_block_words": (C.c_int, []),
    "rto_fit_touched_scratch_bytes": (C.c_int64, [C.c_int64]),
    "rto_fit_touched_list": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    "rto_fit_touched_list_host": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, _P]),
    "rto_fit_step_sparse": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_int64, C.POINTER(CFitOptim), _P]),
    "rto_fit_step_sparse_host": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_int64, C.POINTER(CFitOptim)]),
    "rto_tree_builder_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_tree_builder_free": (None, [_P]),
    "rto_tree_build_plan": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int64), C.POINTER(CGridBuildStats)]),
    "rto_tree_build_write": (C.c_int, [_P, _P, _P, _P]),
    "rto_tree_build_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, _P, _P, C.c_int64, C.POINTER(C.c_int64),
                                      C.POINTER(CGridBuildStats)]),
    "rto_refiner_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_refiner_free": (None, [_P]),
    "rto_tree_refine_plan": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_uint32, C.c_int64, C.c_int, C.POINTER(C.c_int64),
                                       C.POINTER(CRefineStats)]),
    "rto_tree_refine_write": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
    "rto_tree_refine_host": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_int64, C.c_int, _P, _P, C.c_int64,
                                       C.POINTER(C.c_int64), _P, C.POINTER(CRefineStats)]),
    "rto_guidance_train_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rto_guidance_train_free": (None, [_P]),
    "rto_guidance_train_acts_bytes": (C.c_int, [C.POINTER(CGuidanceTrainLayer), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "rto_guidance_train_forward": (C.c_int, [_P, _P, _P, C.POINTER(CGuidanceTrainLayer), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rto_guidance_train_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(CGuidanceTrainLayer), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rto_loss_forward_backward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rto_probe_gather": (C.c_int, [C.c_uint64, C.c_int]),
    "rto_probe_gather_sweep": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_double)]),
    "rto_probe_scratch": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "rto_probe_valu": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "rto_probe_valu_name": (C.c_char_p, [C.c_int]),
    "rto_probe_thresholds": (C.c_int, [C.c_uint32, C.c_uint32, _P]),
    "rto_probe_math": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    "rto_probe_sigmoid": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "rto_probe_basis": (C.c_int, [_P, C.POINTER(COptions), _P, C.c_int64, C.c_int, _P]),
    "rto_timer_reset": (C.c_int, [_P, _P]),
    "rto_timer_start": (C.c_int, [_P, C.c_int]),
    "rto_timer_stop": (C.c_int, [_P, C.c_int]),
    "rto_timer_record": (C.c_int, [_P, C.c_int]),
    "rto_timer_report": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
}


def build_jobs(env=None):
    """make's job count: MAX_JOBS when it is set to a positive number (16 at most), else 4"""
    try:
        jobs = int((os.environ if env is None else env).get("MAX_JOBS", ""))
    except ValueError:
        jobs = 0
    return min(jobs, 16) if jobs > 0 else 4


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 build of librto.so (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "-j%d" % build_jobs()], stdout=out)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("librto.so was not produced at " + LIB_PATH)
    return LIB_PATH


_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64.so (soname
    libamdhip64.so.7, the name librto.so needs too).  Whichever copy is mapped first serves both, but
    torch cannot find a GPU if it comes second behind /opt/rocm's -- so map torch's copy before
    librto.so.  Without torch installed this is a no-op and /opt/rocm's runtime is used."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        cand = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def lib():
    """The loaded library with prototypes set.  Raises if librto.so is absent or lacks a symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "librto.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the render path)" % LIB_PATH)
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("RTO_LIB") and os.environ.get("RTO_LIB_OLDER_BUILD") and not hasattr(L, name):
                continue  # (same-box A/B against the library of an OLDER revision, tools/ab_rev.sh: symbols added since are absent)
            fn = getattr(L, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != RTO_OK:
        raise RtoError(rc, lib().rto_last_error().decode("utf-8", "replace"))
    return rc


class LayerParams:
    """GridParams / MeshParams: C struct CSTRUCT as DEFAULT(options) sets it, then keywords; a subclass has _load(c), to_c(merge)"""
    def __init__(self, options=None, **kw):
        c = self.CSTRUCT()
        co = options.to_c() if options is not None else None
        getattr(lib(), self.DEFAULT)(C.byref(c), C.byref(co) if co is not None else None)
        self._load(c)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError("%s has no field '%s'" % (self.CSTRUCT.__name__[1:], k))
            setattr(self, k, v)
