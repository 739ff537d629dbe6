"""rt-octree_amd -- MI355X-native RT-Octree render path (host-side mirror of the reference's
operator interface over the C ABI in include/rto.h).

The directory name carries a hyphen (it is the name the build contract asks for); import it as
`rt_octree_amd` through the alias module at the repository root.
"""
from ._lib import LIB_PATH, RtoError, build_library, lib  # noqa: F401
from .volrend import (  # noqa: F401
    Camera, N3Tree, RenderContext, RenderOptions, Timer, launch_renderer, launch_renderer_batch, filtering, render_rays, camera_rays,
    SUPPORTED_SPP, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_FAST, FILTER_EXACT, FILTER_FAST, DEPTH_BATCHED,
    GridParams, draw_grid_layers, GRID_MERGE,
)
from .meshes import Mesh, MeshSet, MeshParams, draw_mesh_layers, trace_mesh_rays, MESH_MERGE  # noqa: F401
from .metrics import FrameMetrics, ImageMetrics, read_png  # noqa: F401
from .quantize import Quantizer, quantize_median_cut  # noqa: F401
from .simplify import Simplifier, simplify_tree  # noqa: F401
from .visibility import leaf_weights, leaf_weights_host, kill_unseen  # noqa: F401
from .grid_build import TreeBuilder, build_tree, tree_to_grid  # noqa: F401
from .fit import TreeFit, HostTreeFit, fit_grad, fit_grad_host, fit_grad_rays, fit_grad_rays_host, sgd_step, sgd_step_host  # noqa: F401
from .fit import fit_optim, step_sparse, step_sparse_host, touched_list, touched_list_host, touched_words  # noqa: F401
from .refine import Refiner, refine_tree, refine_tree_host, keys_from_weights, keys_from_density  # noqa: F401

__all__ = [
    "LIB_PATH", "RtoError", "build_library", "lib", "Camera", "N3Tree", "RenderContext",
    "RenderOptions", "Timer", "launch_renderer", "launch_renderer_batch", "filtering", "render_rays", "camera_rays", "SUPPORTED_SPP",
    "KERNEL_AUTO", "KERNEL_GENERIC", "KERNEL_FAST", "FILTER_EXACT", "FILTER_FAST", "DEPTH_BATCHED",
    "GridParams", "draw_grid_layers", "GRID_MERGE",
    "Mesh", "MeshSet", "MeshParams", "draw_mesh_layers", "trace_mesh_rays", "MESH_MERGE",
    "FrameMetrics", "ImageMetrics", "read_png",
    "Quantizer", "quantize_median_cut", "Simplifier", "simplify_tree",
    "leaf_weights", "leaf_weights_host", "kill_unseen",
    "TreeBuilder", "build_tree", "tree_to_grid",
    "TreeFit", "HostTreeFit", "fit_grad", "fit_grad_host", "fit_grad_rays", "fit_grad_rays_host", "sgd_step", "sgd_step_host",
    "fit_optim", "step_sparse", "step_sparse_host", "touched_list", "touched_list_host", "touched_words",
    "Refiner", "refine_tree", "refine_tree_host", "keys_from_weights", "keys_from_density",
]
