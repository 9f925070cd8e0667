"""ctypes mirror of include/gh_raster.h (the C-ABI drop-in boundary). Pure declarations."""
from __future__ import annotations

import ctypes as C

GH_TILE = 16
GH_CAM_FLOATS = 40
GH_FLAG_BLEND_W_PER_GAUSSIAN = 1
GH_FLAG_BLEND_COLOR_B_RGB = 2
GH_FLAG_PER_VIEW_GAUSSIANS = 4
GH_FLAG_SPLIT_STREAMS = 8
GH_FLAG_STATIC_LISTS = 16
GH_FLAG_DEPTH24 = 32
GH_FLAG_DEFER_LOSS_SUM = 64
GH_FLAG_FRESH_ORDER = 128
GH_VERSION_MAJOR, GH_VERSION_MINOR = 0, 8        # the header this mirror was written against (checked against gh_version() on load)
GH_ABI_TAG = 0x47480000 | (GH_VERSION_MAJOR << 8) | GH_VERSION_MINOR
# GhCounters.overflow: bits 0-3 are errors, bit 4 is information (the depth keys' top byte did not vary)
GH_COUNTER_OVERFLOW = 1
GH_COUNTER_STALE_LISTS = 2
GH_COUNTER_BOUND_MISS = 4
GH_COUNTER_DEPTH24_FAILED = 8
GH_COUNTER_ERROR_MASK = GH_COUNTER_OVERFLOW | GH_COUNTER_STALE_LISTS | GH_COUNTER_BOUND_MISS | GH_COUNTER_DEPTH24_FAILED
GH_COUNTER_DEPTH24_OK = 16

GH_OK = 0
GH_ERR_INVALID_ARG = -1
GH_ERR_WORKSPACE_SMALL = -2
GH_ERR_LAUNCH = -3
GH_ERR_UNSUPPORTED = -4
GH_ERR_ABI = -5
_STATUS = {0: "GH_OK", -1: "GH_ERR_INVALID_ARG", -2: "GH_ERR_WORKSPACE_SMALL", -3: "GH_ERR_LAUNCH",
           -4: "GH_ERR_UNSUPPORTED", -5: "GH_ERR_ABI"}

fp = C.POINTER(C.c_float)


class GhDims(C.Structure):
    """GhDims(P, n_views, H, W, sh_degree, M, scale_modifier, flags, max_instances): the ABI tag (first field of the C struct) is
    filled in here, so that every struct this mirror builds carries the version this mirror was written against."""
    _fields_ = [("abi", C.c_uint32), ("P", C.c_int32), ("n_views", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("sh_degree", C.c_int32), ("M", C.c_int32), ("scale_modifier", C.c_float),
                ("flags", C.c_uint32), ("max_instances", C.c_int64)]

    def __init__(self, *args, **kw):
        super().__init__(GH_ABI_TAG, *args, **kw)


class GhInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "cams", "means3D", "opacities", "scales", "rotations", "shs", "colors_precomp",
        "blend_xyz_b", "blend_opacity_b", "blend_color_w", "blend_color_b", "tile_depth_bound", "cov3D_precomp")]


class GhFitLoss(C.Structure):
    _fields_ = [("gt_rgb", C.c_void_p), ("gt_mask", C.c_void_p), ("bbox", C.c_void_p), ("lambda_l1", C.c_float),
                ("lambda_mask", C.c_float), ("scale", C.c_float), ("dL_dimage", C.c_void_p), ("dL_dalpha", C.c_void_p),
                ("loss", C.c_void_p)]


class GhOutputs(C.Structure):
    _fields_ = [("image", C.c_void_p), ("radii", C.c_void_p), ("alpha", C.c_void_p), ("tile_depth_seen", C.c_void_p),
                ("tile_depth_seen_scale", C.c_float), ("tile_depth_seen_slack", C.c_uint32),
                ("l1_target", C.c_void_p), ("l1_dL_dimage", C.c_void_p), ("l1_loss", C.c_void_p),
                ("fit_loss", C.POINTER(GhFitLoss))]


class GhCounters(C.Structure):
    _fields_ = [("num_rendered", C.c_uint32), ("overflow", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class GhGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "dL_dimage", "dL_dalpha", "dL_dmeans3D", "dL_dmeans2D", "dL_dopacities", "dL_dscales", "dL_drotations",
        "dL_dshs", "dL_dcolors", "dL_dblend_xyz_b", "dL_dblend_opacity_b", "dL_dblend_color_w",
        "dL_dblend_color_b", "upstream_scale", "dL_dcov3D", "deferred_loss")]


class GhAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_size_t),
                ("reg_l1", C.c_float), ("reg_l2", C.c_float), ("partials", C.c_void_p), ("n_partials", C.c_int),
                ("step_state", C.c_void_p)]


LAYOUT_FIELDS = ("total_bytes", "counters", "geom", "clamped",
                 "tiles_touched", "slot_begin", "depth_keys_a", "depth_keys_b", "depth_vals_a", "depth_vals_b",
                 "block_sums", "keys_a", "keys_b", "vals_a", "vals_b", "sorted_slot", "inst_r0", "inst_r1", "inst_r2",
                 "sort_tables", "ranges", "tile_walk", "tile_order", "bwd_items", "ckpt_rgb", "final_C", "final_T", "n_contrib", "inst_grad", "inst_flag", "sh_rgb", "dmean_sh", "sh_scratch", "grad_sums", "bwd_scratch", "cull_bound", "inst_c", "attr", "half_counters", "key_bits", "tile_bound", "block_tiles", "render_guard", "loss_partials", "view_start")


class GhLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in LAYOUT_FIELDS]


def status_name(code: int) -> str:
    return _STATUS.get(code, f"GH_ERR({code})")


def declare_raster(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_raster.h declares."""
    lib.gh_version.restype = C.c_int
    lib.gh_version.argtypes = []
    lib.gh_workspace_layout.restype = C.c_int
    lib.gh_workspace_layout.argtypes = [C.POINTER(GhDims), C.POINTER(GhLayout)]
    lib.gh_workspace_bytes.restype = C.c_size_t
    lib.gh_workspace_bytes.argtypes = [C.POINTER(GhDims)]
    lib.gh_partition_is_per_view.restype = C.c_int
    lib.gh_partition_is_per_view.argtypes = [C.POINTER(GhDims)]
    lib.gh_forward.restype = C.c_int
    lib.gh_forward.argtypes = [C.POINTER(GhDims), C.POINTER(GhInputs), C.POINTER(GhOutputs),
                               C.c_void_p, C.c_size_t, C.c_void_p]
    lib.gh_backward.restype = C.c_int
    lib.gh_backward.argtypes = [C.POINTER(GhDims), C.POINTER(GhInputs), C.POINTER(GhGrads),
                                C.c_void_p, C.c_size_t, C.c_void_p]


    lib.gh_uv_sample_forward.restype = C.c_int
    lib.gh_uv_sample_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.gh_uv_sample_backward.restype = C.c_int
    lib.gh_uv_sample_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.gh_uv_gather_forward.restype = C.c_int
    lib.gh_uv_gather_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gh_uv_gather_backward.restype = C.c_int
    lib.gh_uv_gather_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gh_uv_scatter_sorted.restype = C.c_int
    lib.gh_uv_scatter_sorted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gh_adam_reg_step.restype = C.c_int
    lib.gh_adam_reg_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.gh_adam_reg_step_group.restype = C.c_int
    lib.gh_adam_reg_step_group.argtypes = [C.POINTER(GhAdamTensor), C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                           C.c_void_p, C.c_void_p]
    lib.gh_uv_gather_forward2.restype = C.c_int
    lib.gh_uv_gather_forward2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p]
    lib.gh_uv_scatter_sorted2.restype = C.c_int
    lib.gh_uv_scatter_sorted2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int, C.c_void_p]
    lib.gh_reg_total.restype = C.c_int
    lib.gh_reg_total.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    lib.gh_l1_loss.restype = C.c_int
    lib.gh_l1_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.gh_fit_loss.restype = C.c_int
    lib.gh_fit_loss.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 4 + \
        [C.c_int, C.c_void_p, C.c_void_p]
    lib.gh_knn_workspace_bytes.restype = C.c_size_t
    lib.gh_knn_workspace_bytes.argtypes = [C.c_int]
    lib.gh_knn_indices.restype = C.c_int
    lib.gh_knn_indices.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.gh_knn_mismatch_mask.restype = C.c_int
    lib.gh_knn_mismatch_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.gh_forward_shared.restype = C.c_int
    lib.gh_forward_shared.argtypes = [C.POINTER(GhDims), C.POINTER(GhInputs), C.POINTER(GhOutputs), C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]
    lib.gh_backward_shared.restype = C.c_int
    lib.gh_backward_shared.argtypes = [C.POINTER(GhDims), C.POINTER(GhInputs), C.POINTER(GhGrads), C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
    lib.gh_forward_refresh.restype = C.c_int
    lib.gh_forward_refresh.argtypes = lib.gh_forward_shared.argtypes
    lib.gh_backward_refresh.restype = C.c_int
    lib.gh_backward_refresh.argtypes = lib.gh_backward_shared.argtypes
    lib.gh_forward_stages.restype = C.c_int
    lib.gh_forward_stages.argtypes = lib.gh_forward.argtypes + [C.c_uint32]
    lib.gh_backward_stages.restype = C.c_int
    lib.gh_backward_stages.argtypes = lib.gh_backward.argtypes + [C.c_uint32]
    lib.gh_select_workspace_bytes.restype = C.c_size_t
    lib.gh_select_workspace_bytes.argtypes = [C.c_int]
    lib.gh_select_rows.restype = C.c_int
    lib.gh_select_rows.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + \
                                  [C.c_void_p, C.c_size_t, C.c_void_p]


GH_FWD_PREPROCESS, GH_FWD_BINNING, GH_FWD_RENDER, GH_FWD_ALL = 1, 2, 4, 7
GH_BWD_RENDER, GH_BWD_PREPROCESS, GH_BWD_ALL = 1, 2, 3

EXPORTED_SYMBOLS = ("gh_version", "gh_workspace_layout", "gh_workspace_bytes", "gh_partition_is_per_view", "gh_forward", "gh_backward",
                    "gh_forward_stages", "gh_backward_stages", "gh_forward_shared", "gh_backward_shared", "gh_forward_refresh", "gh_backward_refresh", "gh_uv_sample_forward", "gh_uv_sample_backward",
                    "gh_uv_gather_forward", "gh_uv_gather_backward", "gh_uv_scatter_sorted", "gh_adam_reg_step", "gh_reg_total", "gh_adam_reg_step_group", "gh_uv_gather_forward2", "gh_uv_scatter_sorted2",
                    "gh_knn_workspace_bytes", "gh_knn_indices", "gh_knn_mismatch_mask", "gh_l1_loss", "gh_fit_loss",
                    "gh_select_workspace_bytes", "gh_select_rows")


# ---- include/gh_metrics.h: image-quality scores (a header of its own, not part of gh_raster.h's versioned surface) ----
GH_METRICS_CHW = 0
GH_METRICS_PRED_HWC = 1
GH_METRICS_GT_HWC = 2
GH_METRICS_HWC = GH_METRICS_PRED_HWC | GH_METRICS_GT_HWC

METRICS_SYMBOLS = ("gh_image_scores_workspace", "gh_image_scores")


def declare_metrics(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_metrics.h declares."""
    lib.gh_image_scores_workspace.restype = C.c_size_t
    lib.gh_image_scores_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gh_image_scores.restype = C.c_int
    lib.gh_image_scores.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_double] + [C.c_void_p] * 3 + \
        [C.c_size_t, C.c_void_p]


# ---- include/gh_pool.h: per-cell pooling of point features (a header of its own, as gh_metrics.h is) ----
GH_POOL_MAX = 0
GH_POOL_MEAN = 1
GH_POOL_MAX_CELLS = 8192

POOL_SYMBOLS = ("gh_pool_plan_workspace", "gh_pool_plan", "gh_pool_forward", "gh_pool_backward", "gh_plane_mean_forward",
                "gh_plane_mean_backward")


def declare_pool(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_pool.h declares."""
    lib.gh_pool_plan_workspace.restype = C.c_size_t
    lib.gh_pool_plan_workspace.argtypes = [C.c_int, C.c_int]
    lib.gh_pool_plan.restype = C.c_int
    lib.gh_pool_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]
    lib.gh_pool_forward.restype = C.c_int
    lib.gh_pool_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.gh_pool_backward.restype = C.c_int
    lib.gh_pool_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gh_plane_mean_forward.restype = C.c_int
    lib.gh_plane_mean_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gh_plane_mean_backward.restype = C.c_int
    lib.gh_plane_mean_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


# ---- include/gh_head.h: the fused Gaussian head (a header of its own, as gh_pool.h is) ----
GH_HEAD_USE_RGB = 1
GH_HEAD_XYZ_OFFSET = 2
GH_HEAD_RESTRICT_OFFSET = 4
GH_HEAD_CLIP_SCALING = 8
GH_HEAD_ROWS = 64
GH_HEAD_SEGMENTS = 16
GH_HEAD_MAX_O = 59

HEAD_SYMBOLS = ("gh_head_workspace_bytes", "gh_head_forward", "gh_head_backward")


class GhHeadDesc(C.Structure):
    _fields_ = [("shs_width", C.c_int32), ("flags", C.c_uint32), ("clip_scaling", C.c_float)]


def declare_head(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_head.h declares."""
    lib.gh_head_workspace_bytes.restype = C.c_size_t
    lib.gh_head_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gh_head_forward.restype = C.c_int
    lib.gh_head_forward.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GhHeadDesc)] + \
        [C.c_void_p] * 6 + [C.c_void_p]
    lib.gh_head_backward.restype = C.c_int
    lib.gh_head_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(GhHeadDesc)] + \
        [C.c_void_p] * 5 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


# ---- include/gh_vert.h: the fused vertex MLP block (a header of its own, as gh_head.h is) ----
GH_VERT_ACT_SIGMOID = 0
GH_VERT_ACT_TANH_OFFSET = 1
GH_VERT_ROWS = 64
GH_VERT_SEGMENTS = 16
GH_VERT_MAX_CF = 256

VERT_SYMBOLS = ("gh_vert_workspace_bytes", "gh_vert_forward", "gh_vert_backward")
VERT_PARAMS = ("ln_weight", "ln_bias", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias", "fc_weight", "fc_bias")


class GhVertDesc(C.Structure):
    _fields_ = [("K", C.c_int32), ("act", C.c_uint32), ("radius", C.c_float), ("eps", C.c_float)]


class GhVertParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VERT_PARAMS]


class GhVertGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VERT_PARAMS]


def declare_vert(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_vert.h declares."""
    lib.gh_vert_workspace_bytes.restype = C.c_size_t
    lib.gh_vert_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.gh_vert_forward.restype = C.c_int
    lib.gh_vert_forward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(GhVertParams), C.POINTER(GhVertDesc),
                                    C.c_void_p, C.c_void_p]
    lib.gh_vert_backward.restype = C.c_int
    lib.gh_vert_backward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(GhVertParams), C.POINTER(GhVertDesc),
                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(GhVertGrads), C.c_void_p, C.c_size_t,
                                     C.c_void_p]


# ---- include/gh_plane.h: the plane fetch (a header of its own, as gh_vert.h is) ----
PLANE_SYMBOLS = ("gh_plane_workspace", "gh_plane_sample_forward", "gh_plane_index", "gh_plane_sample_backward")


def declare_plane(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_plane.h declares."""
    lib.gh_plane_workspace.restype = C.c_size_t
    lib.gh_plane_workspace.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.gh_plane_sample_forward.restype = C.c_int
    lib.gh_plane_sample_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.c_void_p]
    lib.gh_plane_index.restype = C.c_int
    lib.gh_plane_index.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]
    lib.gh_plane_sample_backward.restype = C.c_int
    lib.gh_plane_sample_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p]


# ---- include/gh_attn.h: the interaction attention's core (a header of its own, as gh_plane.h is) ----
GH_ATTN_D = 32
GH_ATTN_MAX_BH = 65535
GH_ATTN_MAX_V = 1 << 30

ATTN_SYMBOLS = ("gh_attn_workspace_bytes", "gh_attn_forward", "gh_attn_backward")


class GhAttnDims(C.Structure):
    _fields_ = [("BS", C.c_int32), ("V", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("norm", C.c_float)]


class GhAttnTensor(C.Structure):
    """A (BS, V, H, D) view with unit last stride: the pointer and the batch, row and head strides in elements."""
    _fields_ = [("p", C.c_void_p), ("stride_b", C.c_int64), ("stride_v", C.c_int64), ("stride_h", C.c_int64)]


def declare_attn(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_attn.h declares."""
    T = C.POINTER(GhAttnTensor)
    lib.gh_attn_workspace_bytes.restype = C.c_size_t
    lib.gh_attn_workspace_bytes.argtypes = [C.POINTER(GhAttnDims)]
    lib.gh_attn_forward.restype = C.c_int
    lib.gh_attn_forward.argtypes = [C.POINTER(GhAttnDims), T, T, T, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gh_attn_backward.restype = C.c_int
    lib.gh_attn_backward.argtypes = [C.POINTER(GhAttnDims), T, T, T, C.c_void_p, C.c_void_p, T] + [C.c_void_p] * 3 + \
        [C.c_void_p, C.c_size_t, C.c_void_p]


# ---- include/gh_uvd.h: the UV search (a header of its own, as gh_attn.h is) ----
GH_UVD_MAX_SPLIT = 16
GH_UVD_REC_BYTES = 80
GH_UVD_TARGET_WGS = 8192
GH_UVD_MIN_CHUNK = 128

UVD_SYMBOLS = ("gh_uvd_workspace_bytes", "gh_uvd_auto_split", "gh_uvd_forward")


def declare_uvd(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_uvd.h declares."""
    lib.gh_uvd_workspace_bytes.restype = C.c_size_t
    lib.gh_uvd_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gh_uvd_auto_split.restype = C.c_int
    lib.gh_uvd_auto_split.argtypes = [C.c_int, C.c_int]
    lib.gh_uvd_forward.restype = C.c_int
    lib.gh_uvd_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + \
        [C.c_void_p, C.c_size_t, C.c_void_p]


# ---- include/gh_cond.h: the point conditioning (a header of its own, as gh_uvd.h is) ----
GH_COND_ROWS = 64
GH_COND_MAX_LEVELS = 8
GH_COND_MAX_CODE = 64
GH_COND_MAX_HD = 64

COND_SYMBOLS = ("gh_cond_width", "gh_cond_fold_bytes", "gh_cond_rows", "gh_cond_fold", "gh_cond_mlp_forward", "gh_cond_mlp_backward")
COND_PARAMS = ("ln_weight", "ln_bias", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")


class GhCondRows(C.Structure):
    """The segments of the varying row: uv (P,2), xyz (P,3), flag (P,), code (P,Cc) through code_stride; absent ones are NULL."""
    _fields_ = [("uv", C.c_void_p), ("xyz", C.c_void_p), ("flag", C.c_void_p), ("code", C.c_void_p), ("code_stride", C.c_int64),
                ("Cc", C.c_int32), ("levels", C.c_int32)]


class GhCondParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in COND_PARAMS]


def declare_cond(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_cond.h declares."""
    R, Pm = C.POINTER(GhCondRows), C.POINTER(GhCondParams)
    lib.gh_cond_width.restype = C.c_int
    lib.gh_cond_width.argtypes = [R]
    lib.gh_cond_fold_bytes.restype = C.c_size_t
    lib.gh_cond_fold_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gh_cond_rows.restype = C.c_int
    lib.gh_cond_rows.argtypes = [R, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.gh_cond_fold.restype = C.c_int
    lib.gh_cond_fold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, Pm, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.gh_cond_mlp_forward.restype = C.c_int
    lib.gh_cond_mlp_forward.argtypes = [R, C.c_int, C.c_int, C.c_int, C.c_int, Pm, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.gh_cond_mlp_backward.restype = C.c_int
    lib.gh_cond_mlp_backward.argtypes = [R, C.c_int, C.c_int, C.c_int, C.c_int, Pm, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p]


# ---- include/gh_res.h: the encoders' ResNet blocks, pooled half per cell (a header of its own, as gh_cond.h is) ----
GH_RES_ROWS = 128
GH_RES_MAX_H = 128

RES_SYMBOLS = ("gh_res_forward", "gh_res_backward", "gh_res_cell_sum", "gh_res_cell_max", "gh_res_cell_max_backward")


def declare_res(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_res.h declares."""
    V, I, L = C.c_void_p, C.c_int, C.c_int64
    lib.gh_res_forward.restype = C.c_int
    lib.gh_res_forward.argtypes = [V, L, I, I, I, V, V, I, V, V, L, V, L, V, V, L, V, V]
    lib.gh_res_backward.restype = C.c_int
    lib.gh_res_backward.argtypes = [V, L, V, L, I, I, I, V, V, L, V, L, V, V, L, V, V]
    lib.gh_res_cell_sum.restype = C.c_int
    lib.gh_res_cell_sum.argtypes = [V, L, I, I, I, V, V, I, V, V]
    lib.gh_res_cell_max.restype = C.c_int
    lib.gh_res_cell_max.argtypes = [V, L, I, I, I, V, V, V, V, V]
    lib.gh_res_cell_max_backward.restype = C.c_int
    lib.gh_res_cell_max_backward.argtypes = [V, V, I, I, I, V, L, V]


bind_res = declare_res          # for a caller that loads the library itself and binds this header alone


# ---- include/gh_attn_rows.h: the row work around the attention core (a header of its own, as gh_res.h is) ----
GH_ATTN_ROWS_MAX_H = 8
GH_ATTN_ROWS_MAX_F = 192

ATTN_ROWS_SYMBOLS = ("gh_attn_rows_workspace_bytes", "gh_attn_rows_pre_forward", "gh_attn_rows_post_forward", "gh_attn_rows_post_backward",
                     "gh_attn_rows_pre_backward")
ATTN_ROWS_PARAMS = ("wq_weight", "wq_bias", "wk_weight", "wk_bias", "wv_weight", "wv_bias", "ln1_weight", "ln1_bias", "fc_weight", "fc_bias",
                    "ln2_weight", "ln2_bias", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")


class GhAttnRowsDims(C.Structure):
    _fields_ = [("V", C.c_int32), ("F", C.c_int32), ("H", C.c_int32), ("hid", C.c_int32), ("eps1", C.c_float), ("eps2", C.c_float),
                ("x_stride", C.c_int64), ("out_stride", C.c_int64), ("dout_stride", C.c_int64), ("dx_stride", C.c_int64)]


class GhAttnRowsParams(C.Structure):
    """The module's sixteen tensors in state-dict order."""
    _fields_ = [(n, C.c_void_p) for n in ATTN_ROWS_PARAMS]


def declare_attn_rows(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_attn_rows.h declares."""
    D, Pm, V = C.POINTER(GhAttnRowsDims), C.POINTER(GhAttnRowsParams), C.c_void_p
    lib.gh_attn_rows_workspace_bytes.restype = C.c_size_t
    lib.gh_attn_rows_workspace_bytes.argtypes = [D]
    lib.gh_attn_rows_pre_forward.restype = C.c_int
    lib.gh_attn_rows_pre_forward.argtypes = [D, Pm, V, V, V, V, V]
    lib.gh_attn_rows_post_forward.restype = C.c_int
    lib.gh_attn_rows_post_forward.argtypes = [D, Pm, V, V, V, V, V, V, V, V]
    lib.gh_attn_rows_post_backward.restype = C.c_int
    lib.gh_attn_rows_post_backward.argtypes = [D, Pm, V, V, V, V, V, V, V, C.c_size_t, V]
    lib.gh_attn_rows_pre_backward.restype = C.c_int
    lib.gh_attn_rows_pre_backward.argtypes = [D, Pm, V, V, V, V, V, V, V, C.c_size_t, V, V]


# ---- include/gh_scene.h: the texture scene code (a header of its own, as gh_attn_rows.h is) ----
GH_SCENE_PER_PLANE = 1
GH_SCENE_MAX_CI = 1024
GH_SCENE_MAX_CO = 128
GH_SCENE_MAX_TILES = 2147483647

SCENE_SYMBOLS = ("gh_scene_code_forward", "gh_scene_code_backward")


class GhSceneDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("Ci", C.c_int32), ("Co", C.c_int32), ("Np", C.c_int32), ("S", C.c_int32), ("flags", C.c_uint32)]


def declare_scene(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_scene.h declares."""
    D, V, L = C.POINTER(GhSceneDims), C.c_void_p, C.c_int64
    lib.gh_scene_code_forward.restype = C.c_int
    lib.gh_scene_code_forward.argtypes = [D, V, L, L, V, L, L, V, V, V, L, L, V, V]
    lib.gh_scene_code_backward.restype = C.c_int
    lib.gh_scene_code_backward.argtypes = [D, V, V, V, V, L, L, V]


# ---- include/gh_trunk.h: forward_gs's trunk MLP and Gaussian head in one pass (a header of its own, as gh_scene.h is) ----
GH_TRUNK_SILU = 0
GH_TRUNK_RELU = 1
GH_TRUNK_ROWS = 128
GH_TRUNK_MAX_CIN = 192

TRUNK_SYMBOLS = ("gh_trunk_forward", "gh_trunk_backward")


def declare_trunk(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_trunk.h declares."""
    D, V, L, I = C.POINTER(GhHeadDesc), C.c_void_p, C.c_int64, C.c_int
    lib.gh_trunk_forward.restype = C.c_int
    lib.gh_trunk_forward.argtypes = [V, L, I, I, I, I, V] + [V] * 8 + [D, I] + [V] * 6 + [V]
    lib.gh_trunk_backward.restype = C.c_int
    lib.gh_trunk_backward.argtypes = [V, V, L, I, I, I, I] + [V] * 6 + [D, I] + [V] * 5 + [V, L, V, V]


# ---- include/gh_conv.h: the perceptual loss's 3x3 convolution and 2x2 max pooling (a header of its own, as gh_trunk.h is) ----
GH_CONV_RELU = 1
GH_CONV_MAX_C = 512
GH_CONV_PIXELS = 128
GH_CONV_CHUNK = 128
GH_CONV_FILL = 512

CONV_SYMBOLS = ("gh_conv3x3_weight_floats", "gh_conv3x3_forward", "gh_conv3x3_backward_data", "gh_maxpool2x2_forward", "gh_maxpool2x2_backward")


def declare_conv(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_conv.h declares."""
    V, I, U = C.c_void_p, C.c_int, C.c_uint32
    lib.gh_conv3x3_weight_floats.restype = C.c_size_t
    lib.gh_conv3x3_weight_floats.argtypes = [I, I]
    lib.gh_conv3x3_forward.restype = C.c_int
    lib.gh_conv3x3_forward.argtypes = [V, I, I, I, I, I, V, V, U, I, V, V, V]
    lib.gh_conv3x3_backward_data.restype = C.c_int
    lib.gh_conv3x3_backward_data.argtypes = [V, V, I, I, I, I, I, V, U, I, V, V]
    lib.gh_maxpool2x2_forward.restype = C.c_int
    lib.gh_maxpool2x2_forward.argtypes = [V, I, I, I, I, V, V, V]
    lib.gh_maxpool2x2_backward.restype = C.c_int
    lib.gh_maxpool2x2_backward.argtypes = [V, V, I, I, I, I, V, V]


# ---- include/gh_mano.h: the hand points, skinning and folded subdivision (a header of its own, as gh_conv.h is) ----
GH_MANO_MAX_H = 4
GH_MANO_MAX_J = 16
GH_MANO_MAX_NB = 16
GH_MANO_MAX_LEVELS = 3
GH_MANO_MAX_V = 65536
GH_MANO_MAX_P = 4194304
GH_MANO_MAX_B = 65535
GH_MANO_CHUNK = 4096

MANO_SYMBOLS = ("gh_mano_workspace_bytes", "gh_mano_forward", "gh_mano_backward")
MANO_MODEL_ARRAYS = ("v_template", "shapedirs", "posedirs", "lbs_weights", "j_template", "j_shapedirs", "pose_mean", "st_idx", "st_w",
                     "tr_ptr", "tr_point", "tr_w")
MANO_PARAMS = ("global_orient", "hand_pose", "betas", "transl")


class GhManoDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("J", C.c_int32), ("NB", C.c_int32)]


class GhManoModel(C.Structure):
    """One hand model: the sizes, `parents` in the struct itself, then the device arrays in the header's layouts."""
    _fields_ = [("V", C.c_int32), ("P", C.c_int32), ("levels", C.c_int32), ("nnz", C.c_int32), ("parents", C.c_int32 * GH_MANO_MAX_J)] + \
        [(n, C.c_void_p) for n in MANO_MODEL_ARRAYS]


class GhManoParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MANO_PARAMS]


class GhManoGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MANO_PARAMS]


def declare_mano(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_mano.h declares."""
    D, M, V = C.POINTER(GhManoDims), C.POINTER(GhManoModel), C.c_void_p
    lib.gh_mano_workspace_bytes.restype = C.c_size_t
    lib.gh_mano_workspace_bytes.argtypes = [D, M]
    lib.gh_mano_forward.restype = C.c_int
    lib.gh_mano_forward.argtypes = [D, M, C.POINTER(GhManoParams), V, V, V, C.c_size_t, V]
    lib.gh_mano_backward.restype = C.c_int
    lib.gh_mano_backward.argtypes = [D, M, V, V, C.POINTER(GhManoGrads), V, C.c_size_t, V]


# ---- include/gh_xf.h: the Transformer1D backbones' forward and backward to the input (a header of its own, as gh_mano.h is) ----
GH_XF_ROWS = 64
GH_XF_COLS = 64
GH_XF_ATTN_ROWS = 64
GH_XF_ATTN_KEYS = 64
GH_XF_GN_CHUNK = 256
GH_XF_MAX_M = 1024
GH_XF_MAX_C = 1024
GH_XF_MAX_K = 4096
GH_XF_MAX_N_OUT = 8192
GH_XF_MAX_T = 1 << 30
GH_XF_ATTN_BWD_ROWS = 128
GH_XF_ATTN_BWD_STAGE = 64
GH_XF_GRAD_MAX_M = 512
GH_XF_WGRAD_ROWS = 32
GH_XF_WGRAD_CHUNK = 256
GH_XF_WGRAD_MAX_BLOCKS = 1024
GH_XF_LNP_ROWS = 64
GH_XF_PRO_NONE, GH_XF_PRO_LN, GH_XF_PRO_GN, GH_XF_PRO_CF = 0, 1, 2, 3
GH_XF_EPI_PLAIN, GH_XF_EPI_BIAS_RES, GH_XF_EPI_GEGLU, GH_XF_EPI_BIAS_RES_CF = 0, 1, 2, 3

XF_SYMBOLS = ("gh_xf_linear_workspace_bytes", "gh_xf_linear", "gh_xf_group_moments_workspace_bytes", "gh_xf_group_moments", "gh_xf_attention",
              "gh_xf_workspace_bytes", "gh_xf_forward", "gh_xf_attention_lse", "gh_xf_attention_backward_workspace_bytes",
              "gh_xf_attention_backward", "gh_xf_geglu_backward", "gh_xf_layernorm_backward", "gh_xf_group_norm_backward_workspace_bytes",
              "gh_xf_group_norm_backward", "gh_xf_tape_bytes", "gh_xf_forward_tape", "gh_xf_backward_workspace_bytes", "gh_xf_backward",
              "gh_xf_linear_wgrad_chunk", "gh_xf_linear_wgrad_workspace_bytes", "gh_xf_linear_wgrad", "gh_xf_layernorm_param_grads_workspace_bytes",
              "gh_xf_layernorm_param_grads", "gh_xf_group_norm_param_grads_workspace_bytes", "gh_xf_group_norm_param_grads",
              "gh_xf_backward_params_workspace_bytes", "gh_xf_backward_params")
XF_STEM = ("gn_w", "gn_b", "in_w", "in_b", "out_w", "out_b")
XF_STEM_T = ("gn_w", "in_t", "out_t")
XF_LAYER_T = ("ln1_w", "qkv1_t", "o1_t", "ln2_w", "qkv2_t", "o2_t", "ln3_w", "ln3_b", "ff1_w", "ff1_b", "ff1_t", "ff2_t")
XF_LAYER = ("ln1_w", "ln1_b", "qkv1", "o1_w", "o1_b", "ln2_w", "ln2_b", "qkv2", "o2_w", "o2_b", "ln3_w", "ln3_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")


class GhXfLinear(C.Structure):
    _fields_ = [("T", C.c_int32), ("K", C.c_int32), ("N_out", C.c_int32), ("prologue", C.c_int32), ("epilogue", C.c_int32),
                ("rows_per_batch", C.c_int32), ("groups", C.c_int32), ("eps", C.c_float),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("x_stride_b", C.c_int64), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("moments", C.c_void_p),
                ("res", C.c_void_p), ("res_stride", C.c_int64), ("res_stride_b", C.c_int64),
                ("y", C.c_void_p), ("y_stride", C.c_int64), ("y_stride_b", C.c_int64)]


class GhXfDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "C", "N", "G", "heads", "D", "layers")] + [("gn_eps", C.c_float), ("ln_eps", C.c_float)]


class GhXfStem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in XF_STEM]


class GhXfLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in XF_LAYER]


class GhXfStemT(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in XF_STEM_T]


class GhXfLayerT(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in XF_LAYER_T]


class GhXfWgrad(C.Structure):
    _fields_ = [("T", C.c_int32), ("K", C.c_int32), ("N_out", C.c_int32), ("prologue", C.c_int32), ("dy_cf", C.c_int32),
                ("rows_per_batch", C.c_int32), ("groups", C.c_int32), ("eps", C.c_float),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("x_stride_b", C.c_int64),
                ("dy", C.c_void_p), ("dy_stride", C.c_int64), ("dy_stride_b", C.c_int64),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("moments", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p)]


class GhXfStemG(C.Structure):                                    # the gradients' buffers: GhXfStem's and GhXfLayer's fields
    _fields_ = [(n, C.c_void_p) for n in XF_STEM]


class GhXfLayerG(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in XF_LAYER]


def declare_xf(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_xf.h declares."""
    V, I, L = C.c_void_p, C.c_int, C.c_int64
    lib.gh_xf_linear_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_linear_workspace_bytes.argtypes = [I, I]
    lib.gh_xf_linear.restype = C.c_int
    lib.gh_xf_linear.argtypes = [C.POINTER(GhXfLinear), V, C.c_size_t, V]
    lib.gh_xf_group_moments_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_group_moments_workspace_bytes.argtypes = [I, I, I, I]
    lib.gh_xf_group_moments.restype = C.c_int
    lib.gh_xf_group_moments.argtypes = [V, L, L, I, I, I, I, V, V, C.c_size_t, V]
    lib.gh_xf_attention.restype = C.c_int
    lib.gh_xf_attention.argtypes = [V, L, I, I, I, I, V, L, V]
    lib.gh_xf_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_workspace_bytes.argtypes = [C.POINTER(GhXfDims)]
    lib.gh_xf_forward.restype = C.c_int
    lib.gh_xf_forward.argtypes = [C.POINTER(GhXfDims), C.POINTER(GhXfStem), C.POINTER(GhXfLayer), V, V, V, C.c_size_t, V]
    lib.gh_xf_attention_lse.restype = C.c_int
    lib.gh_xf_attention_lse.argtypes = [V, L, I, I, I, I, V, L, V, V]
    lib.gh_xf_attention_backward_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_attention_backward_workspace_bytes.argtypes = [I, I, I]
    lib.gh_xf_attention_backward.restype = C.c_int
    lib.gh_xf_attention_backward.argtypes = [V, L, V, L, V, V, L, I, I, I, I, V, L, V, C.c_size_t, V]
    lib.gh_xf_geglu_backward.restype = C.c_int
    lib.gh_xf_geglu_backward.argtypes = [V, L, V, L, V, V, V, V, V, V, I, I, V, L, V]
    lib.gh_xf_layernorm_backward.restype = C.c_int
    lib.gh_xf_layernorm_backward.argtypes = [V, L, V, L, V, V, I, I, V, L, V]
    lib.gh_xf_group_norm_backward_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_group_norm_backward_workspace_bytes.argtypes = [I, I, I, I]
    lib.gh_xf_group_norm_backward.restype = C.c_int
    lib.gh_xf_group_norm_backward.argtypes = [V, V, V, V, V, V, I, I, I, I, C.c_float, V, C.c_size_t, V]
    lib.gh_xf_tape_bytes.restype = C.c_size_t
    lib.gh_xf_tape_bytes.argtypes = [C.POINTER(GhXfDims)]
    lib.gh_xf_forward_tape.restype = C.c_int
    lib.gh_xf_forward_tape.argtypes = [C.POINTER(GhXfDims), C.POINTER(GhXfStem), C.POINTER(GhXfLayer), V, V, V, C.c_size_t, V, C.c_size_t, V]
    lib.gh_xf_backward_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_backward_workspace_bytes.argtypes = [C.POINTER(GhXfDims)]
    lib.gh_xf_backward.restype = C.c_int
    lib.gh_xf_backward.argtypes = [C.POINTER(GhXfDims), C.POINTER(GhXfStemT), C.POINTER(GhXfLayerT), V, V, V, V, V, C.c_size_t, V]
    lib.gh_xf_linear_wgrad_chunk.restype = C.c_int
    lib.gh_xf_linear_wgrad_chunk.argtypes = [I, I, I]
    lib.gh_xf_linear_wgrad_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_linear_wgrad_workspace_bytes.argtypes = [I, I, I]
    lib.gh_xf_linear_wgrad.restype = C.c_int
    lib.gh_xf_linear_wgrad.argtypes = [C.POINTER(GhXfWgrad), V, C.c_size_t, V]
    lib.gh_xf_layernorm_param_grads_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_layernorm_param_grads_workspace_bytes.argtypes = [I, I]
    lib.gh_xf_layernorm_param_grads.restype = C.c_int
    lib.gh_xf_layernorm_param_grads.argtypes = [V, L, V, L, V, I, I, V, V, V, C.c_size_t, V]
    lib.gh_xf_group_norm_param_grads_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_group_norm_param_grads_workspace_bytes.argtypes = [I, I, I, I]
    lib.gh_xf_group_norm_param_grads.restype = C.c_int
    lib.gh_xf_group_norm_param_grads.argtypes = [V, V, V, I, I, I, I, C.c_float, V, V, V, C.c_size_t, V]
    lib.gh_xf_backward_params_workspace_bytes.restype = C.c_size_t
    lib.gh_xf_backward_params_workspace_bytes.argtypes = [C.POINTER(GhXfDims)]
    lib.gh_xf_backward_params.restype = C.c_int
    lib.gh_xf_backward_params.argtypes = [C.POINTER(GhXfDims), C.POINTER(GhXfStemT), C.POINTER(GhXfLayerT), C.POINTER(GhXfStem), C.POINTER(GhXfLayer),
                                          C.POINTER(GhXfStemG), C.POINTER(GhXfLayerG), V, V, V, V, V, C.c_size_t, V]


# ---- include/gh_lpips.h: the evaluator's perceptual score, LPIPS over AlexNet (a header of its own, as gh_conv.h is) ----
GH_LPIPS_RELU = 1
GH_LPIPS_MAX_C = 512
GH_LPIPS_PIXELS = 128
GH_LPIPS_CHUNK = 128
GH_LPIPS_FILL = 512
GH_LPIPS_FLAT_CIN = 16
GH_LPIPS_HEAD_PIXELS = 256
GH_LPIPS_TAPS = 5
GH_LPIPS_MIN_SIZE = 31
GH_LPIPS_PRED_HWC = 1
GH_LPIPS_GT_HWC = 2
GH_LPIPS_QUANTIZE = 4
GH_LPIPS_SIGNED = 8

LPIPS_SYMBOLS = ("gh_conv2d_weight_floats", "gh_conv2d_forward", "gh_maxpool3x3s2_forward", "gh_lpips_layer_workspace", "gh_lpips_layer",
                 "gh_lpips_prepare", "gh_lpips_workspace", "gh_lpips_forward")


class GhLpipsWeights(C.Structure):
    """The frozen parameters of gh_lpips_forward: fifteen pointers in the header's order."""
    _fields_ = [("w", C.c_void_p * GH_LPIPS_TAPS), ("b", C.c_void_p * GH_LPIPS_TAPS), ("lin", C.c_void_p * GH_LPIPS_TAPS)]


def declare_lpips(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol include/gh_lpips.h declares."""
    V, I, U, L = C.c_void_p, C.c_int, C.c_uint32, C.c_longlong
    lib.gh_conv2d_weight_floats.restype = C.c_size_t
    lib.gh_conv2d_weight_floats.argtypes = [I, I, I]
    lib.gh_conv2d_forward.restype = C.c_int
    lib.gh_conv2d_forward.argtypes = [V, I, I, I, I, I, I, I, I, V, V, U, I, V, V]
    lib.gh_maxpool3x3s2_forward.restype = C.c_int
    lib.gh_maxpool3x3s2_forward.argtypes = [V, I, I, I, I, V, V]
    lib.gh_lpips_layer_workspace.restype = C.c_size_t
    lib.gh_lpips_layer_workspace.argtypes = [I, L]
    lib.gh_lpips_layer.restype = C.c_int
    lib.gh_lpips_layer.argtypes = [V, I, L, I, V, I, V, V, V, C.c_size_t, V]
    lib.gh_lpips_prepare.restype = C.c_int
    lib.gh_lpips_prepare.argtypes = [V, V, V, V, I, I, I, I, I, U, V, V, V, V]
    lib.gh_lpips_workspace.restype = C.c_size_t
    lib.gh_lpips_workspace.argtypes = [I, I, I, C.POINTER(I)]
    lib.gh_lpips_forward.restype = C.c_int
    lib.gh_lpips_forward.argtypes = [V, I, I, I, C.POINTER(I), C.POINTER(GhLpipsWeights), V, V, V, C.c_size_t, V]


ALL_SYMBOLS = (EXPORTED_SYMBOLS + METRICS_SYMBOLS + POOL_SYMBOLS + HEAD_SYMBOLS + VERT_SYMBOLS + PLANE_SYMBOLS + ATTN_SYMBOLS + UVD_SYMBOLS +
               COND_SYMBOLS + RES_SYMBOLS + ATTN_ROWS_SYMBOLS + SCENE_SYMBOLS + TRUNK_SYMBOLS + CONV_SYMBOLS + MANO_SYMBOLS + XF_SYMBOLS +
               LPIPS_SYMBOLS)


def declare(lib: C.CDLL) -> None:
    """Attach argtypes/restypes for every symbol of the seventeen headers (ALL_SYMBOLS)."""
    for one in (declare_raster, declare_metrics, declare_pool, declare_head, declare_vert, declare_plane, declare_attn, declare_uvd, declare_cond, declare_res,
                declare_attn_rows, declare_scene, declare_trunk, declare_conv, declare_mano, declare_xf, declare_lpips):
        one(lib)
