"""Drop-in replacement for `diff_gaussian_rasterization` as used by the reference.

Mirrors the call protocol of tgs/models/renderer_one_shot.py:281-296, :338-346, :355-379:

    raster_settings = GaussianRasterizationSettings(image_height=..., image_width=..., tanfovx=..., tanfovy=...,
        bg=..., scale_modifier=..., viewmatrix=..., projmatrix=..., sh_degree=..., campos=...,
        prefiltered=False, debug=False)
    rendered_image, radii = GaussianRasterizer(raster_settings=raster_settings)(
        means3D=..., means2D=..., shs=..., colors_precomp=..., opacities=..., scales=..., rotations=...,
        cov3D_precomp=None)

plus `rasterize_views`, the view-batched entry with the attribute blend of :298-334 fused into the
kernels. All compute goes through the C-ABI of include/gh_raster.h (hand-written HIP for gfx950);
there is no PyTorch/CPU fallback — a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import collections
import weakref
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .camera import pack_camera
# (the names not used below are re-exported: callers, tests and tools reach them through this module)
from ._raster_state import (CounterWord, DepthBoundCache, GeometryCache, GhDepthBoundMiss, GhOverflowError, GhStaleGeometryError,
                            _DEPTH24_MSG, _DeviceState, _MISS_MSG, _PENDING_MAX, _Pending, _Policy, _SPLIT_AUTO_MIN_PIXELS, _STALE_MSG,
                            _WS_POOL_DEPTH, _dev_index, _grow_capacity, _initial_capacity, _learn_depth24, _policy, _queue_readback,
                            _record, _state, _states, _states_lock, _ws_acquire, _ws_release, capacity_key, check_overflow,
                            clear_workspace_pool, counter_word, enable_stage_timing, graph_counters, last_grad_block, last_guard,
                            last_num_rendered, report_counter_word, set_fused_loss, set_geometry_reuse, set_graph_mode,
                            set_split_streams)
from ._raster_launch import (_Call, _Ctx, _OnDevice, _fits_owner, _forward_full, _forward_refresh, _forward_shared, _fused_loss,
                             _inputs_struct, _launch, _prep, _prepare_call, _ptr, _raw_stream, _run_stages, cached_raster_forward,
                             raster_backward, raster_forward, stage_timing_summary, workspace_counters, workspace_views)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _geometry_key(means3D, opacities, scales, rotations, rs):
    objs = (means3D, opacities, scales, rotations, rs.viewmatrix, rs.projmatrix, rs.campos)
    vals = tuple(o._version for o in objs) + (int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy),
                                               float(rs.scale_modifier), _raw_stream(means3D.device))
    return objs, vals


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, raster_settings, sync, expect_backward,
                cov3D_precomp=None):
        rs = raster_settings
        cams = pack_camera(rs.viewmatrix, rs.projmatrix, rs.campos, rs.tanfovx, rs.tanfovy, rs.bg)
        parent = None
        st = _state(means3D.device)
        if _policy.reuse_geometry:
            # Only the documented pair is shared: the call DIRECTLY after a full call, with the very same (unmodified, `is` +
            # `_version`) geometry tensors and camera on the same stream, precomputed colours, while the first call's context is
            # still alive (its backward has not run). The record holds weak references and is dropped after one reuse, so
            # nothing of an earlier step can be picked up. (An in-place update through `.data` does not move `_version`:
            # between an RGB call and its mask call nothing updates parameters.)
            # (shape of the Gaussians: scales + rotations, or the precomputed covariance in both places)
            objs, vals = _geometry_key(means3D, opacities, scales if cov3D_precomp is None else cov3D_precomp,
                                       rotations if cov3D_precomp is None else cov3D_precomp, rs)
            with st.lock:
                g, st.geom_last = st.geom_last, None
            if g is not None and sh is None and g[1] == vals and all(a() is b for a, b in zip(g[0], objs)):
                parent = g[2]()                    # alive until its backward has run
                # never the lists of a call that overflowed: its verdict is known when its counters were read already (the caller
                # has been told, and this IS the re-run the message asks for — found by tools/fuzz_dropin.py --shrink), and a call
                # that reads D back itself (sync=True, or an inference call) asks now
                p = None if parent is None else parent.verdict
                if p is not None and (p.done or sync is True or (sync is None and not expect_backward)) and p.resolve():
                    parent = None
        image, radii, rctx = raster_forward(
            cams, means3D, opacities, scales, rotations, H=int(rs.image_height), W=int(rs.image_width),
            shs=sh, colors_precomp=colors_precomp, sh_degree=int(rs.sh_degree),
            scale_modifier=float(rs.scale_modifier), sync=sync, geometry_of=parent,
            expect_backward=expect_backward, cov3D_precomp=cov3D_precomp)
        if _policy.reuse_geometry and parent is None:
            with st.lock:
                st.geom_last = (tuple(weakref.ref(o) for o in objs), vals, weakref.ref(rctx))
        ctx.rctx = rctx
        # the backward kernels read these tensors again, through the pointers the context holds: registering them makes autograd
        # raise its usual "modified by an inplace operation" error when one of them was written between forward and backward,
        # as it does for the reference extension (which saves them) — instead of gradients of a scene that never existed
        ctx.save_for_backward(*[t for t in (means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp) if t is not None])
        ctx.shapes = (means3D.shape, means2D.shape, None if sh is None else sh.shape,
                      None if colors_precomp is None else colors_precomp.shape, opacities.shape,
                      None if scales is None else scales.shape, None if rotations is None else rotations.shape,
                      None if cov3D_precomp is None else cov3D_precomp.shape)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return image[0], radii[0]

    @staticmethod
    def backward(ctx, grad_image, _grad_radii):
        ctx.saved_tensors                                  # (version check of the inputs, see forward)
        g = raster_backward(ctx.rctx, grad_image)
        ctx.rctx = None
        s = ctx.shapes
        return (g["means3D"].reshape(s[0]), g["means2D"][0].reshape(s[1]),
                g["shs"].reshape(s[2]) if s[2] is not None else None,
                g["colors_precomp"].reshape(s[3]) if s[3] is not None else None,
                g["opacities"].reshape(s[4]), g["scales"].reshape(s[5]) if s[5] is not None else None,
                g["rotations"].reshape(s[6]) if s[6] is not None else None, None, None, None,
                g["cov3D_precomp"].reshape(s[7]) if s[7] is not None else None)


def _any_global_hook() -> bool:
    m = torch.nn.modules.module
    f = getattr(m, "_has_any_global_hook", None)
    if f is not None:
        return bool(f())
    return bool(getattr(m, "_global_forward_hooks", None) or getattr(m, "_global_forward_pre_hooks", None) or
                getattr(m, "_global_backward_hooks", None) or getattr(m, "_global_backward_pre_hooks", None))


class GaussianRasterizer(nn.Module):
    """Same constructor / call keywords / 2-tuple return as the module the reference imports at
    tgs/models/renderer_one_shot.py:3 and calls at :338-346 and :372-379."""

    def __init__(self, raster_settings: GaussianRasterizationSettings, sync: Optional[bool] = None):
        """sync=None (default): the first call of an image / Gaussian-count shape reads the instance count D back once to size
        the workspace capacity (1.5 D + 1024); later calls under autograd are sync-free in the forward, and their BACKWARD first
        checks the forward's counters (an event that completed long before on a host-bound loop): an overflowed call — which
        returned a NaN image, device-side guard — raises GhOverflowError there, before a gradient exists, with the capacity
        already raised; the caller's optimiser never sees the NaN. Calls outside autograd (inference: no backward will come)
        read D back like the reference wrapper and re-run transparently with a larger capacity.
        sync=True reads D back on every call like the reference wrapper does; sync=False never blocks (check_overflow())."""
        super().__init__()
        self.raster_settings = raster_settings
        self.sync = sync

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        # (cov3D_precomp: the reference never passes it, renderer_one_shot.py:313, :346; supported since round 5 — the covariance is
        # used as given, scale_modifier is not applied, and its gradient flows back like the published module's)
        if means3D.shape[0] == 0:
            # No Gaussians. The published wrapper skips the kernels then (`if(P != 0)` around the rasteriser call in the extension's
            # RasterizeGaussiansCUDA — third-party source, not in the reference tree) and returns the image it allocated: ZEROS, not the
            # background. The drop-in returns what the published module returns; the C-ABI / raster_forward composite the background
            # over nothing (T = 1), which is what App. A's formulas give. Connected to the graph so that a backward yields empty gradients.
            rs = self.raster_settings
            img = torch.zeros(3, int(rs.image_height), int(rs.image_width), dtype=torch.float32, device=means3D.device)
            return img + 0.0 * means3D.sum(), torch.zeros(0, dtype=torch.int32, device=means3D.device)
        # will a backward come? (decided here: inside an autograd Function's forward the grad mode is always off, and
        # needs_input_grad ignores torch.no_grad())
        expect_backward = torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp))
        # (The reference wraps the call in torch.autocast(dtype=float32), renderer_one_shot.py:337. Nothing below is an autocast-
        # eligible torch op — tensors go to the C-ABI as raw pointers after an explicit float32 check in _prep — so no
        # autocast(enabled=False) context is entered here: it cost 6 us per call for nothing.)
        return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                         self.raster_settings, self.sync, expect_backward, cov3D_precomp)

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """The published module's frustum test (its `mark_visible`: a point is visible when its view-space depth exceeds 0.2 — the
        near cull of App. A.1; the reference never calls it). (P,) bool, no gradient. A handful of torch ops on the caller's device:
        not part of the render path."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.to(positions.dtype)      # row-vector convention: p_view = [x y z 1] @ viewmatrix
            return (positions[:, 0] * vm[0, 2] + positions[:, 1] * vm[1, 2] + positions[:, 2] * vm[2, 2] + vm[3, 2]) > 0.2

    # nn.Module.__call__ runs the hook machinery around forward(); this module never has hooks worth 3 us per call on a path
    # that is called twice per view (hooks registered by a caller are honoured: fall back to the full protocol then)
    def __call__(self, *args, **kwargs):
        if self._forward_hooks or self._forward_pre_hooks or self._backward_hooks or self._backward_pre_hooks or _any_global_hook():
            return super().__call__(*args, **kwargs)
        return self.forward(*args, **kwargs)


# ---------------------------------------------------------------------------------------------------
# The view-batched autograd nodes, _RasterizeViews (rasterize_views) and loss._RenderedLoss (rendered_*_loss), are applied through
# _apply_views as node.apply(_ViewArgs, cams, xyz, opacity, scaling, rotation, shs, xyz_b, opacity_b, color_w, color_b) and share
# _views_forward / _views_backward. _ViewArgs.spec: the loss node's ("l1", target) or ("fit", gt_rgb, gt_mask, bbox, lambdas, scale).
_ViewArgs = collections.namedtuple("_ViewArgs", "cache depth_bound H W sh_degree scale_modifier use_rgb sync max_instances return_alpha "
                                                "per_view defer_loss spec")
_GRAD_AT = 2        # needs_input_grad[_GRAD_AT:]: the nine Gaussian tensors (behind the _ViewArgs and the cameras)
_GRAD_NAMES = tuple(("means3D", "opacities", "scales", "rotations", colour, "xyz_b", "opacity_b", "color_w", "color_b")
                    for colour in ("shs", "colors_precomp"))                                # [use_rgb]


def _apply_views(node, cams, xyz, opacity, scaling, rotation, shs, *, H: int, W: int, use_rgb: bool, sh_degree: int = 3,
                 scale_modifier: float = 1.0, xyz_b=None, opacity_b=None, color_w=None, color_b=None, sync: bool = True,
                 max_instances: Optional[int] = None, return_alpha: bool = False, per_view_gaussians: bool = False,
                 geometry_cache=None, depth_bound: Optional[DepthBoundCache] = None, defer_loss: bool = False, spec=None, who: str = ""):
    """geometry_cache / depth_bound become (GeometryCache or None, DepthBoundCache or None) here, once: a DepthBoundCache passed as
    geometry_cache is the depth bound (fit.OneShotFit passes either kind). who: the caller's prefix of the error message."""
    if depth_bound is not None:
        if geometry_cache is not None:
            raise ValueError(who + "geometry_cache (static geometry) or depth_bound (moving geometry), not both")
    elif isinstance(geometry_cache, DepthBoundCache):
        geometry_cache, depth_bound = None, geometry_cache
    a = _ViewArgs(geometry_cache, depth_bound, int(H), int(W), int(sh_degree if not use_rgb else 0), float(scale_modifier), bool(use_rgb),
                  bool(sync), max_instances, bool(return_alpha), bool(per_view_gaussians), bool(defer_loss), spec)
    return node.apply(a, cams, xyz, opacity, scaling, rotation, shs, xyz_b, opacity_b, color_w, color_b)


def _views_forward(ctx, a: _ViewArgs, cams, gaussians, l1_target=None, fit_loss=None):
    xyz, opacity, scaling, rotation, shs, xyz_b, opacity_b, color_w, color_b = gaussians
    image, radii, rctx = cached_raster_forward(a.cache, cams, xyz, opacity, scaling, rotation, H=a.H, W=a.W, sh_degree=a.sh_degree,
                                               scale_modifier=a.scale_modifier, xyz_b=xyz_b, opacity_b=opacity_b, color_w=color_w,
                                               color_b=color_b, sync=a.sync, max_instances=a.max_instances, return_alpha=a.return_alpha,
                                               per_view_gaussians=a.per_view, depth_bound=a.depth_bound,
                                               shs=None if a.use_rgb else shs,
                                               colors_precomp=shs.reshape(shs.shape[0], 3) if a.use_rgb else None,
                                               l1_target=l1_target, fit_loss=fit_loss, defer_loss=a.defer_loss)
    ctx.rctx, ctx.use_rgb = rctx, a.use_rgb
    # (the backward kernels re-read the inputs through the context's pointers: autograd's version check, see _RasterizeGaussians)
    ctx.save_for_backward(*[t for t in (cams,) + gaussians if t is not None])
    ctx.shapes = [None if t is None else t.shape for t in gaussians]
    ctx.set_materialize_grads(False)             # an output that carries no gradient arrives as None, not as a zero image
    ctx.mark_non_differentiable(radii)
    return image, radii, rctx


def _views_backward(ctx, dL_dimage, dL_dalpha, grad_scale=None):
    ctx.saved_tensors                                  # inputs written in place since the forward: autograd's own error
    names = _GRAD_NAMES[ctx.use_rgb]
    wanted = {n for n, need in zip(names, ctx.needs_input_grad[_GRAD_AT:]) if need}     # only the gradients autograd asks for
    g = raster_backward(ctx.rctx, dL_dimage, want_means2D=False, dL_dalpha=dL_dalpha, grad_scale=grad_scale, want=wanted)
    ctx.rctx = None
    return (None,) * _GRAD_AT + tuple(g[n].reshape(s) if s is not None and n in g else None for n, s in zip(names, ctx.shapes))


class _RasterizeViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, cams, *gaussians):
        image, radii, rctx = _views_forward(ctx, a, cams, gaussians)
        alpha = rctx.alpha if a.return_alpha else image.new_zeros(0)
        if not a.return_alpha:
            ctx.mark_non_differentiable(alpha)
        return image, alpha, radii

    @staticmethod
    def backward(ctx, grad_image, grad_alpha, _gr):
        return _views_backward(ctx, grad_image, grad_alpha if ctx.rctx.alpha is not None else None)


def rasterize_views(cams: torch.Tensor, xyz, opacity, scaling, rotation, shs, *, H: int, W: int, use_rgb: bool,
                    sh_degree: int = 3, scale_modifier: float = 1.0, xyz_b=None, opacity_b=None, color_w=None,
                    color_b=None, sync: bool = True, max_instances: Optional[int] = None, return_alpha: bool = False,
                    per_view_gaussians: bool = False, geometry_cache: Optional[GeometryCache] = None,
                    depth_bound: Optional[DepthBoundCache] = None):
    """View-batched render with the attribute blend of renderer_one_shot.py:298-334 fused into the kernels.
    per_view_gaussians=True renders a POSE BATCH: the Gaussian tensors hold Nv*P rows and camera v sees rows
    [v*P, (v+1)*P) only — the batch loop of GS3DRenderer.forward (renderer_one_shot.py:615-633) in one launch sequence.

    cams: (Nv, GH_CAM_FLOATS) from camera.pack_cameras_from_w2c; returns (images (Nv,3,H,W), radii (Nv,P)) or, with
    return_alpha, (images, alpha (Nv,H,W), radii): alpha is the reference's mask render (colour 1, bg 0,
    renderer_one_shot.py:353-380) produced by the same pass as a 4th channel (bit-identical to a separate pass).
    Differentiable w.r.t. xyz, opacity, scaling, rotation, shs and the blend parameters (through image and alpha); only
    the gradients autograd needs are computed. geometry_cache: see GeometryCache (static Gaussians and cameras);
    depth_bound: see DepthBoundCache (Gaussians that move a little between steps) — one or the other.
    """
    image, alpha, radii = _apply_views(_RasterizeViews, cams, xyz, opacity, scaling, rotation, shs, H=H, W=W, use_rgb=use_rgb,
                                       sh_degree=sh_degree, scale_modifier=scale_modifier, xyz_b=xyz_b, opacity_b=opacity_b,
                                       color_w=color_w, color_b=color_b, sync=sync, max_instances=max_instances,
                                       return_alpha=return_alpha, per_view_gaussians=per_view_gaussians,
                                       geometry_cache=geometry_cache, depth_bound=depth_bound, who="rasterize_views: ")
    return (image, alpha, radii) if return_alpha else (image, radii)


# ---------------------------------------------------------------------------------------------------
# Names of the module-level state of rounds 1-4, kept readable for tests and tools: they resolve to the CURRENT device's state /
# the policy object (PEP 562). Code in this package uses _state(dev) / _policy directly.
_LEGACY_STATE = {"_capacity": "capacity", "_depth24": "depth24", "_pending": "pending", "_free_slots": "free_slots", "_last_D": "last_D",
                 "_last_ws": "last_ws", "_graph_counters": "graph_counters", "_ws_pool": "ws_pool", "_geom_last": "geom_last",
                 "_last_grad_block": "last_grad_block", "_stage_events": "stage_events"}
_LEGACY_POLICY = {"_graph_mode": "graph_mode", "_split_policy": "split", "_reuse_geometry": "reuse_geometry", "_stage_timing": "stage_timing"}


def __getattr__(name):
    if name in _LEGACY_STATE:
        return getattr(_state(), _LEGACY_STATE[name])
    if name in _LEGACY_POLICY:
        return getattr(_policy, _LEGACY_POLICY[name])
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
