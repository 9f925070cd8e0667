"""One call through the C-ABI of include/gh_raster.h. rasterizer.py is the module callers import."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, NamedTuple, Optional

import torch

from . import _abi, _lib
from ._raster_state import (DepthBoundCache, GeometryCache, GhOverflowError, GhStaleGeometryError, _DeviceState, _SPLIT_AUTO_MIN_PIXELS,
                            _STALE_MSG, _grow_capacity, _initial_capacity, _learn_depth24, _policy, _record, _state, _ws_acquire,
                            _ws_release, check_overflow, counter_word)


def _raw_stream(dev: torch.device) -> int:
    """Handle of the caller's current stream on `dev` (the torch.cuda.current_stream() object costs ~10 us of host time)."""
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


class _OnDevice:
    """`with torch.cuda.device(dev)` only when `dev` is not already current (the context manager costs ~10 us per call)."""
    __slots__ = ("ctx",)

    def __init__(self, dev: torch.device):
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.ctx = None if torch.cuda.current_device() == idx else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _ptr(t: Optional[torch.Tensor]):
    # (a plain int: a ctypes pointer FIELD takes it as it stands — thirty c_void_p objects per call were thirty GC-tracked
    # allocations per call for nothing)
    return None if t is None else t.data_ptr()


def _prep(t: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.device != dev:
        raise ValueError(f"tensor on {t.device}, expected {dev}")
    if t.dtype is torch.float32 and t.is_contiguous():          # the common case: only the pointer is needed
        return t
    return t.detach().to(torch.float32).contiguous()


class _Ctx:
    """What a forward leaves for its backward and for calls over its tile lists. call: its _Call (the launch's flags: dims.flags)."""
    __slots__ = ("call", "dims", "inp", "ws", "stream", "alpha", "radii", "parent", "refresh", "pending", "verdict", "l1", "fit",
                 "defer_loss", "__weakref__")

    def __init__(self, call: _Call, dims, inp, ws, stream, alpha, radii, parent, refresh: bool, l1, fit):
        self.call, self.dims, self.inp, self.ws, self.stream, self.alpha, self.radii = call, dims, inp, ws, stream, alpha, radii
        self.parent, self.refresh = parent, refresh
        self.pending = self.verdict = None             # the counter read-back of a sync-free call (see _forward_full)
        self.l1 = l1                                   # (loss, dL/dimage) of a fused image loss (GhOutputs.l1_*), else None
        self.fit = fit                                 # (loss, dL/dimage, dL/dalpha) of a fused fit loss (GhOutputs.fit_loss), else None
        # GH_FLAG_DEFER_LOSS_SUM: the fused loss's final sum is the backward's to write (GhGrads.deferred_loss)
        self.defer_loss = bool(dims.flags & _abi.GH_FLAG_DEFER_LOSS_SUM)

    def __del__(self):
        try:
            _ws_release(self.ws, self.stream)
        except Exception:                      # interpreter shutdown
            pass


class _Call(NamedTuple):
    """One call's arguments after validation: prepared tensors and the shape / flag words derived from them."""
    t: dict
    rows: int
    NV: int
    P: int
    M: int
    flags: int
    wpg: bool
    b_rgb: bool
    split: bool
    H: int
    W: int
    sh_degree: int
    scale_modifier: float
    cams_obj: object          # the caller's camera tensor as passed (identity: DepthBoundCache)


def _prepare_call(dev, cams, means3D, opacities, scales, rotations, H, W, shs, colors_precomp, sh_degree, scale_modifier, xyz_b,
                  opacity_b, color_w, color_b, per_view_gaussians, split_streams, plain: bool, cov3D_precomp=None) -> _Call:
    """Validate the arguments of raster_forward and derive rows / P / flags. plain: a full forward without static lists (the only
    kind that may be split over two streams)."""
    if (shs is None) == (colors_precomp is None):
        raise ValueError("Please provide exactly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise ValueError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    t = dict(cov3D=_prep(cov3D_precomp, dev), cams=_prep(cams, dev).reshape(-1, _abi.GH_CAM_FLOATS), means3D=_prep(means3D, dev),
             opacities=_prep(opacities, dev).reshape(-1), scales=_prep(scales, dev), rotations=_prep(rotations, dev),
             shs=_prep(shs, dev), colors_precomp=_prep(colors_precomp, dev), xyz_b=_prep(xyz_b, dev),
             opacity_b=None if opacity_b is None else _prep(opacity_b, dev).reshape(-1),
             color_w=_prep(color_w, dev), color_b=_prep(color_b, dev))
    rows, NV = t["means3D"].shape[0], t["cams"].shape[0]
    M = 0 if shs is None else t["shs"].shape[1]
    flags = 0
    if per_view_gaussians:
        if NV == 0 or rows % NV:
            raise ValueError("per_view_gaussians: the Gaussian tensors must hold n_views * P rows")
        flags |= _abi.GH_FLAG_PER_VIEW_GAUSSIANS
    P = rows // NV if per_view_gaussians else rows
    if split_streams is None:
        split_streams = _policy.split is True or (_policy.split == "auto" and NV >= 4 and H * W > _SPLIT_AUTO_MIN_PIXELS)
    split = bool(split_streams) and NV >= 2 and P > 0 and plain and not _policy.stage_timing
    if split:
        flags |= _abi.GH_FLAG_SPLIT_STREAMS
    wpg = False
    if t["color_w"] is not None:
        if t["color_w"].numel() == 48:
            pass
        elif t["color_w"].numel() == rows * 48:
            flags |= _abi.GH_FLAG_BLEND_W_PER_GAUSSIAN
            wpg = True
        else:
            raise ValueError("color_w must have 48 or P*48 elements")
    b_rgb = False
    if t["color_b"] is not None:
        if t["color_b"].numel() == rows * 3 and colors_precomp is not None:  # the 3 columns RGB mode reads (renderer_one_shot.py:328)
            flags |= _abi.GH_FLAG_BLEND_COLOR_B_RGB
            b_rgb = True
        elif t["color_b"].numel() != rows * 48:
            raise ValueError("color_b must have P*48 elements (or P*3 with colors_precomp)")
    return _Call(t, rows, NV, P, M, flags, wpg, b_rgb, split, int(H), int(W), int(sh_degree), float(scale_modifier), cams)


def _inputs_struct(c: _Call, bound=None):
    t = c.t
    return _abi.GhInputs(_ptr(t["cams"]), _ptr(t["means3D"]), _ptr(t["opacities"]), _ptr(t["scales"]), _ptr(t["rotations"]),
                         _ptr(t["shs"]), _ptr(t["colors_precomp"]), _ptr(t["xyz_b"]), _ptr(t["opacity_b"]),
                         _ptr(t["color_w"]), _ptr(t["color_b"]), _ptr(bound), _ptr(t["cov3D"]))


def stage_timing_summary() -> Dict[str, float]:
    """Average milliseconds per launch of each stage since enable_stage_timing(True) (current device)."""
    torch.cuda.synchronize()
    acc: Dict[str, list] = {}
    for name, e0, e1 in _state().stage_events:
        acc.setdefault(name, []).append(e0.elapsed_time(e1))
    return {k: sum(v) / len(v) for k, v in acc.items()}


def _run_stages(st: _DeviceState, fn, args, stages):
    """Call a *_stages entry point once per stage with events in between (same stream, same order)."""
    rc = 0
    for name, bit in stages:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args, C.c_uint32(bit))
        e1.record()
        st.stage_events.append((name, e0, e1))
        if rc != 0:
            break
    return rc


def _fused_loss(dev, image, alpha, l1_target, fit_loss, allowed: bool, defer_loss: bool):
    """Is an image loss fused into this call, and is its sum deferred: ((loss, dL/dimage) or None, (loss, dL/dimage, dL/dalpha) or
    None, GhOutputs' four trailing fields (l1_target / l1_dL_dimage / l1_loss / fit_loss), GH_FLAG_DEFER_LOSS_SUM or 0). The render
    kernel's epilogue computes the L1 form without a mask channel and the fit form with one, where the call allows it and the module
    policy is on; elsewhere the caller runs gh_l1_loss / gh_fit_loss on the stored images (loss.py does) and there is no sum to defer."""
    if not allowed or not _policy.fused_loss:
        return None, None, (None, None, None, None), 0
    defer = _abi.GH_FLAG_DEFER_LOSS_SUM if defer_loss else 0
    if l1_target is not None and alpha is None:
        if l1_target.shape != image.shape or l1_target.dtype is not torch.float32 or not l1_target.is_contiguous():
            raise ValueError("l1_target must be a contiguous float32 (n_views, 3, H, W) tensor")
        l1 = (torch.empty((), dtype=torch.float32, device=dev), torch.empty_like(image))
        return l1, None, (_ptr(l1_target), _ptr(l1[1]), _ptr(l1[0]), None), defer
    if fit_loss is not None and alpha is not None:
        gt_rgb, gt_mask, bbox, lam_l1, lam_m, scale = fit_loss
        NV, _, H, W = image.shape
        for t, shape in ((gt_rgb, (NV, H, W, 3)), (gt_mask, (NV, H, W)), (bbox, (NV, H, W))):
            if t is not None and (tuple(t.shape) != shape or t.dtype is not torch.float32 or not t.is_contiguous()):
                raise ValueError("fit_loss: gt_rgb (n_views,H,W,3), gt_mask and bbox (n_views,H,W) must be contiguous float32 tensors")
        fit = (torch.empty((), dtype=torch.float32, device=dev), torch.empty_like(image), torch.empty_like(alpha))
        rec = _abi.GhFitLoss(_ptr(gt_rgb), _ptr(gt_mask), _ptr(bbox), float(lam_l1), float(lam_m), float(scale), _ptr(fit[1]), _ptr(fit[2]),
                             _ptr(fit[0]))
        return None, fit, (None, None, None, C.pointer(rec)), defer   # (the pointer object keeps `rec` alive through the call)
    return None, None, (None, None, None, None), 0


def _launch(st, L, dev, c: _Call, flags: int, cap: int, return_alpha: bool, owner: Optional[_Ctx] = None, refresh: bool = False,
            depth_bound: Optional[DepthBoundCache] = None, bound=None, seen=None, l1_target=None, fit_loss=None, defer_loss=False):
    """The launch sequence of every forward. owner: the context whose tile lists this call walks (gh_forward_refresh with refresh,
    else gh_forward_shared); None: a full forward (gh_forward) with radii of its own. depth_bound / bound / seen: a full forward's
    occlusion bound. Returns (image, device view of the GhCounters — None for a shared call: they are the owner's —, context)."""
    image = torch.empty(c.NV, 3, c.H, c.W, dtype=torch.float32, device=dev)
    alpha = torch.empty(c.NV, c.H, c.W, dtype=torch.float32, device=dev) if return_alpha else None
    # (the library fuses no loss into a call with a depth bound or two streams)
    l1, fit, loss_fields, defer = _fused_loss(dev, image, alpha, l1_target, fit_loss, depth_bound is None and not c.split, defer_loss)
    dims = _abi.GhDims(c.P, c.NV, c.H, c.W, c.sh_degree, c.M, c.scale_modifier, flags | defer, cap)
    nbytes = L.gh_workspace_bytes(C.byref(dims))
    if nbytes == 0:
        raise RuntimeError("gh_workspace_bytes rejected the dimensions")
    # a refresh: the library applies THIS call's layout to the owner's workspace, and the arrays a refresh reads of it (cull_bound,
    # inst_c) lie behind the ones sized by the colour mode (sh_rgb, dmean_sh, sh_scratch: M != 0): the two calls must agree on it
    #  — and the owner's workspace must span this call's layout
    if refresh and ((owner.call.M != 0) != (c.M != 0) or owner.ws.numel() < nbytes):
        raise ValueError("refresh_of: the static lists were built in the other colour mode (shs vs colors_precomp); "
                         "build them again with this call's colour inputs")
    stream = _raw_stream(dev)
    ws = _ws_acquire(st, dev, nbytes, stream)
    if owner is None:
        # The launch-order hint in the workspace describes the cameras of the call that left it: other cameras (or a buffer
        # fresh from the allocator) -> GH_FLAG_FRESH_ORDER, the order by this call's own list lengths. Results are the same either way.
        # (the tensor OBJECT through a weak reference + its version counter: the address of a freed camera tensor is what the caching
        #  allocator hands to the next one, and so is a freed object's id())
        # A step being CAPTURED into a graph is replayed over this very buffer with this very camera tensor: from its second replay on
        # the hint is its own, and the flag would be baked into every replay — never set under capture.
        prev = getattr(ws, "_gh_cam_sig", None)
        if (prev is None or prev[0]() is not c.cams_obj or prev[1:] != (c.cams_obj._version, c.NV, c.H, c.W)) \
                and not torch.cuda.is_current_stream_capturing():
            dims.flags |= _abi.GH_FLAG_FRESH_ORDER
        ws._gh_cam_sig = (weakref.ref(c.cams_obj), c.cams_obj._version, c.NV, c.H, c.W)
        radii = torch.empty(c.NV, c.P, dtype=torch.int32, device=dev)
    else:
        radii = owner.radii                   # same geometry, same radii
    inp = _inputs_struct(c, bound)
    out = _abi.GhOutputs(_ptr(image), None if owner is not None else _ptr(radii), _ptr(alpha), _ptr(seen),
                         1.0 + (depth_bound.margin if depth_bound is not None else 0.0),
                         depth_bound.slack if depth_bound is not None else 0, *loss_fields)
    fn = L.gh_forward if owner is None else L.gh_forward_refresh if refresh else L.gh_forward_shared
    with _OnDevice(dev):
        if owner is not None:
            rc = fn(C.byref(dims), C.byref(inp), C.byref(out), C.c_void_p(owner.ws.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                    C.c_void_p(stream))
        elif _policy.stage_timing:
            rc = _run_stages(st, L.gh_forward_stages, (C.byref(dims), C.byref(inp), C.byref(out), C.c_void_p(ws.data_ptr()), nbytes,
                                                       C.c_void_p(stream)),
                             (("preprocess_fwd", _abi.GH_FWD_PREPROCESS), ("binning", _abi.GH_FWD_BINNING), ("render_fwd", _abi.GH_FWD_RENDER)))
        else:
            rc = fn(C.byref(dims), C.byref(inp), C.byref(out), C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn.__name__} failed: {_abi.status_name(rc)}")
    st.last_ws = ws
    counters = ws[:16].view(torch.int32) if owner is None or refresh else None
    return image, counters, _Ctx(c, dims, inp, ws, stream, alpha, radii, owner, refresh, l1, fit)


def _fits_owner(g0: _Ctx, c: _Call) -> bool:
    """A call over the tile lists of `g0` (geometry_of / refresh_of) has its shapes and its Gaussian layout."""
    o = g0.call
    return (o.P, o.NV, o.H, o.W, o.rows) == (c.P, c.NV, c.H, c.W, c.rows) and \
        (g0.dims.flags & _abi.GH_FLAG_PER_VIEW_GAUSSIANS) == (c.flags & _abi.GH_FLAG_PER_VIEW_GAUSSIANS)


def _forward_shared(st, L, dev, c: _Call, g0: _Ctx, return_alpha: bool):
    """gh_forward_shared: a second call over the lists of `g0` (the reference's mask pass after the RGB pass of a view)."""
    if c.t["shs"] is not None or (g0.dims.flags & _abi.GH_FLAG_SPLIT_STREAMS) or not _fits_owner(g0, c):
        raise ValueError("geometry_of: the second call must have the first one's shapes and precomputed colours")
    image, _, ctx = _launch(st, L, dev, c, c.flags, int(g0.dims.max_instances), return_alpha, g0)
    # the overflow flag is the geometry owner's; an overflow is the first call's (NaN image here too)
    ctx.pending, ctx.verdict = g0.pending, g0.verdict
    return image, g0.radii, ctx


def _forward_refresh(st, L, dev, c: _Call, g0: _Ctx, return_alpha: bool, sync, expect_backward: bool, l1_target=None, fit_loss=None,
                     defer_loss=False):
    """gh_forward_refresh: this call's opacities / colours over the static lists of `g0`."""
    if not (g0.dims.flags & _abi.GH_FLAG_STATIC_LISTS) or not _fits_owner(g0, c) or g0.parent is not None:
        raise ValueError("refresh_of: needs the context of a static_lists forward with this call's shapes")
    cap = int(g0.dims.max_instances)
    image, counters, ctx = _launch(st, L, dev, c, c.flags | _abi.GH_FLAG_STATIC_LISTS, cap, return_alpha, g0, True,
                                   l1_target=l1_target, fit_loss=fit_loss, defer_loss=defer_loss)
    auto = sync is None
    if sync is None:
        sync = not expect_backward
    if sync:
        w = counter_word(counters.tolist())
        st.last_D = w.d
        if w.stale or w.overflow:                   # (no depth sort in a refresh: nothing to learn about GH_FLAG_DEPTH24)
            GeometryCache.clear_all()
            if w.stale:
                raise GhStaleGeometryError(_STALE_MSG)
            raise GhOverflowError("the static tile lists were built by a call that overflowed its capacity; caches cleared")
    else:
        if not _policy.graph_mode:
            # a refresh whose opacity guard fired (or whose lists an overflow truncated) poisons every later step too: look at
            # the read-backs that have arrived, so that a stale loop surfaces within two calls instead of _PENDING_MAX
            check_overflow(block=False, keep_recent=2, dev=st.index)
        pc = _record(st, counters, cap, (c.P, c.NV, c.H, c.W, False), False)
        if auto:
            ctx.pending = pc
    return image, g0.radii, ctx


def _forward_full(st, L, dev, c: _Call, return_alpha: bool, sync, expect_backward: bool, max_instances, static_lists: bool,
                  depth_bound, l1_target=None, fit_loss=None, defer_loss=False):
    """gh_forward: projection, both sorts, lists, render — with the capacity / GH_FLAG_DEPTH24 / occlusion-bound policies around it
    (a synced call that the device flags is re-run with what it learned; a sync-free call is recorded for check_overflow)."""
    P, NV, H, W = c.P, c.NV, c.H, c.W
    key = (P, NV, H, W, c.split)
    if depth_bound is not None and (static_lists or _policy.graph_mode or P == 0 or NV * H * W < depth_bound.min_pixels):
        depth_bound = None                       # lists that outlive the call / a captured call / a small call: no per-call speculation
    base_flags = c.flags | (_abi.GH_FLAG_STATIC_LISTS if static_lists else 0)
    while True:
        cap = int(max_instances) if max_instances is not None else st.capacity.get(key, _initial_capacity(P, NV))
        # three depth-sort passes only for a shape a read-back has shown them to suffice for (_DeviceState.depth24)
        flags = base_flags | (_abi.GH_FLAG_DEPTH24 if st.depth24.get(key) is True else 0)
        bound, seen = depth_bound._buffers(dev, NV, H, W, key=(P, bool(c.flags & _abi.GH_FLAG_PER_VIEW_GAUSSIANS), c.cams_obj)) \
            if depth_bound is not None else (None, None)
        image, counters, ctx = _launch(st, L, dev, c, flags, cap, return_alpha, depth_bound=depth_bound, bound=bound, seen=seen,
                                       l1_target=l1_target, fit_loss=fit_loss, defer_loss=defer_loss)
        do_sync = sync
        if do_sync is None:
            # auto: read D back once per shape to size the capacity, then sync-free — but only for calls whose backward will
            # come (it checks this call's counters before it produces a gradient, see raster_backward). A call outside
            # autograd (inference) has no such second chance and reads D back like the reference wrapper does.
            do_sync = (max_instances is None and key not in st.capacity) or not expect_backward
            if not do_sync:
                check_overflow(block=False, keep_recent=2, dev=st.index)  # an overflow of an earlier sync-free call surfaces at most two calls late
        if not do_sync:
            # verdict: the counter read-back of a sync-free call, whoever is to ask for it; an explicit sync=False never blocks
            # (check_overflow() is the caller's job), an auto call's backward checks it first
            ctx.verdict = _record(st, counters, cap, key, True, depth_bound)
            if sync is None:
                ctx.pending = ctx.verdict
            return image, ctx.radii, ctx
        w = counter_word(counters.tolist())                   # the one host read-back, as in the reference wrapper
        st.last_D = w.d
        _learn_depth24(st, key, w.bits, w.d)
        if not (w.depth24_failed or w.overflow or w.bound_miss):
            if max_instances is None and key not in st.capacity:
                _grow_capacity(st, key, w.need(c.split), floor=1 << 16)
            return image, ctx.radii, ctx
        ctx.ws = None                                          # (the flagged attempt's workspace is dropped, not pooled)
        if w.depth24_failed:                                   # the three-pass depth sort does not cover this call's depths
            if depth_bound is not None:
                depth_bound.clear()
        elif w.overflow:
            if max_instances is not None:
                raise GhOverflowError(f"tile instances D={w.d} exceed max_instances={cap}")
            _grow_capacity(st, key, w.need(c.split))           # (above `cap`, the capacity it overflowed)
            if depth_bound is not None:
                depth_bound.clear()                            # (the truncated lists' report is not a bound)
        else:                                                  # the occlusion bound missed: the same call again, unbounded
            depth_bound.clear()
            depth_bound.misses += 1


def raster_forward(cams, means3D, opacities, scales, rotations, *, H: int, W: int, shs=None, colors_precomp=None,
                   sh_degree: int = 0, scale_modifier: float = 1.0, xyz_b=None, opacity_b=None, color_w=None,
                   color_b=None, max_instances: Optional[int] = None, sync: Optional[bool] = True, return_alpha: bool = False,
                   per_view_gaussians: bool = False, geometry_of: Optional["_Ctx"] = None,
                   split_streams: Optional[bool] = None, expect_backward: bool = False, static_lists: bool = False,
                   refresh_of: Optional["_Ctx"] = None, depth_bound: Optional[DepthBoundCache] = None, cov3D_precomp=None,
                   l1_target: Optional[torch.Tensor] = None, fit_loss=None, defer_loss: bool = False):
    """Low-level forward through the C-ABI. Returns (image (NV,3,H,W), radii (NV,P) int32, ctx);
    cov3D_precomp (P,6): the published module's precomputed 3-D covariance (xx xy xz yy yz zz, used as given: scale_modifier is
    not applied) in place of scales + rotations (pass None for both); its gradient comes back as "cov3D_precomp".
    with return_alpha the fused mask channel (NV,H,W) is available as ctx.alpha.
    per_view_gaussians (pose batch, the batch loop of GS3DRenderer.forward): every per-Gaussian tensor holds NV*P rows and
    view v renders rows [v*P, (v+1)*P) — NV different Gaussian sets in one launch sequence.
    geometry_of: context of an earlier forward with the SAME means3D / opacities / scales / rotations / cameras (apart from
    bg): this call re-uses its projection and tile lists (gh_forward_shared) and only walks the lists with its own colours —
    the reference's mask pass after the RGB pass of a view. Colours must be colors_precomp.
    split_streams (GH_FLAG_SPLIT_STREAMS, n_views >= 2): the views run as two halves on two HIP streams inside the library
    (forked from / joined into the current stream, graph-capturable); bit-identical images, radii and gradients.
    None = the module policy (set_split_streams).
    static_lists (GH_FLAG_STATIC_LISTS): build tile lists that stay valid for other opacities / colours (culling treats
    every opacity o as max(2, 2 o)); same image and gradients, larger D. refresh_of: context of such a forward with the SAME
    means3D / scales / rotations / xyz_b / cameras: this call (gh_forward_refresh) skips projection and sorts, refreshes the
    per-instance records with ITS opacities and colours (shs or colors_precomp) and walks the lists; forward bit-identical
    to a full call. An opacity above the lists' bound poisons the call (NaN image, GhStaleGeometryError). GeometryCache is
    the policy object on top of the two.
    depth_bound: a DepthBoundCache (full forwards only): instances behind the previous call's per-tile occlusion depth are
    not listed; verified by the forward, re-run without the bound on a miss.
    l1_target (n_views,3,H,W): fused image loss — ctx.l1 = (mean|image - l1_target|, its gradient w.r.t. image) from the render
    kernel's own epilogue (GhOutputs.l1_*). ctx.l1 is None where the library does not fuse it (alpha, a depth bound, two
    streams, shared calls): the caller then runs gh_l1_loss on the image (loss.py does).
    fit_loss (gt_rgb (n_views,H,W,3), gt_mask (n_views,H,W), bbox (n_views,H,W) or None, lambda_l1, lambda_mask, scale), with
    return_alpha: the fit's image loss the same way — ctx.fit = (loss, dL/dimage, dL/dalpha) (GhOutputs.fit_loss), None where
    it is not fused (loss.py then runs gh_fit_loss).
    defer_loss (GH_FLAG_DEFER_LOSS_SUM, with a fused loss only): the loss tensor of ctx.l1 / ctx.fit is written by this context's
    raster_backward (GhGrads.deferred_loss) instead of a one-workgroup sum kernel behind the forward; ctx.defer_loss says so.
    sync: True = read D back (and re-run with a larger capacity if needed); False = never block (check_overflow() is the
    caller's job); None = auto: read D back for the first call of a shape and for calls whose backward will not come
    (expect_backward False), otherwise sync-free with the check at the start of raster_backward.
    The three-pass depth sort (GH_FLAG_DEPTH24) is used only for call shapes a read-back has shown it to hold for: the first
    call of a shape, and every call of a loop that never reads its counters back, run the four-pass sort."""
    L = _lib.lib()
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("guassianhand_amd rasteriser needs tensors on a ROCm device (no CPU fallback)")
    plain = geometry_of is None and refresh_of is None and not static_lists
    c = _prepare_call(dev, cams, means3D, opacities, scales, rotations, H, W, shs, colors_precomp, sh_degree, scale_modifier, xyz_b,
                      opacity_b, color_w, color_b, per_view_gaussians, split_streams, plain, cov3D_precomp)
    st = _state(dev)
    with st.lock:
        if geometry_of is not None:
            return _forward_shared(st, L, dev, c, geometry_of, return_alpha)
        if refresh_of is not None:
            return _forward_refresh(st, L, dev, c, refresh_of, return_alpha, sync, expect_backward, l1_target, fit_loss, defer_loss)
        return _forward_full(st, L, dev, c, return_alpha, sync, expect_backward, max_instances, static_lists, depth_bound, l1_target,
                             fit_loss, defer_loss)


def cached_raster_forward(cache: Optional[GeometryCache], cams, means3D, opacities, scales, rotations, **kw):
    """raster_forward through a GeometryCache (None: a plain call). A hit re-uses the cached static tile lists
    (gh_forward_refresh); a miss is a full forward with static_lists=True whose context becomes the cache entry. With
    sync=True a refresh that finds an opacity above the lists' bound is re-run as a full call, transparently."""
    if cache is None:
        return raster_forward(cams, means3D, opacities, scales, rotations, **kw)
    if kw.get("geometry_of") is not None or kw.get("split_streams"):
        raise ValueError("a GeometryCache call takes neither geometry_of nor split_streams")
    xyz_b = kw.get("xyz_b")
    objs = (cams, means3D, scales, rotations, xyz_b)
    shs = kw.get("shs")
    vals = tuple(None if o is None else (o._version, tuple(o.shape), o.device) for o in objs) + \
        (int(kw["H"]), int(kw["W"]), float(kw.get("scale_modifier", 1.0)), bool(kw.get("per_view_gaussians", False)),
         # the colour mode: the workspace layout behind the static part depends on M (one cache used with
         # use_rgb=True and use_rgb=False is two entries, i.e. a miss)
         0 if shs is None else int(shs.shape[1]), int(kw.get("sh_degree", 0)))
    g0 = cache.lookup(objs, vals)
    if g0 is not None:
        try:
            out = raster_forward(cams, means3D, opacities, scales, rotations, refresh_of=g0,
                                 **{k: v for k, v in kw.items() if k != "max_instances"})
            cache.hits += 1
            return out
        except GhStaleGeometryError:               # (sync=True only) the caches are cleared: rebuild below
            pass
    image, radii, ctx = raster_forward(cams, means3D, opacities, scales, rotations, static_lists=True, split_streams=False, **kw)
    cache.store(objs, vals, ctx)
    cache.builds += 1
    return image, radii, ctx


def raster_backward(ctx: _Ctx, dL_dimage: Optional[torch.Tensor], want_means2D: bool = True,
                    dL_dalpha: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None,
                    want=None) -> Dict[str, torch.Tensor]:
    """grad_scale: optional one-element device tensor multiplied into dL_dimage / dL_dalpha as the kernel reads them
    (GhGrads.upstream_scale): the dL/dloss of a scalar loss whose image gradient was produced unscaled.
    want: the gradients to produce, a subset of {means3D, opacities, scales, rotations, shs, colors_precomp, xyz_b, opacity_b,
    color_w, color_b} (None = all): the others get a NULL pointer in GhGrads — with no geometry gradient asked for the
    per-Gaussian chain rule is skipped altogether (the one-shot fit trains colour / opacity biases only)."""
    L = _lib.lib()
    c = ctx.call
    t = c.t
    dev = t["means3D"].device
    st = _state(dev)
    if ctx.pending is not None and ctx.pending.resolve():
        # auto-sync forward (the drop-in's default): its counters are checked HERE, before any gradient exists — an overflowed
        # call returned a NaN image, and a NaN loss must not reach the caller's optimiser step. The forward finished long ago
        # on any host-bound loop, so this wait is normally free.
        with st.lock:
            st.geom_last = None                    # the re-run of the step must not be taken for this call's mask pass
        raise ctx.pending.error()
    P, NV, M, H, W = c.P, c.NV, c.M, c.H, c.W
    if dL_dimage is None:
        dL_dimage = torch.zeros(NV, 3, H, W, dtype=torch.float32, device=dev)
    g = dL_dimage.detach().to(torch.float32).reshape(NV, 3, H, W).contiguous()
    ga = None if dL_dalpha is None else dL_dalpha.detach().to(torch.float32).reshape(NV, H, W).contiguous()
    gs = None if grad_scale is None else grad_scale.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    R_ = c.rows                                  # rows of the per-Gaussian tensors (P, or NV*P for a pose batch)
    # ONE contiguous fp32 block for every gradient the kernels write (the C-ABI takes plain pointers, so they may all point
    # into one allocation): a single torch.empty per backward, and the sharded fit all-reduces `block` as it stands —
    # [4 caller floats | color_w | opacity_b | color_b | xyz_b | means3D | opacities | scales | rotations | colour | (means2D)]:
    # the blend-parameter gradients (what the one-shot fit trains) lead, so the fit reduces a short prefix.
    # Every part starts on a 16-byte boundary (the 48-wide rows are written as float4s).
    shapes = [("color_w", ((R_, 48) if c.wpg else (48,)) if t["color_w"] is not None else None),
              ("opacity_b", (R_,) if t["opacity_b"] is not None else None),
              ("color_b", (R_, 3 if c.b_rgb else 48) if t["color_b"] is not None else None),
              ("xyz_b", (3,) if t["xyz_b"] is not None else None),
              ("means3D", (R_, 3)), ("opacities", (R_,)), ("scales", (R_, 3) if t["scales"] is not None else None),
              ("rotations", (R_, 4) if t["rotations"] is not None else None), ("cov3D_precomp", (R_, 6) if t["cov3D"] is not None else None),
              ("shs", (R_, M, 3) if M else None), ("colors_precomp", (R_, 3) if t["colors_precomp"] is not None else None),
              ("means2D", (NV, P, 3) if want_means2D else None)]
    off, spans = 4, []                             # floats 0..3: reserved for the caller (e.g. the loss of the sharded fit)
    for k, shp in shapes:
        if shp is None or (want is not None and k != "means2D" and k not in want):
            continue
        n = 1
        for d_ in shp:
            n *= d_
        spans.append((k, shp, off, n))
        off += (n + 3) & ~3
    block = torch.empty(off, dtype=torch.float32, device=dev)
    o = {k: None for k, _ in shapes}
    for k, shp, a, n in spans:
        o[k] = block[a:a + n].view(shp)
    reducible = spans[-1][2] if (want_means2D and spans and spans[-1][0] == "means2D") else off   # means2D is per view: not part of the all-reduced prefix
    blend_end = 4
    for k, shp, a, n in spans:
        if k in ("color_w", "opacity_b", "color_b", "xyz_b"):
            blend_end = a + ((n + 3) & ~3)
    ctx_block = (block, reducible, [(k, shp, a, n) for k, shp, a, n in spans if k != "means2D"], blend_end)
    gr = _abi.GhGrads(dL_dimage=_ptr(g), dL_dalpha=_ptr(ga), dL_dmeans3D=_ptr(o["means3D"]), dL_dmeans2D=_ptr(o["means2D"]),
                      dL_dopacities=_ptr(o["opacities"]), dL_dscales=_ptr(o["scales"]), dL_drotations=_ptr(o["rotations"]),
                      dL_dshs=_ptr(o["shs"]), dL_dcolors=_ptr(o["colors_precomp"]), dL_dblend_xyz_b=_ptr(o["xyz_b"]),
                      dL_dblend_opacity_b=_ptr(o["opacity_b"]), dL_dblend_color_w=_ptr(o["color_w"]),
                      dL_dblend_color_b=_ptr(o["color_b"]), upstream_scale=_ptr(gs), dL_dcov3D=_ptr(o["cov3D_precomp"]),
                      deferred_loss=_ptr((ctx.l1 or ctx.fit)[0]) if ctx.defer_loss else None)
    stream = _raw_stream(dev)
    ctx.stream = stream                            # the workspace goes back to the pool of the stream that used it last
    with _OnDevice(dev):
        bargs = (C.byref(ctx.dims), C.byref(ctx.inp), C.byref(gr), C.c_void_p(ctx.ws.data_ptr()), ctx.ws.numel(),
                 C.c_void_p(stream))
        if ctx.parent is not None:
            fn = L.gh_backward_refresh if ctx.refresh else L.gh_backward_shared
            rc = fn(C.byref(ctx.dims), C.byref(ctx.inp), C.byref(gr), C.c_void_p(ctx.parent.ws.data_ptr()),
                    C.c_void_p(ctx.ws.data_ptr()), ctx.ws.numel(), C.c_void_p(stream))
        elif _policy.stage_timing:
            rc = _run_stages(st, L.gh_backward_stages, bargs, (("render_bwd", _abi.GH_BWD_RENDER),
                                                            ("preprocess_bwd", _abi.GH_BWD_PREPROCESS)))
        else:
            rc = L.gh_backward(*bargs)
    if rc != 0:
        raise RuntimeError(f"gh_backward failed: {_abi.status_name(rc)}")
    st.last_grad_block = ctx_block
    return {k: v for k, v in o.items() if v is not None}


def workspace_counters(ctx: _Ctx):
    """GhCounters of a forward as a host list [num_rendered, overflow, reserved0, reserved1] (synchronises; tests / tools)."""
    return [c & 0xFFFFFFFF for c in ctx.ws[:16].view(torch.int32).tolist()]


def workspace_views(ctx: _Ctx) -> Dict[str, torch.Tensor]:
    """Typed views of the internal stage arrays (for tests / profiling), via gh_workspace_layout."""
    L = _lib.lib()
    lay = _abi.GhLayout()
    L.gh_workspace_layout(C.byref(ctx.dims), C.byref(lay))
    if ctx.dims.flags & _abi.GH_FLAG_SPLIT_STREAMS:
        raise ValueError("workspace_views: a split call keeps two sets of per-instance arrays; render with split_streams=False")
    c = ctx.call
    ws, N, cap = ctx.ws, c.NV * c.P, int(ctx.dims.max_instances)
    gx, gy = (c.W + 15) // 16, (c.H + 15) // 16
    pix = c.NV * c.H * c.W

    def v(off, nbytes, dtype, *shape):
        return ws[off:off + nbytes].view(dtype).reshape(*shape)

    geom = v(lay.geom, N * 64, torch.float32, N, 16)
    sorted_tile = v(lay.keys_a, cap * 4, torch.int32, cap)
    if L.gh_partition_is_per_view(C.byref(ctx.dims)) == 1:      # the keys hold tile ids inside the view: the global id through the payload's view
        sorted_tile = sorted_tile + (v(lay.vals_a, cap * 4, torch.int32, cap).clamp(0, max(N - 1, 0)) // max(c.P, 1)) * (gx * gy)
    return dict(counters=v(lay.counters, 16, torch.int32, 4), g0=geom[:, 0:4], g1=geom[:, 4:8], gb=geom[:, 8],
                # (view-space depth and 3-sigma tile rect of every projected Gaussian: the geometry line's last float4, v0.8)
                depth=geom[:, 13], rect=geom[:, 14].contiguous().view(torch.int32),
                tiles_touched=v(lay.tiles_touched, N * 4, torch.int32, N), slot_begin=v(lay.slot_begin, N * 4, torch.int32, N),
                depth_order=v(lay.depth_vals_b if (ctx.dims.flags & _abi.GH_FLAG_DEPTH24) else lay.depth_vals_a, N * 4, torch.int32, N),
                sorted_tile=sorted_tile, sorted_slot=v(lay.sorted_slot, cap * 4, torch.int32, cap),
                sorted_gid=v(lay.vals_a, cap * 4, torch.int32, cap),
                inst_r2=v(lay.inst_r2, cap * 8, torch.int32, cap, 2),
                ranges=v(lay.ranges, c.NV * gx * gy * 8, torch.int32, c.NV * gx * gy, 2),
                final_T=v(lay.final_T, pix * 4, torch.float32, c.NV, c.H, c.W),
                n_contrib=v(lay.n_contrib, pix * 4, torch.int32, c.NV, c.H, c.W))
