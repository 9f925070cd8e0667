"""The Gaussian head: the reference's GSLayer (tgs/models/renderer_one_shot.py:156-214) — five nn.Linear heads over the same (P,Cin)
feature block and the activations behind them — as one HIP pass forward and one backward, through include/gh_head.h.

    gs_head(x, pts, weight, bias, shs_width=..., use_rgb=..., ...)  -> renderer.GaussianModel

`weight` (O,Cin) and `bias` (O) are the five heads' parameters concatenated in the order of the reference's `feature_channels`
(xyz 3, scaling 3, rotation 4, opacity 1, shs `shs_width`), O = 11 + shs_width. The call is differentiable in x, pts, weight and bias;
when neither weight nor bias needs a gradient (the frozen head of the one-shot fit, where only `map_bias` trains through it) the
backward is one launch that writes grad_x and grad_pts and does none of the weight-gradient reduction. x is read in place through its
row stride (a column window of a wider tensor is not copied). Every sum has a fixed order that depends on (Cin, O) alone — and on P
for the weight gradient — and there are no atomics: a row's outputs and its grad_x are bitwise the same alone or among 100,000 rows,
and weight gradients are bitwise reproducible run to run.

CPU tensors, and `ops="torch"` on any device, go through `gs_head_ref`: `renderer.gs_activations` over one `F.linear`, in float64 on
request (the yardstick of the GPU tests). ROCm tensors go through the HIP kernels only.

`GSLayer` is the module itself with the reference's state-dict keys (`out_layers.{0..4}.{weight,bias}`) and initialisation, so a
reference checkpoint loads unchanged; `fused_gs_layer_cls(base)` grafts the same forward onto the reference's own class, and
`fuse_gs_head(renderer)` swaps the class of `renderer.gs_net` for it (parameters untouched) — what the config strings
`guassianhand_amd.tgs_renderer.GS3DRendererFusedHead` / `GS3DRendererEditFusedHead` do in `configure()`."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam
from ._call import check_f32, check_ops, cotangent, launch, lib, ptr, row_stride, rows, workspace
from .renderer import GaussianModel, gs_activations

FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")          # the order of the concatenated rows (gh_head.h)
FIXED_WIDTHS = {"xyz": 3, "scaling": 3, "rotation": 4, "opacity": 1}
SHS_WIDTHS = (3, 12, 27, 48)


def head_config(shs_width, use_rgb, xyz_offset, restrict_offset, clip_scaling) -> tuple:
    """The head's configuration as the autograd functions carry it and head_desc reads it."""
    return (int(shs_width), bool(use_rgb), bool(xyz_offset), bool(restrict_offset), None if clip_scaling is None else float(clip_scaling))


def check_widths(shs_width, use_rgb, why: str = "") -> None:
    if int(shs_width) not in SHS_WIDTHS:
        raise ValueError(f"shs_width must be one of {SHS_WIDTHS}, got {shs_width}")
    if use_rgb and int(shs_width) != 3:
        raise ValueError(f"use_rgb needs shs_width = 3{why}, got {shs_width}")


def check_pts_and_clip(x, pts, clip_scaling) -> None:
    if pts.shape[0] != x.shape[0] or pts.shape[1] != 3:
        raise ValueError(f"pts: expected ({x.shape[0]}, 3) for x {tuple(x.shape)}, got {tuple(pts.shape)}")
    if clip_scaling is not None and not float(clip_scaling) >= 0:
        raise ValueError(f"clip_scaling must be >= 0 or None, got {clip_scaling}")


def _check(x, pts, weight, bias, shs_width, use_rgb, clip_scaling) -> None:
    """Everything that can be refused on the host is, before any device work."""
    check_f32(x, (("x", x, 2), ("pts", pts, 2), ("weight", weight, 2), ("bias", bias, 1)))
    check_widths(shs_width, use_rgb, " (the reference builds a 3-channel head under use_rgb)")
    O = 11 + int(shs_width)
    if weight.shape[0] != O or bias.shape[0] != O:
        raise ValueError(f"weight / bias: expected {O} rows (11 + shs_width = {shs_width}) for these flags, got {weight.shape[0]} / {bias.shape[0]}")
    if weight.shape[1] != x.shape[1] or x.shape[1] < 1:
        raise ValueError(f"weight is {tuple(weight.shape)}, x has {x.shape[1]} columns")
    check_pts_and_clip(x, pts, clip_scaling)


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
class _TruncExpKeep(torch.autograd.Function):
    """renderer.trunc_exp without its cast to float32 (tgs/utils/ops.py:37-53 in the tensor's own dtype)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


def _activations_keep(raw, pts, use_rgb, xyz_offset, restrict_offset, clip_scaling) -> GaussianModel:
    """renderer.gs_activations statement for statement, in the dtype of its inputs (float64 for the tests' yardstick)."""
    v = raw["xyz"]
    if restrict_offset:
        v = (torch.sigmoid(v) - 0.5) * (1.2 / 32)
    xyz = v + pts if xyz_offset else pts
    scaling = _TruncExpKeep.apply(raw["scaling"])
    if clip_scaling is not None:
        scaling = torch.clamp(scaling, min=0, max=clip_scaling)
    shs = raw["shs"]
    if use_rgb:
        shs = torch.sigmoid(shs)
    shs = torch.reshape(shs, (shs.shape[0], shs.shape[1] // 3, 3))
    return GaussianModel(xyz=xyz, opacity=torch.sigmoid(raw["opacity"]), rotation=F.normalize(raw["rotation"]), scaling=scaling, shs=shs)


def gs_head_ref(x, pts, weight, bias, *, shs_width, use_rgb=False, xyz_offset=True, restrict_offset=False, clip_scaling=None,
                acc: Optional[torch.dtype] = None) -> GaussianModel:
    """The head in plain torch, differentiable: gs_activations over one F.linear. acc=torch.float64 computes (and returns) in double."""
    if acc is not None:
        x, pts, weight, bias = (t.to(acc) for t in (x, pts, weight, bias))
    # (contiguous parts: torch's CPU sigmoid / exp round differently through their strided loops than through their vector loops,
    #  which is what the reference's five separate heads take)
    raw = {k: v.contiguous() for k, v in zip(FIELDS, torch.split(F.linear(x, weight, bias), [3, 3, 4, 1, int(shs_width)], dim=1))}
    if x.dtype == torch.float32:
        return gs_activations(raw, pts, use_rgb=use_rgb, xyz_offset=xyz_offset, restrict_offset=restrict_offset, clip_scaling=clip_scaling)
    return _activations_keep(raw, pts, use_rgb, xyz_offset, restrict_offset, clip_scaling)


_gs_head_ref = gs_head_ref                                          # the name the tests call it by


# ---- device path ---------------------------------------------------------------------------------------------------------------
def head_desc(shs_width, use_rgb, xyz_offset, restrict_offset, clip_scaling) -> _abi.GhHeadDesc:
    """GhHeadDesc of a head_config."""
    flags = (_abi.GH_HEAD_USE_RGB if use_rgb else 0) | (_abi.GH_HEAD_XYZ_OFFSET if xyz_offset else 0) | \
        (_abi.GH_HEAD_RESTRICT_OFFSET if restrict_offset else 0) | (_abi.GH_HEAD_CLIP_SCALING if clip_scaling is not None else 0)
    return _abi.GhHeadDesc(int(shs_width), flags, 0.0 if clip_scaling is None else float(clip_scaling))


def new_outputs(P: int, shs_width: int, device, with_raw: bool):
    """The five outputs in FIELDS order, uninitialised, and `raw` (P, 11 + shs_width) for the backward, or None."""
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
    return (new(P, 3), new(P, 3), new(P, 4), new(P, 1), new(P, shs_width)), (new(P, 11 + shs_width) if with_raw else None)


def pack(xyz, scaling, rotation, opacity, shs) -> GaussianModel:
    """The five outputs in FIELDS order -> GaussianModel, shs (P, shs_width) as (P, shs_width / 3, 3)."""
    return GaussianModel(xyz=xyz, opacity=opacity, rotation=rotation, scaling=scaling, shs=shs.reshape(shs.shape[0], shs.shape[1] // 3, 3))


class _GsHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pts, weight, bias, cfg):
        shs_width = cfg[0]
        ctx.set_materialize_grads(False)
        x, pts, weight, bias = rows(x.detach()), pts.detach().contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
        P, Cin = x.shape
        O, dev = 11 + shs_width, x.device
        outs, raw = new_outputs(P, shs_width, dev, any(ctx.needs_input_grad[:4]))
        if P > 0:
            launch("gh_head_forward", dev, ptr(x), row_stride(x), P, Cin, ptr(pts), ptr(weight), ptr(bias), C.byref(head_desc(*cfg)),
                   *[ptr(o) for o in outs], ptr(raw), what=f"gh_head_forward (P={P}, Cin={Cin}, O={O})")
        ctx.cfg = cfg
        ctx.save_for_backward(x, weight, raw)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xyz, g_scaling, g_rotation, g_opacity, g_shs):
        x, weight, raw = ctx.saved_tensors
        P, Cin = x.shape
        O, dev = weight.shape[0], x.device
        need_pts, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        gx = new(P, Cin)
        gpts = new(P, 3) if need_pts else None
        gw, gb = (new(O, Cin), new(O)) if need_w else (None, None)
        if P == 0:
            if need_w:
                gw.zero_(), gb.zero_()
        else:
            gs = [cotangent(g) for g in (g_xyz, g_scaling, g_rotation, g_opacity, g_shs)]
            nbytes = int(lib().gh_head_workspace_bytes(P, Cin, O)) if need_w else 0
            ws = workspace(nbytes, dev) if need_w else None
            launch("gh_head_backward", dev, ptr(raw), ptr(x), row_stride(x), P, Cin, ptr(weight), C.byref(head_desc(*ctx.cfg)),
                   *[ptr(g) for g in gs], ptr(gx), Cin, ptr(gpts), ptr(gw), ptr(gb), ptr(ws), nbytes,
                   what=f"gh_head_backward (P={P}, Cin={Cin}, O={O})")
        return (gx if ctx.needs_input_grad[0] else None, gpts, gw if ctx.needs_input_grad[2] else None,
                gb if ctx.needs_input_grad[3] else None, None)


def gs_head(x: torch.Tensor, pts: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, shs_width: int, use_rgb: bool = False,
            xyz_offset: bool = True, restrict_offset: bool = False, clip_scaling: Optional[float] = None,
            ops: str = "fused") -> GaussianModel:
    """x (P,Cin), pts (P,3), weight (11 + shs_width, Cin), bias (11 + shs_width), all float32 -> GaussianModel(xyz (P,3), opacity (P,1),
    rotation (P,4), scaling (P,3), shs (P, shs_width / 3, 3)): GSLayer.forward with the five heads concatenated in FIELDS order.
    The keyword defaults are GSLayer.Config's. ops="torch" runs the plain-torch restatement on x's device instead of the kernels;
    CPU tensors always take it."""
    check_ops(ops)
    _check(x, pts, weight, bias, shs_width, use_rgb, clip_scaling)
    cfg = head_config(shs_width, use_rgb, xyz_offset, restrict_offset, clip_scaling)
    if ops == "torch" or not x.is_cuda:
        return gs_head_ref(x, pts, weight, bias, shs_width=cfg[0], use_rgb=cfg[1], xyz_offset=cfg[2], restrict_offset=cfg[3],
                           clip_scaling=cfg[4])
    return pack(*_GsHeadFn.apply(x, pts, weight, bias, cfg))


# ---- the module ------------------------------------------------------------------------------------------------------------------
def gs_layer_forward(self, x: torch.Tensor, pts: torch.Tensor, ops: Optional[str] = None) -> GaussianModel:
    """GSLayer.forward(x, pts) (renderer_one_shot.py:191-214) as one gs_head call. Reads self.cfg.{feature_channels, use_rgb, xyz_offset,
    restrict_offset, clip_scaling} and self.out_layers (one nn.Linear per feature_channels key, in that mapping's order, whatever it
    is); the five parameters are concatenated in FIELDS order."""
    cfg = self.cfg
    keys = list(cfg.feature_channels.keys())
    if sorted(keys) != sorted(FIELDS) or len(self.out_layers) != len(FIELDS):
        raise ValueError(f"feature_channels must name exactly {FIELDS}, got {keys}")
    layers = {k: layer for k, layer in zip(keys, self.out_layers)}
    for k, n in FIXED_WIDTHS.items():
        if layers[k].out_features != n:
            raise ValueError(f"the {k} head must have {n} outputs, got {layers[k].out_features}")
    weight = torch.cat([layers[k].weight for k in FIELDS], dim=0)
    bias = torch.cat([layers[k].bias for k in FIELDS], dim=0)
    clip = getattr(cfg, "clip_scaling", None)
    return gs_head(x, pts, weight, bias, shs_width=layers["shs"].out_features, use_rgb=bool(cfg.use_rgb), xyz_offset=bool(cfg.xyz_offset),
                   restrict_offset=bool(cfg.restrict_offset), clip_scaling=None if clip is None else float(clip),
                   ops=ops or getattr(self, "head_ops", "fused"))


class GSLayer(nn.Module):
    """The reference's GSLayer with its state-dict keys — out_layers.{0..4}.{weight,bias} in feature_channels order — and its
    initialisation (renderer_one_shot.py:170-189): zero weights and biases except the RGB head's (nn.Linear's own), scaling bias
    init_scaling, rotation bias (1,0,0,0), opacity bias logit(init_density). Takes the reference's config mapping
    (`GSLayer({"in_channels": 128, "feature_channels": {...}, "use_rgb": True, ...})`) or keywords."""

    DEFAULTS = dict(in_channels=128, feature_channels=None, xyz_offset=True, restrict_offset=False, use_rgb=False, clip_scaling=None,
                    init_scaling=-5.0, init_density=0.1)
    FEATURE_CHANNELS = dict(xyz=3, scaling=3, rotation=4, opacity=1, shs=48)      # every shipped config's `gs_out.feature_channels`

    def __init__(self, cfg=None, ops: str = "fused", **kw):
        super().__init__()
        given = dict(cfg or {})
        given.update(kw)
        given.pop("weights", None)
        given.pop("freeze", None)
        unknown = set(given) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"GSLayer: unknown config keys {sorted(unknown)}")
        c = {**self.DEFAULTS, **given}
        c["feature_channels"] = dict(c["feature_channels"] or self.FEATURE_CHANNELS)
        self.cfg = SimpleNamespace(**c)
        self.head_ops = ops
        self.out_layers = nn.ModuleList()
        for key, out_ch in self.cfg.feature_channels.items():
            rgb_head = key == "shs" and self.cfg.use_rgb
            layer = nn.Linear(int(self.cfg.in_channels), 3 if rgb_head else int(out_ch))
            if not rgb_head:
                nn.init.constant_(layer.weight, 0)
                nn.init.constant_(layer.bias, 0)
            if key == "scaling":
                nn.init.constant_(layer.bias, float(self.cfg.init_scaling))
            elif key == "rotation":
                nn.init.constant_(layer.bias, 0)
                nn.init.constant_(layer.bias[0], 1.0)
            elif key == "opacity":
                nn.init.constant_(layer.bias, math.log(self.cfg.init_density / (1 - self.cfg.init_density)))
            self.out_layers.append(layer)

    def forward(self, x: torch.Tensor, pts: torch.Tensor) -> GaussianModel:
        return gs_layer_forward(self, x, pts)


_SEAM = (__name__, "fused_gs_layer_cls")


def is_fused_cls(cls) -> bool:
    return _seam.is_grafted(_SEAM, cls)


def fused_gs_layer_cls(base):
    """A subclass of the given GSLayer class (the reference's own, tgs.models.renderer_one_shot.GSLayer) whose forward is
    gs_layer_forward; configure(), the parameters and the config handling stay the base class's."""
    return _seam.graft(_SEAM, base, {"forward": lambda self, x, pts: gs_layer_forward(self, x, pts)}, "fused head")


def fuse_gs_head(renderer):
    """Swap the class of `renderer.gs_net` for fused_gs_layer_cls of its own class: forward_gs then ends in one HIP pass. The module
    object, its parameters and its state dict are untouched. Returns the renderer."""
    net = renderer.gs_net
    if not isinstance(net, GSLayer):
        _seam.swap(_SEAM, net)
    return renderer
