"""The Gaussian trunk: the reference's forward_gs (tgs/models/renderer_one_shot.py:254-257) — the trunk MLP `mlp_net`
(tgs/models/networks.py:57-105: Linear, activation, Linear, activation, Linear) and the Gaussian head `gs_net` behind it — as one HIP
pass forward and one backward, through include/gh_trunk.h.

    gs_trunk(x, pts, trunk, head_weight, head_bias, shs_width=..., use_rgb=..., activation="silu", ...)  -> renderer.GaussianModel

`trunk` is the six tensors (W1 (H,Cin), b1, W2 (H,H), b2, W3 (Cout,H), b3); `head_weight` (O,Cout) and `head_bias` (O) are the five
heads' parameters concatenated as gs_head.gs_head takes them. The kernel path is for frozen weights (the one-shot fit, where the
gradient that matters is the one back to the features): it is differentiable in x and pts, stores nothing of the hidden layers (the
backward recomputes the two hidden pre-activations from x) and refuses a weight that asks for a gradient. x is read in place through
its row stride. Every sum has a fixed order that depends on the sizes alone, and there are no atomics: a row's outputs and its grad_x
are bitwise the same alone or among 100,000 rows.

CPU tensors, and `ops="torch"` on any device, go through `_gs_trunk_ref`: F.linear and F.silu / F.relu three times, then
gs_head.gs_head_ref, in float64 on request (the yardstick of the GPU tests), differentiable with respect to everything.

`TrunkMLP` is the trunk as a module with the reference's state-dict keys (`layers.{0,2,4}.{weight,bias}` for two hidden layers) and
nn.Linear's initialisation. `forward_gs_fused(renderer, x, p)` is forward_gs with the kernel where `kernel_args` finds it applicable
and the reference's two statements everywhere else; `fuse_forward_gs(renderer)` swaps the renderer's class for a subclass whose
forward_gs it is — what the config strings `guassianhand_amd.tgs_renderer.GS3DRenderer...Trunk` do in `configure()`."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam, gs_head
from ._call import check_f32, check_ops, cotangent, launch, ptr, row_stride, rows
from .gs_head import FIELDS, FIXED_WIDTHS, SHS_WIDTHS, check_pts_and_clip, check_widths, gs_head_ref, head_config, head_desc, new_outputs, pack
from .renderer import GaussianModel

ACTIVATIONS = {"silu": _abi.GH_TRUNK_SILU, "relu": _abi.GH_TRUNK_RELU}
WIDTHS = (32, 64, 96, 128)                                      # H and Cout of the kernels (gh_trunk.h)
MAX_CIN = _abi.GH_TRUNK_MAX_CIN


def sizes_supported(Cin: int, H: int, Cout: int, shs_width: int) -> bool:
    return 1 <= Cin <= MAX_CIN and H in WIDTHS and Cout in WIDTHS and shs_width in SHS_WIDTHS


def _check(x, pts, trunk, head_weight, head_bias, shs_width, use_rgb, clip_scaling, activation) -> None:
    """Everything that can be refused on the host is, before any device work."""
    if len(trunk) != 6:
        raise ValueError(f"trunk must be (W1, b1, W2, b2, W3, b3), got {len(trunk)} tensors")
    W1, b1, W2, b2, W3, b3 = trunk
    check_f32(x, (("x", x, 2), ("pts", pts, 2), ("W1", W1, 2), ("b1", b1, 1), ("W2", W2, 2), ("b2", b2, 1), ("W3", W3, 2), ("b3", b3, 1),
                  ("head_weight", head_weight, 2), ("head_bias", head_bias, 1)))
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {tuple(ACTIVATIONS)}, got {activation!r}")
    check_widths(shs_width, use_rgb)
    H, Cout, O = W1.shape[0], W3.shape[0], 11 + int(shs_width)
    if W1.shape[1] != x.shape[1] or x.shape[1] < 1:
        raise ValueError(f"W1 is {tuple(W1.shape)}, x has {x.shape[1]} columns")
    if tuple(W2.shape) != (H, H) or W3.shape[1] != H or b1.shape[0] != H or b2.shape[0] != H or b3.shape[0] != Cout:
        raise ValueError(f"trunk shapes do not chain: W1 {tuple(W1.shape)}, b1 {tuple(b1.shape)}, W2 {tuple(W2.shape)}, b2 {tuple(b2.shape)}, "
                         f"W3 {tuple(W3.shape)}, b3 {tuple(b3.shape)}")
    if tuple(head_weight.shape) != (O, Cout) or head_bias.shape[0] != O:
        raise ValueError(f"head_weight / head_bias: expected ({O}, {Cout}) and ({O},) (11 + shs_width = {shs_width} rows), got "
                         f"{tuple(head_weight.shape)} / {tuple(head_bias.shape)}")
    check_pts_and_clip(x, pts, clip_scaling)


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def _gs_trunk_ref(x, pts, trunk: Sequence[torch.Tensor], head_weight, head_bias, *, shs_width, use_rgb=False, xyz_offset=True,
                  restrict_offset=False, clip_scaling=None, activation="silu", acc: Optional[torch.dtype] = None) -> GaussianModel:
    """forward_gs in plain torch, differentiable: the trunk's three F.linear with the activation between them, then the head's
    restatement. acc=torch.float64 computes (and returns) in double."""
    if acc is not None:
        x, pts, head_weight, head_bias = (t.to(acc) for t in (x, pts, head_weight, head_bias))
        trunk = [t.to(acc) for t in trunk]
    W1, b1, W2, b2, W3, b3 = trunk
    act = F.silu if activation == "silu" else F.relu
    y = F.linear(act(F.linear(act(F.linear(x, W1, b1)), W2, b2)), W3, b3)
    return gs_head_ref(y, pts, head_weight, head_bias, shs_width=shs_width, use_rgb=use_rgb, xyz_offset=xyz_offset,
                       restrict_offset=restrict_offset, clip_scaling=clip_scaling)


# ---- device path ---------------------------------------------------------------------------------------------------------------
class _GsTrunkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pts, cfg, activation, *weights):
        shs_width = cfg[0]
        ctx.set_materialize_grads(False)
        x, pts = rows(x.detach()), pts.detach().contiguous()
        weights = [w.detach().contiguous() for w in weights]
        W1, _, _, _, W3, _, Wh, _ = weights
        P, Cin = x.shape
        H, Cout, O, dev = W1.shape[0], W3.shape[0], 11 + shs_width, x.device
        outs, raw = new_outputs(P, shs_width, dev, any(ctx.needs_input_grad[:2]))
        if P > 0:
            launch("gh_trunk_forward", dev, ptr(x), row_stride(x), P, Cin, H, Cout, ptr(pts), *[ptr(w) for w in weights],
                   C.byref(head_desc(*cfg)), ACTIVATIONS[activation], *[ptr(o) for o in outs], ptr(raw),
                   what=f"gh_trunk_forward (P={P}, Cin={Cin}, H={H}, Cout={Cout}, O={O})")
        ctx.cfg, ctx.activation = cfg, activation
        ctx.save_for_backward(x, raw, *weights)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xyz, g_scaling, g_rotation, g_opacity, g_shs):
        x, raw, W1, b1, W2, b2, W3, _, Wh, _ = ctx.saved_tensors
        P, Cin = x.shape
        H, Cout, dev = W1.shape[0], W3.shape[0], x.device
        gx = torch.empty(P, Cin, dtype=torch.float32, device=dev)
        gpts = torch.empty(P, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if P > 0:
            gs = [cotangent(g) for g in (g_xyz, g_scaling, g_rotation, g_opacity, g_shs)]
            launch("gh_trunk_backward", dev, ptr(raw), ptr(x), row_stride(x), P, Cin, H, Cout, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(W3),
                   ptr(Wh), C.byref(head_desc(*ctx.cfg)), ACTIVATIONS[ctx.activation], *[ptr(g) for g in gs], ptr(gx), Cin, ptr(gpts),
                   what=f"gh_trunk_backward (P={P}, Cin={Cin}, H={H}, Cout={Cout}, O={Wh.shape[0]})")
        return (gx if ctx.needs_input_grad[0] else None, gpts, None, None) + (None,) * 8


def gs_trunk(x: torch.Tensor, pts: torch.Tensor, trunk: Sequence[torch.Tensor], head_weight: torch.Tensor, head_bias: torch.Tensor, *,
             shs_width: int, use_rgb: bool = False, xyz_offset: bool = True, restrict_offset: bool = False,
             clip_scaling: Optional[float] = None, activation: str = "silu", ops: str = "fused") -> GaussianModel:
    """x (P,Cin), pts (P,3), trunk = (W1 (H,Cin), b1, W2 (H,H), b2, W3 (Cout,H), b3), head_weight (11 + shs_width, Cout), head_bias,
    all float32 -> GaussianModel as gs_head.gs_head returns it: forward_gs with a two-hidden-layer trunk. ops="torch" runs the
    plain-torch restatement on x's device instead of the kernels; CPU tensors always take it. The kernels take 1 <= Cin <= 192 and
    H, Cout in {32, 64, 96, 128} and produce no gradient of a weight: a weight that requires one is an error on that path."""
    check_ops(ops)
    trunk = tuple(trunk)
    _check(x, pts, trunk, head_weight, head_bias, shs_width, use_rgb, clip_scaling, activation)
    cfg = head_config(shs_width, use_rgb, xyz_offset, restrict_offset, clip_scaling)
    if ops == "torch" or not x.is_cuda:
        return _gs_trunk_ref(x, pts, trunk, head_weight, head_bias, shs_width=cfg[0], use_rgb=cfg[1], xyz_offset=cfg[2],
                             restrict_offset=cfg[3], clip_scaling=cfg[4], activation=activation)
    Cin, H, Cout = x.shape[1], trunk[0].shape[0], trunk[4].shape[0]
    if not sizes_supported(Cin, H, Cout, cfg[0]):
        raise ValueError(f"the trunk kernels take 1 <= Cin <= {MAX_CIN} and H, Cout in {WIDTHS}, got Cin={Cin}, H={H}, Cout={Cout}")
    if torch.is_grad_enabled() and any(w.requires_grad for w in (*trunk, head_weight, head_bias)):
        raise RuntimeError("the trunk kernels produce no gradient of a weight: freeze the trunk and the head, or use ops='torch'")
    return pack(*_GsTrunkFn.apply(x, pts, cfg, activation, *trunk, head_weight, head_bias))


# ---- the module ------------------------------------------------------------------------------------------------------------------
class TrunkMLP(nn.Module):
    """The reference's MLP (tgs/models/networks.py:57-105) with its state-dict keys — `layers.{0, 2, ...}.{weight,bias}`, the
    activations between them — and nn.Linear's own initialisation, so a reference checkpoint loads unchanged."""

    def __init__(self, dim_in: int, dim_out: int, n_neurons: int, n_hidden_layers: int, activation: str = "relu"):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise NotImplementedError(activation)
        make = (lambda: nn.SiLU(inplace=True)) if activation == "silu" else (lambda: nn.ReLU(inplace=True))
        layers = [nn.Linear(dim_in, n_neurons), make()]
        for _ in range(n_hidden_layers - 1):
            layers += [nn.Linear(n_neurons, n_neurons), make()]
        layers += [nn.Linear(n_neurons, dim_out)]
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x)


# ---- the seam: forward_gs ----------------------------------------------------------------------------------------------------------
def _identity_output(renderer) -> bool:
    conf = renderer.cfg.mlp_network_config
    name = conf.get("output_activation", None) if hasattr(conf, "get") else getattr(conf, "output_activation", None)
    return name is None or str(name).lower() == "none"


_REFERENCE_HEADS = (("tgs.models.renderer_one_shot", "GSLayer"), ("tgs.models.renderer_one_shot_edit", "GSLayer"))


def _forward_is_gslayers(net) -> bool:
    """Whether net(x, p) is GSLayer.forward — the reference's own, gs_head.GSLayer's or the fused head's — which the kernels restate.
    A subclass with a forward of its own keeps it: the kernels would replace it silently."""
    owner = next((c for c in type(net).__mro__ if "forward" in vars(c)), None)
    return owner is gs_head.GSLayer or gs_head.is_fused_cls(owner) or (getattr(owner, "__module__", None), getattr(owner, "__name__", None)) in _REFERENCE_HEADS


def kernel_args(renderer, x, p):
    """(trunk, head_weight, head_bias, keywords) for gs_trunk where forward_gs(x, p) of this renderer can run the kernels, else None:
    `mlp_network_config` set and `mlp_net.layers` exactly Linear, act, Linear, act, Linear with both activations nn.SiLU or both nn.ReLU,
    a bias in every layer, the identity behind them, a `gs_net` that is GSLayer-shaped and whose forward is GSLayer's, sizes the kernels take, float32 tensors on a ROCm
    device outside autocast, and no parameter of either module asking for a gradient (torch.no_grad() qualifies)."""
    cfg = getattr(renderer, "cfg", None)
    if getattr(cfg, "mlp_network_config", None) is None or not _identity_output(renderer):
        return None
    layers = getattr(getattr(renderer, "mlp_net", None), "layers", None)
    if layers is None or len(layers) != 5:
        return None
    l1, a1, l2, a2, l3 = layers
    if not all(isinstance(l, nn.Linear) and l.bias is not None for l in (l1, l2, l3)):
        return None
    if type(a1) is nn.SiLU and type(a2) is nn.SiLU:
        activation = "silu"
    elif type(a1) is nn.ReLU and type(a2) is nn.ReLU:
        activation = "relu"
    else:
        return None
    net = renderer.gs_net
    hcfg, heads = getattr(net, "cfg", None), getattr(net, "out_layers", None)
    keys = list(getattr(hcfg, "feature_channels", {}) or {})
    if heads is None or len(heads) != len(FIELDS) or sorted(keys) != sorted(FIELDS) or not _forward_is_gslayers(net):
        return None
    by_key = dict(zip(keys, heads))
    if not all(isinstance(l, nn.Linear) and l.bias is not None for l in heads) or any(by_key[k].out_features != n for k, n in FIXED_WIDTHS.items()):
        return None
    width, use_rgb = by_key["shs"].out_features, bool(hcfg.use_rgb)
    if not sizes_supported(l1.in_features, l1.out_features, l3.out_features, width) or (use_rgb and width != 3):
        return None
    if (l2.in_features, l2.out_features, l3.in_features) != (l1.out_features,) * 3 or by_key["shs"].in_features != l3.out_features:
        return None
    params = [t for l in (l1, l2, l3, *heads) for t in (l.weight, l.bias)]
    if not (isinstance(x, torch.Tensor) and isinstance(p, torch.Tensor) and x.is_cuda and x.dim() == 2 and p.dim() == 2):
        return None
    if torch.is_autocast_enabled() or any(t.dtype != torch.float32 or t.device != x.device for t in (x, p, *params)):
        return None
    if x.shape[1] != l1.in_features or tuple(p.shape) != (x.shape[0], 3):
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in params):
        return None
    clip = getattr(hcfg, "clip_scaling", None)
    kw = dict(shs_width=width, use_rgb=use_rgb, xyz_offset=bool(hcfg.xyz_offset), restrict_offset=bool(hcfg.restrict_offset),
              clip_scaling=None if clip is None else float(clip), activation=activation)
    trunk = (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    return trunk, torch.cat([by_key[k].weight for k in FIELDS], dim=0), torch.cat([by_key[k].bias for k in FIELDS], dim=0), kw


def forward_gs_fused(renderer, x, p):
    """forward_gs(x, p): one gs_trunk call where kernel_args finds the kernels applicable; in every other case the reference's own
    statements, `mlp_net` in torch and then `gs_net` (the fused head where gs_head.fuse_gs_head was applied), with every gradient."""
    args = kernel_args(renderer, x, p)
    if args is not None:
        trunk, weight, bias, kw = args
        return gs_trunk(x, p, trunk, weight, bias, **kw)
    if renderer.cfg.mlp_network_config is not None:
        x = renderer.mlp_net(x)
    return renderer.gs_net(x, p)


_SEAM = (__name__, "fused_forward_gs_cls")


def fused_forward_gs_cls(base):
    """A subclass of the given renderer class whose forward_gs is forward_gs_fused; everything else stays the base class's."""
    return _seam.graft(_SEAM, base, {"forward_gs": forward_gs_fused}, "fused trunk")


def fuse_forward_gs(renderer):
    """Swap the renderer's class for fused_forward_gs_cls of its own class. Module objects, parameters and the state dict are
    untouched; calling it again changes nothing. Returns the renderer."""
    return _seam.swap(_SEAM, renderer)
