"""The texture scene code: the five statements of TGS._forward between the backbone's tokens and `scene_codes_texture`
(infer_one_shot.py:266-271) as one HIP launch each way through include/gh_scene.h.

    tokens_texture = tokens_texture + tokens_shade
    scene_codes_texture = self.tokenizer_texture.detokenize(tokens_texture)          (B, Ci, Np S^2) -> (B, Np, Ci, S, S)
    scene_codes_texture = self.post_processor_texture(scene_codes_texture)           ConvTranspose2d(Ci, Co, 2, stride 2) per plane
    scene_codes_texture = torch.cat([scene_codes_texture[:,0], scene_codes_texture[:,1]], dim=-1).unsqueeze(1)
    scene_codes_texture = scene_codes_texture + torch.cat([self.map_bias[...,:64], self.map_bias[...,:64]], dim=-1)

    scene_code(upsample, tokens, plane_bias=None, *, ops="fused")    -> (B, 1, Co, 2S, Np 2S)

`tokens` is one (B, Ci, Np S^2) tensor or a pair of them (their sum is formed inside the kernel); `upsample` is the reference's
TriplaneUpsampleNetwork (tgs/models/networks_texture.py:30-54) or the standalone class below, read through `.upsample.weight`,
`.upsample.bias` and `.cfg.n_plane`; `plane_bias` is a (Co, 2S, Wb >= 2S) parameter whose first 2S columns are added to every plane
(`map_bias`, (80, 64, 128), read in place). A kernel-2 stride-2 transposed convolution has no overlap, so every output texel is one
dot product over Ci: the forward is one 4Co x Ci x T product per batch element whose epilogue writes the joined layout with both
biases added, and the backward is its transpose plus an ordered sum for the bias. The call is one autograd.Function, differentiable
in the tokens (one gradient tensor serves both of a pair) and in `plane_bias` (the gradient has the parameter's shape, zeros beyond
column 2S). A backward that needs only the bias's gradient runs no product at all: the fit that trains `map_bias` alone.
Tokens and `plane_bias` are read in place through their strides; only a tensor whose last stride is not 1 is copied, once.

`scene_code_ref` holds the statements in plain torch (view / permute / cat, float64 on request). It is the CPU path, the yardstick
of the tests and the fallback: the kernels are taken for float32 ROCm tensors when the convolution has kernel 2, stride 2, no
padding, no output padding, dilation 1 and groups 1, the sizes are within include/gh_scene.h's limits and neither parameter of
`upsample` requires a gradient (the fit freezes them). Everything else runs `scene_code_ref`, which differentiates with respect to
everything; nothing raises where the reference's statements worked.

`TriplaneUpsampleNetwork(in_channels, out_channels, n_plane)` is the module itself, with the reference's state-dict keys
(`upsample.weight`, `upsample.bias`) and nn.ConvTranspose2d's default initialisation; its forward (B, Np, Ci, S, S) ->
(B, Np, Co, 2S, 2S) is the kernel's per-plane form and reads detokenize's view in place. `fused_upsample_cls(base)` grafts that
forward onto the reference's own class (guassianhand_amd.tgs_scene.TriplaneUpsampleNetwork)."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam
from ._call import check_ops, cotangent, launch, ptr

MAX_CI, MAX_CO = _abi.GH_SCENE_MAX_CI, _abi.GH_SCENE_MAX_CO
Tokens = Union[torch.Tensor, Sequence[torch.Tensor]]


def _pair(tokens: Tokens) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    if isinstance(tokens, torch.Tensor):
        return tokens, None
    if len(tokens) == 1:
        return tokens[0], None
    if len(tokens) != 2:
        raise ValueError(f"tokens: expected one tensor or a pair, got {len(tokens)}")
    return tokens[0], tokens[1]


def _plane_size(T: int, Np: int) -> int:
    S = math.isqrt(T // Np) if Np > 0 else 0
    if Np < 1 or Np * S * S != T:
        raise ValueError(f"tokens: {T} tokens are not {Np} square planes")
    return S


# ---- plain-torch restatement (CPU path, fallback, yardstick) ----------------------------------------------------------------------------
def _conv(conv, x: torch.Tensor, acc: Optional[torch.dtype]) -> torch.Tensor:
    """conv (an nn.ConvTranspose2d) applied to x, in `acc` when given."""
    w, b = conv.weight, conv.bias
    if acc is not None:
        x, w, b = x.to(acc), w.to(acc), None if b is None else b.to(acc)
    return F.conv_transpose2d(x, w, b, conv.stride, conv.padding, conv.output_padding, conv.groups, conv.dilation)


def upsample_ref(upsample, triplanes: torch.Tensor, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """TriplaneUpsampleNetwork.forward's statements: (B, Np, Ci, Hp, Wp) -> (B, Np, Co, Hp2, Wp2)."""
    B, Np = triplanes.shape[:2]
    y = _conv(upsample.upsample, triplanes.reshape(B * Np, *triplanes.shape[2:]), acc)
    return y.view(B, Np, *y.shape[1:])


def scene_code_ref(upsample, tokens: Tokens, plane_bias: Optional[torch.Tensor] = None, *, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """The five statements in plain torch, for any number of planes: differentiable with respect to everything.
    acc=torch.float64 computes (and returns) in double."""
    a, b = _pair(tokens)
    if acc is not None:
        a, b = a.to(acc), None if b is None else b.to(acc)
    x = a if b is None else a + b
    Np = int(upsample.cfg.n_plane)
    B, Ci, T = x.shape
    S = _plane_size(T, Np)
    planes = x.view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4)                                   # detokenize
    y = upsample_ref(upsample, planes, acc)                                                   # (B, Np, Co, 2S, 2S)
    y = torch.cat([y[:, p] for p in range(Np)], dim=-1).unsqueeze(1)
    if plane_bias is not None:
        pb = plane_bias if acc is None else plane_bias.to(acc)
        w = y.shape[-1] // Np
        y = y + torch.cat([pb[..., :w]] * Np, dim=-1)
    return y


# ---- device path ---------------------------------------------------------------------------------------------------------------------
def _unit_last(t: torch.Tensor) -> torch.Tensor:
    """The tensor as the kernels read it: unit last stride, anything in the other dimensions; otherwise one copy."""
    t = t.detach()
    return t if t.shape[-1] == 1 or t.stride(-1) == 1 else t.contiguous()


def _dims(B, Ci, Co, Np, S, per_plane) -> _abi.GhSceneDims:
    return _abi.GhSceneDims(B, Ci, Co, Np, S, _abi.GH_SCENE_PER_PLANE if per_plane else 0)


class _SceneCodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok_a, tok_b, plane_bias, weight, bias, Np, per_plane):
        a = _unit_last(tok_a)
        b = None if tok_b is None else _unit_last(tok_b)
        pb = None if plane_bias is None else _unit_last(plane_bias)
        w = weight.detach().contiguous()
        cb = None if bias is None else bias.detach().contiguous()
        B, Ci, T = a.shape
        Co, S, dev = w.shape[1], _plane_size(T, Np), a.device
        shape = (B, Np, Co, 2 * S, 2 * S) if per_plane else (B, 1, Co, 2 * S, Np * 2 * S)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        if B > 0:
            dims = _dims(B, Ci, Co, Np, S, per_plane)
            launch("gh_scene_code_forward", dev, C.byref(dims), ptr(a), a.stride(0), a.stride(1), ptr(b),
                   0 if b is None else b.stride(0), 0 if b is None else b.stride(1), ptr(w), ptr(cb), ptr(pb),
                   0 if pb is None else pb.stride(0), 0 if pb is None else pb.stride(1), ptr(out),
                   what=f"gh_scene_code_forward (B={B}, Ci={Ci}, Co={Co}, Np={Np}, S={S})")
        ctx.save_for_backward(w)
        ctx.geom = (B, Ci, Co, Np, S, per_plane)
        ctx.pb_shape = None if plane_bias is None else tuple(plane_bias.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        (w,) = ctx.saved_tensors
        B, Ci, Co, Np, S, per_plane = ctx.geom
        dev = w.device
        need_a, need_b, need_pb = ctx.needs_input_grad[:3]
        need_pb = need_pb and ctx.pb_shape is not None
        d_tok = torch.empty(B, Ci, Np * S * S, dtype=torch.float32, device=dev) if (need_a or need_b) else None
        d_pb = torch.zeros(ctx.pb_shape, dtype=torch.float32, device=dev) if need_pb else None
        if B > 0 and (d_tok is not None or d_pb is not None):
            g = cotangent(g_out)
            dims = _dims(B, Ci, Co, Np, S, per_plane)
            launch("gh_scene_code_backward", dev, C.byref(dims), ptr(w), ptr(g), ptr(d_tok), ptr(d_pb),
                   0 if d_pb is None else d_pb.stride(0), 0 if d_pb is None else d_pb.stride(1),
                   what=f"gh_scene_code_backward (B={B}, Ci={Ci}, Co={Co}, Np={Np}, S={S})")
        return (d_tok if need_a else None), (d_tok if need_b else None), d_pb, None, None, None, None


def _is_2x2_stride_2(conv) -> bool:
    two = lambda v: tuple(v) == (2, 2)
    zero = lambda v: tuple(v) == (0, 0)
    return (isinstance(conv, nn.ConvTranspose2d) and two(conv.kernel_size) and two(conv.stride) and zero(conv.padding)
            and zero(conv.output_padding) and tuple(conv.dilation) == (1, 1) and conv.groups == 1)


def _kernel_applies(upsample, tensors) -> bool:
    """The conditions of the module docstring, on the convolution and on every tensor the kernels would read."""
    conv = upsample.upsample
    if not _is_2x2_stride_2(conv):
        return False
    params = [conv.weight] + ([] if conv.bias is None else [conv.bias])
    if any(p.requires_grad for p in params):
        return False
    if not (1 <= conv.in_channels <= MAX_CI and 1 <= conv.out_channels <= MAX_CO):
        return False
    dev = tensors[0].device
    return all(t.is_cuda and t.device == dev and t.dtype == torch.float32 for t in list(tensors) + params)


def _tiles_fit(B: int, T: int, Ci: int, Co: int) -> bool:
    tiles = max(B, 1) * ((T + 31) // 32) * max((4 * Co + 31) // 32, (Ci + 31) // 32)
    return tiles <= _abi.GH_SCENE_MAX_TILES and Co * T <= 64 * _abi.GH_SCENE_MAX_TILES


def scene_code(upsample, tokens: Tokens, plane_bias: Optional[torch.Tensor] = None, *, ops: str = "fused") -> torch.Tensor:
    """tokens (B, Ci, Np S^2), one tensor or a pair -> (B, 1, Co, 2S, Np 2S): the sum of the pair, upsampled per plane by
    `upsample.upsample`, the planes side by side, plus the first 2S columns of `plane_bias` (Co, 2S, Wb >= 2S) on every plane.
    Differentiable in the tokens and in `plane_bias`. ops="torch" runs scene_code_ref on the tensors' device; so does everything
    outside the kernels' conditions (module docstring)."""
    check_ops(ops)
    a, b = _pair(tokens)
    for name, t in (("tokens", a), ("tokens[1]", b)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 3):
            raise ValueError(f"{name}: expected a (B, Ci, T) tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    tensors = [t for t in (a, b, plane_bias) if t is not None]
    fused = ops == "fused" and _kernel_applies(upsample, tensors) and (b is None or b.shape == a.shape)
    if fused:
        conv, Np = upsample.upsample, int(upsample.cfg.n_plane)
        B, Ci, T = a.shape
        fused = Ci == conv.in_channels and Np >= 1 and T >= Np and T % Np == 0 and math.isqrt(T // Np) ** 2 == T // Np
        if fused:
            S = math.isqrt(T // Np)
            fused = _tiles_fit(B, T, Ci, conv.out_channels) and (
                plane_bias is None or (plane_bias.dim() == 3 and plane_bias.shape[0] == conv.out_channels and plane_bias.shape[1] == 2 * S
                                       and plane_bias.shape[2] >= 2 * S))
    if not fused:
        return scene_code_ref(upsample, tokens, plane_bias)
    return _SceneCodeFn.apply(a, b, plane_bias, conv.weight, conv.bias, Np, False)


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _tokens_view(triplanes: torch.Tensor) -> torch.Tensor:
    """(B, Np, Ci, S, S) as the (B, Ci, Np S^2) token tensor it was detokenized from: reshape gives a view when the planes lie that
    way in memory (detokenize's own result does: strides S^2, S, 1 over plane, row and column), and one copy otherwise."""
    B, Np, Ci, S, _ = triplanes.shape
    return triplanes.permute(0, 2, 1, 3, 4).reshape(B, Ci, Np * S * S)


def upsample_forward(self, triplanes: torch.Tensor, ops: str = "fused") -> Optional[torch.Tensor]:
    """TriplaneUpsampleNetwork.forward through the kernel's per-plane form, or None where the kernels do not apply."""
    if ops != "fused" or triplanes.dim() != 5 or triplanes.shape[3] != triplanes.shape[4] or not _kernel_applies(self, [triplanes]):
        return None
    B, Np, Ci, S, _ = triplanes.shape
    conv = self.upsample
    if Np != int(self.cfg.n_plane) or Ci != conv.in_channels or S < 1 or not _tiles_fit(B, Np * S * S, Ci, conv.out_channels):
        return None
    return _SceneCodeFn.apply(_tokens_view(triplanes), None, None, conv.weight, conv.bias, Np, True)


class TriplaneUpsampleNetwork(nn.Module):
    """The reference's TriplaneUpsampleNetwork (networks_texture.py:30-54) as a plain nn.Module: the same state-dict keys, the same
    default initialisation, `cfg.in_channels`, `cfg.out_channels`, `cfg.n_plane`."""

    def __init__(self, in_channels: int = 1024, out_channels: int = 80, n_plane: int = 1):
        super().__init__()
        self.cfg = SimpleNamespace(in_channels=in_channels, out_channels=out_channels, n_plane=n_plane)
        self.upsample = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=2, stride=2)

    def forward(self, triplanes: torch.Tensor) -> torch.Tensor:
        out = upsample_forward(self, triplanes)
        return upsample_ref(self, triplanes) if out is None else out


def fused_upsample_cls(base):
    """A subclass of the given class (the reference's own tgs.models.networks_texture.TriplaneUpsampleNetwork) whose forward runs
    the kernel's per-plane form where it applies and the base class's forward, unchanged, everywhere else."""
    def forward(self, triplanes):
        out = upsample_forward(self, triplanes)
        return base.forward(self, triplanes) if out is None else out

    return _seam.graft((__name__, "fused_upsample_cls"), base, {"forward": forward}, "upsample kernel")
