"""The fit's perceptual term: the reference's VGGLoss (utils.py:910-930) over its Vgg19 slices (utils.py:875-908) with the
convolutions, the pooling and the feature distances in HIP through include/gh_conv.h (and gh_l1_loss of gh_raster.h).

    conv3x3(x, weight, bias, relu=False, ops="fused", *, packed=None)     (N, H, W, Cin) -> (N, H, W, Cout), padding 1, stride 1
    max_pool2x2(x, ops="fused")                                            (N, H, W, C)   -> (N, H/2, W/2, C), kernel 2, stride 2, floor
    VGG19Features(widths=(64, 128, 256, 512))                              torchvision vgg19 `features` up to relu4_1, frozen
    PerceptualLoss(features, ops="fused")(x, y=None, *, ops=None)          (B, 3, H, W) images in [0, 1] -> the scalar loss
    perceptual_loss(features, x, y, *, ops="fused")                        the two-argument form
    perceptual_loss_ref(features, x, y, acc=None)                          the statements in plain torch (float64 on request)

Feature maps are channels-last (N, H, W, C) float32: the pixel is the column of the kernels' matrix products, and a pixel's channels
are the contiguous run a lane reads. `weight` is torch's (Cout, Cin, 3, 3); the kernels read two layouts prepared from it once
(`pack_weights`: tap-major for the forward, flipped and transposed for the backward-data product), which VGG19Features caches
per convolution. Both functions are autograd.Functions differentiable in `x` alone: the weights are frozen, as in the reference
(utils.py:897-899), so a backward holds no activation — a convolution keeps one bit per output (was the pre-activation > 0), a pooling
one byte per pooled element (which of the four won). The feature distances keep their own gradient sign(f - t) / n.

The fused path is taken for float32 ROCm tensors whose `weight` and `bias` do not require a gradient, with 1 <= Cin, Cout <= 512.
Everything else — a CPU tensor, another dtype, a weight that trains — runs the plain-torch statements (F.conv2d / F.max_pool2d on the
permuted tensor), which differentiate with respect to everything; nothing raises where torch would have worked. ops="torch" runs those
statements on the tensor's own device (MIOpen on a ROCm device): the A/B switch of tools/perceptual_time.py.

Weights. VGG19Features' own state-dict keys are the reference checkpoint's without its prefix, `slice{k}.{N}.weight` / `.bias` with N
the torchvision `features` index (0, 2, 5, 7, 10, 12, 14, 16, 19). load_state_dict also accepts torchvision's `features.N.*` and the
reference's `vgg_loss.vgg_net.slice{k}.N.*` (its VGGLoss is a submodule of the Lightning module, so `pretrain_model.ckpt` carries
them); other keys of such a checkpoint are ignored."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi
from ._call import check_ops, cotangent, launch, on_device, pad_to, ptr

MAX_C = _abi.GH_CONV_MAX_C
# (slice, torchvision features index, input width, output width) with widths as indices into (3,) + widths
CONVS = ((1, 0, 0, 1), (2, 2, 1, 1), (2, 5, 1, 2), (3, 7, 2, 2), (3, 10, 2, 3), (4, 12, 3, 3), (4, 14, 3, 3), (4, 16, 3, 3), (4, 19, 3, 4))
POOL_BEFORE = (5, 10, 19)          # the pools at features 4, 9 and 18 precede these convolutions
TAPS = (0, 5, 10, 19)              # relu1_1, relu2_1, relu3_1, relu4_1 follow these convolutions
TAP_WEIGHTS = (1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def pack_weights(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wf, wb) of include/gh_conv.h from a (Cout, Cin, 3, 3) weight: wf (9, pad(Cout), Cin) tap-major, wb (9, pad(Cin), Cout) the
    flipped, transposed layout of the backward-data product; the padding rows are zeros."""
    w = weight.detach().float()
    Cout, Cin = w.shape[:2]
    wf = w.new_zeros(9, pad_to(Cout, _abi.GH_CONV_CHUNK), Cin)
    wf[:, :Cout] = w.permute(2, 3, 0, 1).reshape(9, Cout, Cin)
    wb = w.new_zeros(9, pad_to(Cin, _abi.GH_CONV_CHUNK), Cout)
    wb[:, :Cin] = w.flip(2, 3).permute(2, 3, 1, 0).reshape(9, Cin, Cout)
    return wf, wb


# ---- plain-torch restatements (CPU path, fallback, yardstick) -----------------------------------------------------------------------------
def conv3x3_ref(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = False,
                acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """F.conv2d(padding=1) on the permuted tensor, in `acc` when given; (N, H, W, Cin) -> (N, H, W, Cout)."""
    if acc is not None:
        x, weight, bias = x.to(acc), weight.to(acc), None if bias is None else bias.to(acc)
    y = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, padding=1).permute(0, 2, 3, 1)
    return torch.relu(y) if relu else y


def max_pool2x2_ref(x: torch.Tensor) -> torch.Tensor:
    return F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


# ---- device path -----------------------------------------------------------------------------------------------------------------------
def _conv_forward(x, wf, bias, Cout: int, relu: bool, chunk: int = 0):
    """(y, gate) of gh_conv3x3_forward for a contiguous (N, H, W, Cin) x; gate is None without a ReLU."""
    N, H, W, Cin = x.shape
    y = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x.device)
    gate = torch.empty(N * H * W * ((Cout + 31) // 32), dtype=torch.int32, device=x.device) if relu else None
    launch("gh_conv3x3_forward", x.device, ptr(x), N, H, W, Cin, Cout, ptr(wf), ptr(bias), _abi.GH_CONV_RELU if relu else 0, chunk,
           ptr(y), ptr(gate), what=f"gh_conv3x3_forward (N={N}, H={H}, W={W}, Cin={Cin}, Cout={Cout})")
    return y, gate


def _conv_backward(g, gate, wb, Cin: int, relu: bool, chunk: int = 0):
    """dx of gh_conv3x3_backward_data for a contiguous (N, H, W, Cout) cotangent."""
    N, H, W, Cout = g.shape
    dx = torch.empty(N, H, W, Cin, dtype=torch.float32, device=g.device)
    launch("gh_conv3x3_backward_data", g.device, ptr(g), ptr(gate), N, H, W, Cin, Cout, ptr(wb), _abi.GH_CONV_RELU if relu else 0,
           chunk, ptr(dx), what=f"gh_conv3x3_backward_data (N={N}, H={H}, W={W}, Cin={Cin}, Cout={Cout})")
    return dx


class _Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wf, wb, bias, Cout, relu, chunk):
        xc = x.detach().contiguous()
        y, gate = _conv_forward(xc, wf, bias, Cout, relu, chunk)
        ctx.save_for_backward(wb, gate)
        ctx.geom = (xc.shape[3], relu, chunk)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        wb, gate = ctx.saved_tensors
        Cin, relu, chunk = ctx.geom
        return _conv_backward(cotangent(gy), gate, wb, Cin, relu, chunk), None, None, None, None, None, None


def _pool_forward(x):
    """(y, choice) of gh_maxpool2x2_forward for a contiguous (N, H, W, C) x."""
    N, H, W, Cn = x.shape
    y = torch.empty(N, H // 2, W // 2, Cn, dtype=torch.float32, device=x.device)
    choice = torch.empty(N, H // 2, W // 2, Cn, dtype=torch.uint8, device=x.device)
    launch("gh_maxpool2x2_forward", x.device, ptr(x), N, H, W, Cn, ptr(y), ptr(choice), what=f"gh_maxpool2x2_forward ({N}, {H}, {W}, {Cn})")
    return y, choice


def _pool_backward(g, choice, H: int, W: int):
    N, _, _, Cn = choice.shape
    dx = torch.empty(N, H, W, Cn, dtype=torch.float32, device=choice.device)
    launch("gh_maxpool2x2_backward", choice.device, ptr(g), ptr(choice), N, H, W, Cn, ptr(dx), what=f"gh_maxpool2x2_backward ({N}, {H}, {W}, {Cn})")
    return dx


class _MaxPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xc = x.detach().contiguous()
        y, choice = _pool_forward(xc)
        ctx.save_for_backward(choice)
        ctx.hw = (xc.shape[1], xc.shape[2])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (choice,) = ctx.saved_tensors
        return _pool_backward(cotangent(gy), choice, *ctx.hw)


def _conv_applies(x, weight, bias) -> bool:
    """The conditions of the module docstring on every tensor the kernels would read."""
    if not on_device(x) or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.shape[3] != weight.shape[1]:
        return False
    params = [weight] + ([] if bias is None else [bias])
    if any(p.requires_grad or p.dtype != torch.float32 or p.device != x.device for p in params):
        return False
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        return False
    return 1 <= weight.shape[0] <= MAX_C and 1 <= weight.shape[1] <= MAX_C


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False, ops: str = "fused", *,
            packed: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, chunk: int = 0) -> torch.Tensor:
    """x (N, H, W, Cin) -> (N, H, W, Cout): the 3x3 convolution with zero padding 1 and stride 1 of `weight` (Cout, Cin, 3, 3) and
    `bias`, then a ReLU on request. Differentiable in x. `packed` is pack_weights(weight) where the caller keeps it (a module does);
    `chunk` (0, 32, 64, 128) fixes the kernels' chunk of output channels, which no result depends on. ops="torch" and everything
    outside the kernels' conditions (module docstring) run conv3x3_ref."""
    check_ops(ops)
    if ops != "fused" or not _conv_applies(x, weight, bias):
        return conv3x3_ref(x, weight, bias, relu)
    wf, wb = pack_weights(weight) if packed is None else packed
    b = None if bias is None else bias.detach().contiguous()
    return _Conv3x3Fn.apply(x, wf, wb, b, int(weight.shape[0]), bool(relu), int(chunk))


def max_pool2x2(x: torch.Tensor, ops: str = "fused") -> torch.Tensor:
    """x (N, H, W, C) -> (N, H/2, W/2, C): F.max_pool2d(kernel 2, stride 2) channels-last. Differentiable in x."""
    check_ops(ops)
    if ops != "fused" or not on_device(x) or x.shape[3] < 1:
        return max_pool2x2_ref(x)
    return _MaxPool2x2Fn.apply(x)


def feature_distance(f: torch.Tensor, t: torch.Tensor, *, ops: str = "fused") -> torch.Tensor:
    """mean|f - t|, differentiable in f (sign(f - t) / n, sign(0) = 0): gh_l1_loss where the kernels apply."""
    check_ops(ops)
    if ops == "fused" and on_device(f) and on_device(t) and f.shape == t.shape and f.numel() > 0 and not t.requires_grad:
        from .loss import l1_mean_loss
        return l1_mean_loss(f, t)
    return (f - t).abs().mean()


# ---- the network -------------------------------------------------------------------------------------------------------------------------
class VGG19Features(nn.Module):
    """The reference's Vgg19 (utils.py:875-908): torchvision vgg19 `features` 0 .. 20 in four slices, returning relu1_1, relu2_1,
    relu3_1 and relu4_1. Feature maps are channels-last here: forward takes (N, H, W, 3) and returns four (N, h, w, c) tensors.
    The parameters are frozen. `widths` are the four channel counts (the tests run a network of a few channels)."""

    def __init__(self, widths: Sequence[int] = (64, 128, 256, 512)):
        super().__init__()
        if len(widths) != 4 or any(int(w) < 1 for w in widths):
            raise ValueError(f"widths: expected four positive channel counts, got {widths!r}")
        self.widths = tuple(int(w) for w in widths)
        ch = (3,) + self.widths
        for k in (1, 2, 3, 4):
            setattr(self, f"slice{k}", nn.ModuleDict({str(n): nn.Conv2d(ch[i], ch[o], 3, padding=1) for s, n, i, o in CONVS if s == k}))
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed = {}

    def conv(self, n: int) -> nn.Conv2d:
        s = next(s for s, m, _, _ in CONVS if m == n)
        return getattr(self, f"slice{s}")[str(n)]

    def _packed_for(self, n: int, conv: nn.Conv2d):
        w = conv.weight
        key = (w.data_ptr(), w._version, w.device)
        hit = self._packed.get(n)
        if hit is None or hit[0] != key:
            hit = (key, pack_weights(w))
            self._packed[n] = hit
        return hit[1]

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts this module's own keys, torchvision's `features.N.*` and the reference checkpoint's
        `vgg_loss.vgg_net.slice{k}.N.*`; the other keys of such a state dict are ignored."""
        own = {}
        slice_of = {n: s for s, n, _, _ in CONVS}
        for k, v in state_dict.items():
            parts = k.split(".")
            if k.startswith("vgg_loss.vgg_net.slice"):
                own[".".join(parts[2:])] = v
            elif parts[0] == "features" and len(parts) == 3 and parts[1].isdigit():
                if int(parts[1]) in slice_of:
                    own[f"slice{slice_of[int(parts[1])]}.{parts[1]}.{parts[2]}"] = v
            elif parts[0].startswith("slice"):
                own[k] = v
        self._packed = {}
        return super().load_state_dict(own, strict=strict, **kw)

    def forward(self, x: torch.Tensor, *, ops: str = "fused") -> List[torch.Tensor]:
        check_ops(ops)
        taps, h = [], x
        for _, n, _, _ in CONVS:
            if n in POOL_BEFORE:
                h = max_pool2x2(h, ops=ops)
            conv = self.conv(n)
            fused = ops == "fused" and _conv_applies(h, conv.weight, conv.bias)
            h = conv3x3(h, conv.weight, conv.bias, relu=True, ops=ops, packed=self._packed_for(n, conv) if fused else None)
            if n in TAPS:
                taps.append(h)
        return taps


def _normalised(x: torch.Tensor, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """torchvision's Normalize with the ImageNet statistics on (B, 3, H, W), as (B, H, W, 3) contiguous."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected (B, 3, H, W) images, got {tuple(x.shape)}")
    if acc is not None:
        x = x.to(acc)
    mean = torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return ((x - mean) / std).permute(0, 2, 3, 1).contiguous()


class PerceptualLoss(nn.Module):
    """The reference's VGGLoss.forward (utils.py:924-930): both images normalised, the four feature maps compared by L1Loss means
    weighted 1/16, 1/8, 1/4 and 1, the target branch detached. set_target(y) computes the target's feature maps once (a fit's target
    never changes); forward(x) then compares against them, forward(x, y) recomputes them."""

    def __init__(self, features: VGG19Features, ops: str = "fused"):
        super().__init__()
        check_ops(ops)
        self.features, self.ops = features, ops           # ops: the module's default, for a caller that cannot pass one (the fit)
        self._target: Optional[List[torch.Tensor]] = None

    @torch.no_grad()
    def target_features(self, y: torch.Tensor, *, ops: Optional[str] = None) -> List[torch.Tensor]:
        return [t.detach() for t in self.features(_normalised(y.detach()), ops=self.ops if ops is None else ops)]

    def set_target(self, y: torch.Tensor, *, ops: Optional[str] = None) -> None:
        self._target = self.target_features(y, ops=ops)

    def forward(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, *, ops: Optional[str] = None,
                target_features: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        ops = self.ops if ops is None else ops
        check_ops(ops)
        tf = target_features if target_features is not None else (self.target_features(y, ops=ops) if y is not None else self._target)
        if tf is None:
            raise ValueError("PerceptualLoss: no target (pass y or call set_target first)")
        fx = self.features(_normalised(x), ops=ops)
        loss = None
        for w, f, t in zip(TAP_WEIGHTS, fx, tf):
            term = w * feature_distance(f, t, ops=ops)
            loss = term if loss is None else loss + term
        return loss


def perceptual_loss(features: VGG19Features, x: torch.Tensor, y: torch.Tensor, *, ops: str = "fused") -> torch.Tensor:
    """VGGLoss.forward(x, y) over `features`: the two-argument form, which computes the target's feature maps on every call."""
    return PerceptualLoss(features)(x, y, ops=ops)


def perceptual_loss_ref(features: VGG19Features, x: torch.Tensor, y: torch.Tensor, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """VGGLoss.forward(x, y) in plain torch ops (channels-first as the reference runs it), in `acc` when given: the CPU path and the
    tests' yardstick. Differentiable in x."""
    def net(img):
        h = _normalised(img, acc).permute(0, 3, 1, 2)
        taps = []
        for _, n, _, _ in CONVS:
            if n in POOL_BEFORE:
                h = F.max_pool2d(h, 2)
            conv = features.conv(n)
            w, b = conv.weight, conv.bias
            if acc is not None:
                w, b = w.to(acc), b.to(acc)
            h = torch.relu(F.conv2d(h, w, b, padding=1))
            if n in TAPS:
                taps.append(h)
        return taps

    fx, fy = net(x), net(y)
    loss = 0
    for w, f, t in zip(TAP_WEIGHTS, fx, fy):
        loss = loss + w * (f - t.detach()).abs().mean()
    return loss
