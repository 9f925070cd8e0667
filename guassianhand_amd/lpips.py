"""The evaluator's perceptual score: LPIPS over AlexNet — `lpips.LPIPS(net='alex')`, version 0.1, eval mode, spatial=False — as the
reference's test step reports it (infer_one_shot.py:527-555 calling evaluator.py:26-65), with the convolutions, the pooling, LPIPS'
head and the crop-quantise-scale prologue in HIP through include/gh_lpips.h. Forward only: the reference never differentiates it.

The `lpips` package is no dependency of this project and its weights are not shipped: the result is specified by its mathematics,
unpinned against the package (include/gh_lpips.h states it), and a user who has the package loads its weights with one line.

    AlexLPIPS(widths=(64, 192, 384, 256, 256))                     the frozen network: five convolutions, five `lin` weights, shift / scale
    AlexLPIPS.synthetic(seed, widths)                              random weights with non-negative `lin` (tests, timing)
    lpips_distance(net, x0, x1, *, ops="fused", terms=False)       (N, 3, H, W) in [-1, 1] -> (N,) float64 (and the (5, N) per-tap terms)
    lpips_ref(net, x0, x1, acc=None, terms=False)                  the statements in plain torch (float64 on request): the yardstick
    lpips_scores(net, pred, gt, mask_at_box=None, *, bbox_mask=None, layout="chw", quantize=True, ops="fused")
                                                                    the evaluator's protocol for Nv views in [0, 1] -> (Nv,) float64
    conv2d, max_pool3x3s2, lpips_layer, prepare_input              the single kernels, channels-last (the unit tests' entry points)

The evaluator's protocol, per view: both images are cropped to cv2.boundingRect(mask_at_box) (the whole image without a mask), the
prediction is taken as 0 where bbox_mask == 0 (where one is given), both are written as 8-bit images and read back (quantize=True:
q = min(max(rint(v * 255), 0), 255) in float32, to nearest, ties to even), mapped by im2tensor, x = float32(double(q) / 127.5 - 1), and
scored. A NaN stays a NaN and makes that view's score NaN; OpenCV's conversion of a NaN to 8 bits is not emulated. A crop under 31
pixels in either direction (AlexNet's smallest input) scores NaN.

The fused path is taken for float32 ROCm tensors with ops="fused". ops="torch" runs F.conv2d / F.max_pool2d on the tensor's own
device (MIOpen on a ROCm device): the A/B switch of tools/lpips_time.py. CPU tensors and other dtypes run the torch statements too.
A kernel that is missing is an error, never a fall-back. The network must live on the images' device (ValueError otherwise; a network
of another dtype runs the torch statements), and every entry point checks the device and dtype of each tensor a kernel would read
on the host, before its first launch."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from ._call import check_ops, launch, lib, on_device, pad_to, ptr, workspace

MIN_SIZE = _abi.GH_LPIPS_MIN_SIZE
MAX_C = _abi.GH_LPIPS_MAX_C
WIDTHS = (64, 192, 384, 256, 256)
# (torchvision features index, kernel, stride, padding, a 3x3 stride-2 pooling precedes it) of the five convolutions
CONVS = ((0, 11, 4, 2, False), (3, 5, 1, 2, True), (6, 3, 1, 1, True), (8, 3, 1, 1, False), (10, 3, 1, 1, False))
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


def pack_conv(weight: torch.Tensor) -> torch.Tensor:
    """wp of include/gh_lpips.h from a (Cout, Cin, K, K) weight: (pad(Cout), Rp) with wp[co][(K ky + kx) Cin + ci] = W[co][ci][ky][kx],
    R = K K Cin rounded up to a multiple of 4; the padding rows and columns are zeros."""
    w = weight.detach().float()
    Cout, Cin, K, _ = w.shape
    R = K * K * Cin
    wp = w.new_zeros(pad_to(Cout, _abi.GH_LPIPS_CHUNK), -(-R // 4) * 4)
    wp[:Cout, :R] = w.permute(0, 2, 3, 1).reshape(Cout, R)
    return wp


# ---- the single kernels (channels-last) ---------------------------------------------------------------------------------------------------
def _check_on(dev, named) -> None:
    """Every (name, tensor, dtype) a launch would read is a tensor of that dtype on `dev` (None passes), or the call is refused on the
    host with a ValueError before anything is launched: a kernel handed a host address faults the device."""
    for name, t, dt in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the images on {dev}")
        if t.dtype != dt:
            raise ValueError(f"{name}: expected {dt}, got {t.dtype}")


def conv2d_ref(x, weight, bias, stride: int = 1, padding: int = 0, relu: bool = False, acc: Optional[torch.dtype] = None):
    """F.conv2d on the permuted tensor, in `acc` when given; (N, H, W, Cin) -> (N, Ho, Wo, Cout)."""
    if acc is not None:
        x, weight, bias = x.to(acc), weight.to(acc), None if bias is None else bias.to(acc)
    y = F.conv2d(x.permute(0, 3, 1, 2), weight, bias, stride=stride, padding=padding).permute(0, 2, 3, 1)
    return torch.relu(y) if relu else y


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, padding: int = 0,
           relu: bool = False, ops: str = "fused", *, packed: Optional[torch.Tensor] = None, chunk: int = 0) -> torch.Tensor:
    """x (N, H, W, Cin) -> (N, Ho, Wo, Cout): gh_conv2d_forward for a float32 ROCm tensor (K in 3, 5, 11; stride 1 or 4), conv2d_ref
    for ops="torch" and for everything else torch takes. `packed` is pack_conv(weight) where the caller keeps it; `chunk`
    (0, 32, 64, 128) fixes the kernel's chunk of output channels, which no result depends on."""
    check_ops(ops)
    if ops != "fused" or not on_device(x):
        return conv2d_ref(x, weight, bias, stride, padding, relu)
    Cout, Cin, K, K2 = weight.shape
    if K != K2 or x.shape[3] != Cin:
        raise ValueError(f"conv2d: x {tuple(x.shape)} does not fit the weight {tuple(weight.shape)}")
    _check_on(x.device, (("weight", weight, torch.float32), ("bias", bias, torch.float32), ("packed", packed, torch.float32)))
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"conv2d: bias {tuple(bias.shape)} does not fit the weight {tuple(weight.shape)}")
    if packed is not None and packed.numel() != pad_to(Cout, _abi.GH_LPIPS_CHUNK) * (-(-K * K * Cin // 4) * 4):
        raise ValueError(f"conv2d: packed {tuple(packed.shape)} is not pack_conv of a weight {tuple(weight.shape)}")
    x = x.detach().contiguous()
    wp = pack_conv(weight) if packed is None else packed.contiguous()
    b = None if bias is None else bias.detach().contiguous()
    N, H, W, _ = x.shape
    out = lambda s: 0 if s + 2 * padding < K else (s + 2 * padding - K) // stride + 1
    y = torch.empty(N, out(H), out(W), Cout, dtype=torch.float32, device=x.device)
    launch("gh_conv2d_forward", x.device, ptr(x), N, H, W, Cin, Cout, K, stride, padding, ptr(wp), ptr(b), _abi.GH_LPIPS_RELU if relu else 0,
           chunk, ptr(y), what=f"gh_conv2d_forward (N={N}, H={H}, W={W}, Cin={Cin}, Cout={Cout}, K={K}, s={stride}, p={padding})")
    return y


def max_pool3x3s2(x: torch.Tensor, ops: str = "fused") -> torch.Tensor:
    """x (N, H, W, C) -> (N, Ho, Wo, C): F.max_pool2d(kernel 3, stride 2) channels-last."""
    check_ops(ops)
    if ops != "fused" or not on_device(x):
        return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    x = x.detach().contiguous()
    N, H, W, Cn = x.shape
    out = lambda s: 0 if s < 3 else (s - 3) // 2 + 1
    y = torch.empty(N, out(H), out(W), Cn, dtype=torch.float32, device=x.device)
    launch("gh_maxpool3x3s2_forward", x.device, ptr(x), N, H, W, Cn, ptr(y), what=f"gh_maxpool3x3s2_forward ({N}, {H}, {W}, {Cn})")
    return y


def lpips_layer_ref(f: torch.Tensor, lin: torch.Tensor, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """LPIPS' head for one tap on a channels-last (2N, h, w, C) map whose images n and n + N are pair n: (N,) in f's dtype (`acc`)."""
    if acc is not None:
        f, lin = f.to(acc), lin.to(acc)
    N = f.shape[0] // 2
    u = f / (f.pow(2).sum(dim=3, keepdim=True).sqrt() + 1e-10)
    return (lin.view(1, 1, 1, -1) * (u[:N] - u[N:]) ** 2).sum(dim=3).mean(dim=(1, 2))


def lpips_layer(f: torch.Tensor, lin: torch.Tensor, ops: str = "fused") -> torch.Tensor:
    """d_l of a (2N, h, w, C) map and a (C,) `lin` weight: (N,) float64 (gh_lpips_layer on a float32 ROCm tensor)."""
    check_ops(ops)
    if ops != "fused" or not on_device(f):
        return lpips_layer_ref(f, lin).double()
    _check_on(f.device, (("lin", lin, torch.float32),))
    if f.shape[0] % 2 or tuple(lin.shape) != (f.shape[3],):
        raise ValueError(f"lpips_layer: expected an even number of images and lin ({f.shape[3]},), got {tuple(f.shape)} and {tuple(lin.shape)}")
    f = f.detach().contiguous()
    N, P, Cn = f.shape[0] // 2, f.shape[1] * f.shape[2], f.shape[3]
    score = torch.zeros(N, dtype=torch.float64, device=f.device)
    nbytes = lib().gh_lpips_layer_workspace(N, P)
    ws = workspace(nbytes, f.device)
    launch("gh_lpips_layer", f.device, ptr(f), N, P, Cn, ptr(lin.detach().contiguous()), 0, ptr(score), None, ptr(ws), nbytes,
           what=f"gh_lpips_layer (N={N}, P={P}, C={Cn})")
    return score


def _in_place(t: torch.Tensor, layout: str, name: str):
    """(tensor, channel_last) as the kernel reads it: float32 in place where its memory is either (N,3,H,W) or (N,H,W,3), whatever
    the logical layout (metrics._images' rule)."""
    from .metrics import _images
    return _images(t, layout, name)


def prepare_input(pred: torch.Tensor, gt: torch.Tensor, bbox: Optional[torch.Tensor], hw: Tuple[int, int], *,
                  bbox_mask: Optional[torch.Tensor] = None, layout: str = "chw", quantize: bool = True, signed: bool = False,
                  shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """gh_lpips_prepare: the network's (2N, h, w, 3) input from ROCm images (N,3,H,W) / (N,H,W,3), cropped at bbox[n] (an (N, 4) int32
    device tensor in ImageScores.bbox's format, or None for the origin), the prediction zeroed where bbox_mask == 0, quantised and
    scaled. hw = (h, w) is the crop size; a view whose own box has another size comes out as NaN."""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda):
        raise ValueError("prepare_input: pred must be a tensor on a ROCm device")
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout must be 'chw' or 'hwc', got {layout!r}")
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    dev = pred.device
    _check_on(dev, (("gt", gt, gt.dtype), ("bbox", bbox, torch.int32), ("bbox_mask", bbox_mask, torch.uint8),
                    ("shift", shift, torch.float32), ("scale", scale, torch.float32)))
    p, p_hwc = _in_place(pred, layout, "pred")
    g, g_hwc = _in_place(gt, layout, "gt")
    N, H, W = (pred.shape[0], pred.shape[2], pred.shape[3]) if layout == "chw" else pred.shape[:3]
    h, w = int(hw[0]), int(hw[1])
    if tuple(shift.shape) != (3,) or tuple(scale.shape) != (3,):
        raise ValueError(f"shift and scale: expected (3,), got {tuple(shift.shape)} and {tuple(scale.shape)}")
    if bbox is not None and tuple(bbox.shape) != (N, 4):
        raise ValueError(f"bbox: expected ({N}, 4), got {tuple(bbox.shape)}")
    if bbox_mask is not None and tuple(bbox_mask.shape) != (N, H, W):
        raise ValueError(f"bbox_mask: expected ({N}, {H}, {W}), got {tuple(bbox_mask.shape)}")
    bbox = None if bbox is None else bbox.contiguous()
    bbox_mask = None if bbox_mask is None else bbox_mask.contiguous()
    shift, scale = shift.contiguous(), scale.contiguous()
    x = torch.empty(2 * N, h, w, 3, dtype=torch.float32, device=p.device)
    flags = ((_abi.GH_LPIPS_PRED_HWC if p_hwc else 0) | (_abi.GH_LPIPS_GT_HWC if g_hwc else 0) | (_abi.GH_LPIPS_QUANTIZE if quantize else 0) |
             (_abi.GH_LPIPS_SIGNED if signed else 0))
    launch("gh_lpips_prepare", p.device, ptr(p), ptr(g), ptr(bbox_mask), ptr(bbox), N, H, W, h, w, flags, ptr(shift), ptr(scale), ptr(x),
           what=f"gh_lpips_prepare (N={N}, H={H}, W={W}, h={h}, w={w})")
    return x


# ---- the network -------------------------------------------------------------------------------------------------------------------------
class AlexLPIPS(nn.Module):
    """The frozen parameters of LPIPS over AlexNet: `conv1` .. `conv5` (torchvision alexnet `features` 0, 3, 6, 8, 10), `lin1` .. `lin5`
    (the (C,) weights of the bias-free 1x1 layers) and the scaling layer's `shift` / `scale`. `widths` are the five channel counts
    (the tests run a network of a few channels). The packed layouts the kernels read are cached per device.

    load_state_dict accepts three key forms and ignores other keys: this module's own; torchvision's `features.{0,3,6,8,10}.weight/bias`;
    and the lpips package's `net.slice{1..5}.{0,3,6,8,10}.weight/bias`, `lin{k}.model.1.weight` (k = 0 .. 4) or `lins.{k}.model.1.weight`,
    `scaling_layer.shift` / `scaling_layer.scale`. The package's names are written from memory of lpips 0.1, not checked against it:
    the package is not a dependency. With it installed: net.load_state_dict(lpips.LPIPS(net='alex').state_dict())."""

    def __init__(self, widths: Sequence[int] = WIDTHS):
        super().__init__()
        if len(widths) != 5 or any(int(w) < 1 for w in widths):
            raise ValueError(f"widths: expected five positive channel counts, got {widths!r}")
        self.widths = tuple(int(w) for w in widths)
        ch = (3,) + self.widths
        for k, (_, K, s, p, _) in enumerate(CONVS, 1):
            setattr(self, f"conv{k}", nn.Conv2d(ch[k - 1], ch[k], K, stride=s, padding=p))
            setattr(self, f"lin{k}", nn.Parameter(torch.ones(ch[k])))
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32))
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed = None

    @classmethod
    def synthetic(cls, seed: int = 0, widths: Sequence[int] = WIDTHS) -> "AlexLPIPS":
        """Random weights (He-scaled convolutions, small biases, non-negative `lin` with a few exact zeros): the real ones cannot be
        fetched here. The scores of such a network are no LPIPS, but every kernel runs as it does with the real weights."""
        net = cls(widths)
        gen = torch.Generator().manual_seed(1000 + int(seed))
        with torch.no_grad():
            for k in range(1, 6):
                conv = getattr(net, f"conv{k}")
                fan = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / fan) ** 0.5)
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)
                lin = torch.rand(conv.weight.shape[0], generator=gen)
                lin[::5] = 0.0
                getattr(net, f"lin{k}").copy_(lin)
        return net

    def convs(self):
        return [getattr(self, f"conv{k}") for k in range(1, 6)]

    def lins(self):
        return [getattr(self, f"lin{k}") for k in range(1, 6)]

    def packed(self):
        """(wp, bias, lin) x 5 as the kernels read them, repacked when a parameter was replaced, written or moved."""
        params = [t for c in self.convs() for t in (c.weight, c.bias)] + self.lins()
        key = tuple((t.data_ptr(), t._version, t.device) for t in params)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, [(pack_conv(c.weight), c.bias.detach().float().contiguous(), l.detach().float().contiguous())
                                  for c, l in zip(self.convs(), self.lins())])
        return self._packed[1]

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        own = {}
        conv_of = {n: k for k, (n, *_) in enumerate(CONVS, 1)}
        for key, v in state_dict.items():
            parts = key.split(".")
            if parts[0] == "net" and len(parts) == 4 and parts[1].startswith("slice") and parts[2].isdigit():
                parts = ["features"] + parts[2:]
            if parts[0] == "features" and len(parts) == 3 and parts[1].isdigit() and parts[2] in ("weight", "bias"):
                if int(parts[1]) in conv_of:
                    own[f"conv{conv_of[int(parts[1])]}.{parts[2]}"] = v
            elif parts[-3:] == ["model", "1", "weight"] and (len(parts) == 4 and parts[0][:3] == "lin" and parts[0][3:].isdigit()
                                                             or len(parts) == 5 and parts[0] == "lins" and parts[1].isdigit()):
                k = int(parts[0][3:]) if len(parts) == 4 else int(parts[1])
                if 0 <= k < 5:
                    own[f"lin{k + 1}"] = v.reshape(-1)
            elif parts[0] == "scaling_layer" and len(parts) == 2 and parts[1] in ("shift", "scale"):
                own[parts[1]] = v.reshape(-1)
            elif key in ("shift", "scale") or (len(parts) == 1 and key[:3] == "lin" and key[3:].isdigit()) or \
                    (len(parts) == 2 and parts[0][:4] == "conv" and parts[0][4:].isdigit()):
                own[key] = v
        self._packed = None
        return super().load_state_dict(own, strict=strict, **kw)


def _check_pair(x0: torch.Tensor, x1: torch.Tensor) -> None:
    if x0.dim() != 4 or x0.shape[1] != 3 or tuple(x0.shape) != tuple(x1.shape):
        raise ValueError(f"expected two (N, 3, H, W) stacks of one shape, got {tuple(x0.shape)} and {tuple(x1.shape)}")
    if x0.shape[2] < MIN_SIZE or x0.shape[3] < MIN_SIZE:
        raise ValueError(f"LPIPS over AlexNet needs images of at least {MIN_SIZE}x{MIN_SIZE} pixels, got {x0.shape[2]}x{x0.shape[3]}")


def lpips_ref(net: AlexLPIPS, x0: torch.Tensor, x1: torch.Tensor, acc: Optional[torch.dtype] = None, terms: bool = False):
    """lpips.LPIPS(net='alex').forward(x0, x1) in plain torch ops (channels-first as the package runs it), in `acc` when given: (N,) in
    that dtype, with terms=True also the (5, N) per-tap terms. The CPU path and the tests' yardstick."""
    _check_pair(x0, x1)
    dt = acc if acc is not None else (x0.dtype if x0.is_floating_point() else torch.float32)
    shift, scale = net.shift.to(dt).view(1, 3, 1, 1), net.scale.to(dt).view(1, 3, 1, 1)
    h = torch.cat([(x0.to(dt) - shift) / scale, (x1.to(dt) - shift) / scale]).contiguous()   # one memory order, whatever view came in
    N, ds = x0.shape[0], []
    for (_, K, s, p, pool), conv, lin in zip(CONVS, net.convs(), net.lins()):
        if pool:
            h = F.max_pool2d(h, 3, 2)
        h = torch.relu(F.conv2d(h, conv.weight.to(dt), conv.bias.to(dt), stride=s, padding=p))
        u = h / (h.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        ds.append((lin.to(dt).view(1, -1, 1, 1) * (u[:N] - u[N:]) ** 2).sum(dim=1).mean(dim=(1, 2)))
    d = torch.stack(ds)
    total = (((d[0] + d[1]) + d[2]) + d[3]) + d[4]
    return (total, d) if terms else total


def _net_tensors(net: AlexLPIPS):
    return [(f"net.{k}", t) for k, t in list(net.named_parameters()) + list(net.named_buffers())]


def _check_net(net: AlexLPIPS, dev) -> None:
    """The network lives on the images' device, or ValueError — on the host, before any launch, whichever path would run."""
    for name, t in _net_tensors(net):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the images on {dev}: move the network first (net.to(device))")


def _fused_applies(net: AlexLPIPS, x: torch.Tensor) -> bool:
    """Float32 ROCm images and a float32 network of supported widths; anything else runs the torch statements."""
    return (x.is_cuda and x.dtype == torch.float32 and all(w <= MAX_C for w in net.widths) and
            all(t.dtype == torch.float32 for _, t in _net_tensors(net)))


def _forward_fused(net: AlexLPIPS, x: torch.Tensor, N: int, want_terms: bool):
    """gh_lpips_forward on a prepared (2N, h, w, 3) input: (scores (N,), terms (5, N) or None), float64."""
    dev = x.device
    _check_net(net, dev)
    _check_on(dev, [(name, t, torch.float32) for name, t in _net_tensors(net)])
    if not on_device(x) or x.shape[0] != 2 * N or x.shape[3] != 3:
        raise ValueError(f"expected a prepared (2N, h, w, 3) float32 input on a ROCm device, got {tuple(x.shape)}")
    x = x.contiguous()
    h, w = x.shape[1], x.shape[2]
    widths = (C.c_int * 5)(*net.widths)
    nbytes = lib().gh_lpips_workspace(N, h, w, widths)
    if nbytes == 0:
        raise RuntimeError(f"gh_lpips_workspace refused (N={N}, h={h}, w={w}, widths={net.widths})")
    packed = net.packed()
    wts = _abi.GhLpipsWeights()
    for l, (wp, b, lin) in enumerate(packed):
        wts.w[l], wts.b[l], wts.lin[l] = wp.data_ptr(), b.data_ptr(), lin.data_ptr()
    ws = workspace(nbytes, dev)
    scores = torch.empty(N, dtype=torch.float64, device=dev)
    terms = torch.empty(5, N, dtype=torch.float64, device=dev) if want_terms else None
    launch("gh_lpips_forward", dev, ptr(x), N, h, w, widths, C.byref(wts), ptr(scores), ptr(terms), ptr(ws), nbytes,
           what=f"gh_lpips_forward (N={N}, h={h}, w={w}, widths={net.widths})")
    return scores, terms


def lpips_distance(net: AlexLPIPS, x0: torch.Tensor, x1: torch.Tensor, *, ops: str = "fused", terms: bool = False):
    """LPIPS of N pairs: x0, x1 (N, 3, H, W) in [-1, 1] -> (N,) float64 (with terms=True also the (5, N) per-tap terms). Raises ValueError
    under 31x31. Never synchronises on ROCm tensors (graph capturable)."""
    check_ops(ops)
    _check_pair(x0, x1)
    _check_net(net, x0.device)
    if ops != "fused" or not _fused_applies(net, x0) or x1.dtype != x0.dtype or x1.device != x0.device:
        out = lpips_ref(net, x0, x1, terms=terms)
        return (out[0].double(), out[1].double()) if terms else out.double()
    N = x0.shape[0]
    if N == 0:
        z = torch.zeros(0, dtype=torch.float64, device=x0.device)
        return (z, z.new_zeros(5, 0)) if terms else z
    x = prepare_input(x0, x1, None, (x0.shape[2], x0.shape[3]), quantize=False, signed=True, shift=net.shift, scale=net.scale)
    scores, t = _forward_fused(net, x, N, terms)
    return (scores, t) if terms else scores


# ---- the evaluator's protocol ---------------------------------------------------------------------------------------------------------------
def quantize_unit(v: torch.Tensor, quantize: bool = True) -> torch.Tensor:
    """[0, 1] float32 -> [-1, 1] as the reference's PNG round trip and im2tensor give it (module docstring); a NaN stays."""
    t = v.float() * 255.0
    if quantize:
        t = torch.clamp(torch.round(t), 0.0, 255.0)
    return (t.double() / 127.5 - 1.0).float()


def _boxes(mask_at_box: torch.Tensor) -> torch.Tensor:
    """cv2.boundingRect per view of an (Nv, H, W) mask, as image_scores gives it: (Nv, 4) int32 (x, y, w, h) on the mask's device,
    zeros for an empty mask. Plain torch reductions, no synchronisation."""
    m = mask_at_box != 0
    Nv, H, W = m.shape
    rows, cols = m.any(dim=2), m.any(dim=1)
    y0, x0 = rows.int().argmax(dim=1), cols.int().argmax(dim=1)
    y1, x1 = H - 1 - rows.flip(1).int().argmax(dim=1), W - 1 - cols.flip(1).int().argmax(dim=1)
    box = torch.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], dim=1)
    return torch.where(rows.any(dim=1, keepdim=True), box, torch.zeros_like(box)).to(torch.int32)


def _scores_torch(net, pred, gt, boxes, bbm, layout, quantize) -> torch.Tensor:
    """The protocol view by view in torch statements on the tensors' device: the CPU path and ops="torch"."""
    if layout == "hwc":
        pred, gt = pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)
    out = torch.full((pred.shape[0],), math.nan, dtype=torch.float64, device=pred.device)
    for v, (bx, by, bw, bh) in enumerate(boxes):
        if bw < MIN_SIZE or bh < MIN_SIZE:
            continue
        p, g = pred[v:v + 1, :, by:by + bh, bx:bx + bw].float(), gt[v:v + 1, :, by:by + bh, bx:bx + bw].float()
        if bbm is not None:
            p = torch.where(bbm[v:v + 1, None, by:by + bh, bx:bx + bw] != 0, p, torch.zeros((), dtype=p.dtype, device=p.device))
        out[v] = lpips_ref(net, quantize_unit(p, quantize), quantize_unit(g, quantize))[0].double()
    return out


def lpips_scores(net: AlexLPIPS, pred: torch.Tensor, gt: torch.Tensor, mask_at_box: Optional[torch.Tensor] = None, *,
                 bbox_mask: Optional[torch.Tensor] = None, layout: str = "chw", quantize: bool = True, ops: str = "fused") -> torch.Tensor:
    """LPIPS of Nv views by the evaluator's protocol (module docstring). pred, gt: (Nv,3,H,W) for layout="chw" or (Nv,H,W,3) for "hwc",
    in [0, 1]; mask_at_box, bbox_mask: (Nv,H,W) of any dtype, as image_scores takes them. Returns (Nv,) float64 on pred's device, NaN
    for a crop under 31 in either direction. On ROCm tensors: one device-to-host copy (the boxes; none without a mask), then one
    gh_lpips_prepare and one gh_lpips_forward per distinct crop size; the views of a size are read in place where they are one run of
    consecutive views (a single view always is) and gathered once otherwise. The caller's tensors are not written."""
    from .metrics import _mask
    check_ops(ops)
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout must be 'chw' or 'hwc', got {layout!r}")
    if pred.dim() != 4 or tuple(pred.shape) != tuple(gt.shape) or pred.shape[1 if layout == "chw" else 3] != 3:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)}: expected two stacks of one shape with 3 channels ({layout})")
    Nv, H, W = (pred.shape[0], pred.shape[2], pred.shape[3]) if layout == "chw" else pred.shape[:3]
    dev = pred.device
    bbm = None if bbox_mask is None else _mask(bbox_mask, (Nv, H, W), "bbox_mask", False)
    if gt.device != dev or (bbm is not None and bbm.device != dev):
        raise ValueError("pred, gt and the masks must be on the same device")
    _check_net(net, dev)
    if mask_at_box is None:
        boxes_dev, boxes = None, [(0, 0, W, H)] * Nv
    else:
        mbox = _mask(mask_at_box, (Nv, H, W), "mask_at_box", True)
        if mbox.device != dev:
            raise ValueError("pred, gt and the masks must be on the same device")
        boxes_dev = _boxes(mbox)
        boxes = [tuple(int(c) for c in b) for b in boxes_dev.cpu().tolist()]           # the one device-to-host copy
    return _scores_with_boxes(net, pred, gt, boxes_dev, boxes, bbm, layout, quantize, ops)


def _scores_with_boxes(net: AlexLPIPS, pred, gt, boxes_dev, boxes, bbm, layout: str, quantize: bool, ops: str) -> torch.Tensor:
    """lpips_scores behind its argument checks, for a caller that has the boxes already (metrics.Evaluator): boxes_dev the (Nv, 4)
    int32 device tensor (None: whole images), boxes the same numbers on the host, bbm the (Nv, H, W) mask or None."""
    dev, Nv = pred.device, pred.shape[0]
    _check_net(net, dev)
    fused = ops == "fused" and _fused_applies(net, pred) and gt.dtype == pred.dtype
    if not fused:
        return _scores_torch(net, pred.detach(), gt.detach(), boxes, bbm, layout, quantize)
    bbm8 = None if bbm is None else (bbm if bbm.dtype == torch.uint8 else bbm.to(torch.uint8))
    out = torch.full((Nv,), math.nan, dtype=torch.float64, device=dev)
    groups = {}
    for v, (_, _, bw, bh) in enumerate(boxes):
        if bw >= MIN_SIZE and bh >= MIN_SIZE:
            groups.setdefault((bh, bw), []).append(v)
    for (bh, bw), views in groups.items():
        n = len(views)
        if views == list(range(views[0], views[0] + n)):                              # one run: slices, nothing is copied
            sl = slice(views[0], views[0] + n)
            take = lambda t: None if t is None else t[sl]
        else:
            idx = torch.tensor(views, dtype=torch.long, device=dev)
            take = lambda t: None if t is None else t.index_select(0, idx)
        x = prepare_input(take(pred), take(gt), None if boxes_dev is None else take(boxes_dev).contiguous(), (bh, bw),
                          bbox_mask=None if bbm8 is None else take(bbm8).contiguous(), layout=layout, quantize=quantize,
                          shift=net.shift, scale=net.scale)
        s, _ = _forward_fused(net, x, n, False)
        if views == list(range(views[0], views[0] + n)):
            out[views[0]:views[0] + n] = s
        else:
            out.index_copy_(0, idx, s)
    return out
