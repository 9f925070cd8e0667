"""Shared by tests/test_perceptual_cpu.py and tests/test_gpu_perceptual.py: the cases of guassianhand_amd.perceptual, their float64
yardsticks and their kink margins. The tolerance rule is tests/res_block_cases.three_way.

A ReLU gate, a pool choice and the sign of a feature difference are discrete decisions that float32 and float64 can take
differently; such a flip would change a gradient by far more than the tolerance allows, and none can be excused as rounding. So
every case that compares gradients or pooled values first asserts, on its float64 reference alone, that

    every pre-activation v of every convolution has |v| > GUARD max|v| of its layer,
    every pooling window's two largest values differ by more than GUARD max|input|, unless they are exactly equal,
    every feature difference has |f - t| > GUARD max|f - t| of its map, unless f and t are both exactly 0,

with GUARD = 2^-16. Two window entries are exactly equal in float64 where both are ReLU zeros, or where their whole receptive fields
hold the same values — the flat regions of a rendered image, its background and its bbox-zeroed border. Every precision
reproduces the first kind, and a convolution whose result does not depend on the pixel's position (the header's promise) reproduces
the second bit for bit; in both the first of the equal entries wins everywhere, so such a window decides nothing by rounding.
The seeds below were chosen on the CPU (`python -m tests.perceptual_cases`; the fit's with the dense oracle renderer in the
rasteriser's place, taking the seed with the widest margins of the first 120: 7 times the guard) so that the margins hold; a case whose reference fails them fails its test.

CONV_CASES are (N, H, W, Cin, Cout, chunk). The kernel's constants are its 128-pixel tile, its 32-channel slab of input channels
with the lane halves' 16, and its chunk of 32, 64 or 128 output channels (`chunk`; 0 = the library's choice, which is 32 at sizes
like these): the issue's eight shapes run with the library's choice and with 128, and the shapes after them sit one either side of
each constant."""
import copy
import math
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

GUARD = 2.0 ** -16

_ISSUE = ((1, 1, 1, 1, 1), (1, 2, 3, 3, 5), (2, 5, 7, 3, 64), (1, 9, 15, 33, 31), (1, 8, 16, 64, 129), (2, 3, 50, 32, 32), (1, 4, 4, 512, 7),
          (1, 4, 4, 5, 512))
CONV_CASES = tuple(s + (ch,) for s in _ISSUE for ch in (0, 128)) + (
    (1, 1, 127, 3, 4, 0), (1, 3, 43, 4, 3, 0),                              # 127 and 129 pixels
    (1, 2, 3, 15, 6, 0), (1, 2, 3, 16, 6, 0), (1, 2, 3, 17, 6, 0),       # the lane halves' 16 input channels
    (1, 2, 3, 31, 6, 0), (1, 2, 2, 36, 8, 0),                               # the slab's 32; a multiple of 4 with a short last slab
    (1, 2, 3, 6, 31, 32), (1, 2, 3, 6, 32, 32), (1, 2, 3, 6, 33, 32),    # chunk 32
    (1, 2, 3, 6, 63, 64), (1, 2, 3, 6, 64, 64), (1, 2, 3, 6, 65, 64),    # chunk 64
    (1, 2, 3, 6, 127, 128), (1, 2, 3, 6, 128, 128),                         # chunk 128 (129: the issue's fifth shape)
)
# the seed of a shape (N, H, W, Cin, Cout) where it is not 0, found by the search below
SEEDS = {(1, 1, 127, 3, 4): 1, (1, 8, 16, 64, 129): 5, (1, 9, 15, 33, 31): 1, (2, 5, 7, 3, 64): 1}


def conv_id(case):
    N, H, W, Cin, Cout, chunk = case
    return f"N{N}-{H}x{W}-Cin{Cin}-Cout{Cout}-chunk{chunk}"


def conv_seed(case):
    return SEEDS.get(tuple(case[:5]), 0)


@lru_cache(maxsize=None)
def make_conv(shape, seed):
    """x (N, H, W, Cin), weight (Cout, Cin, 3, 3), bias, the cotangent g (N, H, W, Cout), on the CPU in float32."""
    N, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(31000 + 977 * seed + 13 * N + 7 * H + 5 * W + 3 * Cin + Cout)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return SimpleNamespace(x=rn(N, H, W, Cin), weight=rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin), bias=0.3 * rn(Cout), g=rn(N, H, W, Cout))


def conv_f64(c, relu):
    """{y, dx} of the float64 restatement on the CPU, and the pre-activation."""
    from guassianhand_amd.perceptual import conv3x3_ref
    x = c.x.double().requires_grad_(True)
    pre = conv3x3_ref(x, c.weight, c.bias, False, acc=torch.float64)
    y = torch.relu(pre) if relu else pre
    y.backward(c.g.double())
    return dict(y=y.detach(), dx=x.grad), pre.detach()


def conv_run(c, relu, ops, chunk, device):
    """{y, dx} of guassianhand_amd.perceptual.conv3x3 on `device`."""
    from guassianhand_amd.perceptual import conv3x3
    x = c.x.to(device).requires_grad_(True)
    y = conv3x3(x, c.weight.to(device), c.bias.to(device), relu, ops, chunk=chunk)
    y.backward(c.g.to(device))
    return dict(y=y.detach().cpu(), dx=x.grad.cpu())


def relu_margin(pre):
    return float(pre.abs().min() / pre.abs().max()) if pre.numel() else math.inf


def pool_margin(v):
    """The smallest top-two gap of the 2x2 windows of v (N, C, H, W) over max|v|; windows whose two largest are exactly equal are exempt."""
    N, Cn, H, W = v.shape
    if H < 2 or W < 2 or v.numel() == 0:
        return math.inf
    w = F.unfold(v.reshape(N * Cn, 1, H, W), 2, stride=2)                # (N C, 4, windows)
    top = w.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    gap = gap[gap != 0]
    return float(gap.min() / v.abs().max()) if gap.numel() else math.inf


def sign_margin(f, t):
    d = (f - t).abs()
    d = d[~((f == 0) & (t == 0))]
    return float(d.min() / d.max()) if d.numel() else math.inf


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def make_features(widths, seed=0):
    """A VGG19Features of the given widths on the CPU with weights ~ N(0, 2 / (9 Cin)) and biases ~ 0.1 N(0, 1)."""
    from guassianhand_amd.perceptual import CONVS, VGG19Features
    f = VGG19Features(widths)
    gen = torch.Generator().manual_seed(4100 + seed)
    with torch.no_grad():
        for _, n, _, _ in CONVS:
            conv = f.conv(n)
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * math.sqrt(2.0 / (9 * conv.weight.shape[1])))
            conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=gen))
    return f


def net_margins(features, x, y):
    """(relu, pool, sign) margins of VGGLoss(x, y) over `features` in float64 on the CPU: x, y (B, 3, H, W)."""
    from guassianhand_amd.perceptual import CONVS, POOL_BEFORE, TAPS, _normalised
    features = copy.deepcopy(features).cpu()

    def walk(img):
        h = _normalised(img.detach().cpu(), torch.float64).permute(0, 3, 1, 2)
        relu, pool, taps = math.inf, math.inf, []
        for _, n, _, _ in CONVS:
            if n in POOL_BEFORE:
                pool = min(pool, pool_margin(h))
                h = F.max_pool2d(h, 2)
            conv = features.conv(n)
            pre = F.conv2d(h, conv.weight.double(), conv.bias.double(), padding=1)
            relu = min(relu, relu_margin(pre))
            h = torch.relu(pre)
            if n in TAPS:
                taps.append(h)
        return relu, pool, taps

    rx, px, fx = walk(x)
    ry, py, fy = walk(y)
    return min(rx, ry), min(px, py), min(sign_margin(f, t) for f, t in zip(fx, fy))


def assert_net_margins(features, x, y, tag=""):
    m = net_margins(features, x, y)
    print(f"{tag} margins: relu {m[0]:.3e}, pool {m[1]:.3e}, sign {m[2]:.3e} (guard {GUARD:.3e})")
    assert min(m) > GUARD, (tag, m)


LOSS_WIDTHS = (4, 5, 6, 7)
# (B, H, W, seed): after three pools the 8x8 image reaches 1x1
LOSS_CASES = ((2, 9, 11, 3), (1, 8, 8, 0))


def make_images(B, H, W, seed):
    gen = torch.Generator().manual_seed(5200 + 31 * seed + B + 3 * H + W)
    return torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 3, H, W, generator=gen)


def loss_f64(features, x, y):
    """{loss, dimg} of perceptual_loss_ref in float64 on the CPU."""
    from guassianhand_amd.perceptual import perceptual_loss_ref
    xl = x.detach().cpu().double().requires_grad_(True)
    loss = perceptual_loss_ref(copy.deepcopy(features).cpu(), xl, y.detach().cpu(), acc=torch.float64)
    loss.backward()
    return dict(loss=loss.detach(), dimg=xl.grad)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------
FIT_WIDTHS, FIT_SEED = (4, 4, 8, 8), 83


def fit_case(seed=FIT_SEED, device="cpu"):
    """A two-view 16x16 fit problem of tests/helpers.tiny_fit_problem with random targets, a bbox that zeroes a border, and a small
    network: `args` are step()'s arguments, `feats` lives on the CPU."""
    from tests.helpers import tiny_fit_problem
    pb = tiny_fit_problem(P=160, n_views=2, hw=(16, 16), map_hw=(16, 32), device=device)
    gen = torch.Generator().manual_seed(2100 + seed)
    H = W = 16
    gt, mask = torch.rand(2, H, W, 3, generator=gen), (torch.rand(2, H, W, generator=gen) > 0.5).float()
    bbox = torch.ones(2, H, W)
    bbox[:, :3], bbox[:, :, 13:] = 0, 0
    gt, mask, bbox = gt.to(device), mask.to(device), bbox.to(device)
    return SimpleNamespace(pb=pb, gt=gt, mask=mask, bbox=bbox, feats=make_features(FIT_WIDTHS, seed=10 + seed),
                           args=(pb["w2c"], pb["K"], H, W, pb["bg"], gt, mask, bbox))


def fit_margins_on_the_cpu(seed):
    """The margins of the fit case's first step with the dense oracle renderer in the rasteriser's place (the seed search)."""
    from tests.helpers import oracle_render_views
    c = fit_case(seed)
    pb, n = c.pb, c.pb["uv"].shape[0]
    img = oracle_render_views(pb["gs"], *c.args[:5], color_w=torch.ones(48), xyz_b=torch.zeros(3), color_b=torch.zeros(n, 48),
                              opacity_b=torch.zeros(n, 1))["comp_rgb"]
    return net_margins(c.feats, (img * c.bbox[..., None]).permute(0, 3, 1, 2), c.gt.permute(0, 3, 1, 2))


# ---- pooling ----------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = ((1, 1), (2, 2), (3, 5), (7, 8))
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def make_pool(H, W, N=2, Cn=3):
    """x (N, H, W, C) of small integers (ties everywhere) and, where the image has windows for them, one window per pair of positions
    whose two entries tie for the maximum, a NaN in each position, two NaNs, +inf, a window of -inf and one of -inf with a number."""
    gen = torch.Generator().manual_seed(600 + 10 * H + W)
    x = torch.randint(-3, 4, (N, H, W, Cn), generator=gen).float()
    wins = [(n, i, j, c) for n in range(N) for c in range(Cn) for i in range(H // 2) for j in range(W // 2)]
    nan, inf = float("nan"), float("inf")
    special = [tuple(5.0 if q in pr else float(-q) for q in range(4)) for pr in PAIRS]
    special += [tuple(nan if q == k else 1.0 for q in range(4)) for k in range(4)]
    special += [(nan, 2.0, nan, 3.0), (1.0, inf, inf, 0.0), (-inf, -inf, -inf, -inf), (-inf, -inf, -2.0, -inf), (inf, nan, 1.0, -inf)]
    if len(wins) >= len(special):
        for (n, i, j, c), vals in zip(wins[::max(1, len(wins) // len(special))], special):
            for q, v in enumerate(vals):
                x[n, 2 * i + (q >> 1), 2 * j + (q & 1), c] = v
    elif wins:
        n, i, j, c = wins[0]
        x[n, 2 * i, 2 * j, c], x[n, 2 * i + 1, 2 * j + 1, c] = nan, inf
    g = torch.randn(N, H // 2, W // 2, Cn, generator=gen)
    return x, g, len(wins) >= len(special)


def pool_cpu(x, g):
    """(y, choice, dx) of F.max_pool2d and its autograd on the CPU in float32, channels-last like the kernels' tensors."""
    xl = x.clone().requires_grad_(True)
    N, H, W, Cn = x.shape
    if H < 2 or W < 2:                                       # F.max_pool2d refuses an empty output: nothing pooled, a zero gradient
        return x.new_zeros(N, H // 2, W // 2, Cn), torch.zeros(N, H // 2, W // 2, Cn, dtype=torch.uint8), torch.zeros_like(x)
    y, idx = F.max_pool2d(xl.permute(0, 3, 1, 2), 2, return_indices=True)
    y.backward(g.permute(0, 3, 1, 2))
    dx = xl.grad
    ih, iw = idx // W, idx % W
    oh = torch.arange(H // 2).view(1, 1, -1, 1)
    ow = torch.arange(W // 2).view(1, 1, 1, -1)
    choice = (2 * (ih - 2 * oh) + (iw - 2 * ow)).to(torch.uint8)
    return y.detach().permute(0, 2, 3, 1).contiguous(), choice.permute(0, 2, 3, 1).contiguous(), dx


def bits(t):
    return t.contiguous().view(torch.int32)


if __name__ == "__main__":                                   # the seed search: per case, the first seed whose margins hold
    for shape in sorted(set(tuple(c[:5]) for c in CONV_CASES)):
        for seed in range(200):
            m = relu_margin(conv_f64(make_conv(shape, seed), True)[1])
            if m > 2 * GUARD:
                break
        print(f"conv {shape}: seed {seed}, relu margin {m:.3e}{'' if SEEDS.get(shape, 0) == seed else '   <-- SEEDS'}")
    for B, H, W, _ in LOSS_CASES:
        for seed in range(200):
            m = net_margins(make_features(LOSS_WIDTHS, seed), *make_images(B, H, W, seed))
            if min(m) > 2 * GUARD:
                break
        print(f"loss {(B, H, W)}: seed {seed}, margins {m}")
    best = max(range(120), key=lambda seed: min(fit_margins_on_the_cpu(seed)))      # a rendered image is smooth: the widest margins
    print(f"fit: seed {best}, margins {fit_margins_on_the_cpu(best)}{'' if best == FIT_SEED else '   <-- FIT_SEED'}")
