"""Shared by tests/test_conv_bits_cpu.py, tests/test_gpu_conv_bits.py and tools/record_conv_bits.py: the cases whose output bits
tests/golden/conv_bits.json records for the two pixel-column convolutions (gh_conv.hip's 3x3 both ways, gh_lpips.hip's dense one)
and for the two pooling kernels, and the inputs they run on.

The inputs come from no random generator, so the fixture depends on no library's stream: element i of a tensor is
((i * 2654435761 + salt) mod 65521) / 65521 - 1/2 — integer arithmetic on the flat index, then correctly rounded float64 division and
subtraction — times a float64 scale (1 / sqrt(fan_in) for weights: sqrt and division are correctly rounded too), cast to float32.
The pooling inputs are small integers of the same sequence (ties everywhere) with a window of -inf, -inf beside a number, and NaNs.

A case id maps to {output name: SHA-256 of the output's contiguous little-endian bytes}."""
import hashlib
import math
from functools import lru_cache

import torch

from tests import lpips_cases as LC
from tests import perceptual_cases as PC

MUL, MOD = 2654435761, 65521
CHUNKS = (0, 32, 64, 128)
# (N, H, W, Cin, Cout): the lane halves' 16 channels + 1, three input channels, a short last slab with an odd width, a chunk boundary
# over two slabs, 127 pixels
CONV3X3_SHAPES = ((1, 2, 3, 17, 6), (2, 5, 7, 3, 64), (1, 9, 15, 33, 31), (1, 8, 16, 64, 129), (1, 1, 127, 3, 4))
# where gh_lpips.h's order is gh_conv.h's (Cin > GH_LPIPS_FLAT_CIN, K 3, stride 1, padding 1): one side of the flat threshold, a short
# last slab, a partial tile, a chunk boundary, and a pixel whose taps are all padding but the centre
AGREE_SHAPES = ((1, 2, 3, 17, 6), (2, 5, 7, 33, 31), (1, 3, 5, 64, 129), (1, 1, 1, 37, 40))


def _index(n: int, salt: int) -> torch.Tensor:
    return (torch.arange(n, dtype=torch.int64) * MUL + salt) % MOD


def unit(shape, salt: int, scale: float = 1.0) -> torch.Tensor:
    """The module docstring's sequence in [-1/2, 1/2) times `scale`, as a float32 tensor of `shape`."""
    n = math.prod(shape)
    return ((_index(n, salt).double() / MOD - 0.5) * scale).float().reshape(shape)


def small_ints(shape, salt: int, span: int = 5) -> torch.Tensor:
    """Integers -(span // 2) .. span // 2 of the same sequence, as float32: most windows hold equal values."""
    return (_index(math.prod(shape), salt) % span - span // 2).float().reshape(shape)


def _salt(*dims) -> int:
    s = 0
    for d in dims:
        s = s * 131 + d
    return s


@lru_cache(maxsize=None)
def conv_inputs(N, H, W, Cin, Cout, K):
    """x (N, H, W, Cin), weight (Cout, Cin, K, K) / sqrt(fan_in), bias (Cout,), cotangent g of a same-size output (N, H, W, Cout)."""
    s = _salt(N, H, W, Cin, Cout, K)
    return (unit((N, H, W, Cin), s + 1, 2.0), unit((Cout, Cin, K, K), s + 2, 2.0 / math.sqrt(K * K * Cin)), unit((Cout,), s + 3, 0.6),
            unit((N, H, W, Cout), s + 4, 2.0))


def pool2x2_input(H, W, N=2, Cn=3):
    """x (N, H, W, C) and the cotangent g (N, H/2, W/2, C): ties everywhere; where the image has room, a NaN in window positions 1 and
    3, a window of -inf, and one of -inf with a number."""
    x, g = small_ints((N, H, W, Cn), _salt(H, W, 2)), unit((N, H // 2, W // 2, Cn), _salt(H, W, 3))
    nan, inf = float("nan"), float("inf")
    if H >= 2 and W >= 2:
        x[0, 0, 1, 0] = nan
        x[N - 1, H - 1, W - 1] = nan
        x[N - 1, :2, :2, 1] = -inf
    if H >= 2 and W >= 4:
        x[N - 1, :2, 2:4, 2] = -inf
        x[N - 1, 1, 2, 2] = -2.0
        x[0, 0, 3, 1] = inf
    return x, g


def pool3x3_input(H, W, Cn):
    """x (3, H, W, C): image 0 of distinct values, image 1 of few (ties) with a window of -inf, image 2 with NaNs and a -inf."""
    x = unit((3, H, W, Cn), _salt(H, W, Cn, 5))
    x[1] = small_ints((H, W, Cn), _salt(H, W, Cn, 6), 3)
    x[1, :3, :3] = float("-inf")
    x[2, 1, 1] = float("nan")
    x[2, H - 1, W - 1] = float("nan")
    x[2, 0, 0] = float("-inf")
    return x


# ---- the cases: (id, kind, parameters) ----------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for N, H, W, Cin, Cout in CONV3X3_SHAPES:
        for relu in (0, 1):
            for ch in CHUNKS:
                out.append((f"conv3x3-N{N}-{H}x{W}-Cin{Cin}-Cout{Cout}-relu{relu}-chunk{ch}", "conv3x3", (N, H, W, Cin, Cout, relu, ch)))
    for case in LC.CONV_CASES:
        for full in (1, 0):                                  # bias + ReLU, or neither
            for ch in LC.CHUNKS:
                out.append((f"conv2d-{LC.case_id(case)}-{'bias-relu' if full else 'plain'}-chunk{ch}", "conv2d", (case, full, ch)))
    for H, W in PC.POOL_SHAPES:
        out.append((f"pool2x2-{H}x{W}", "pool2x2", (H, W)))
    for H, W in LC.POOL_SHAPES:
        for Cn in LC.POOL_CHANNELS:
            out.append((f"pool3x3s2-{H}x{W}-C{Cn}", "pool3x3s2", (H, W, Cn)))
    return tuple(out)


CASES = _cases()
IDS = tuple(c[0] for c in CASES)


def sha(t: torch.Tensor) -> str:
    """SHA-256 of the tensor's contiguous bytes (the hosts and the device are little-endian)."""
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(case, dev):
    """{output name: tensor} of one case through the library's entry points on `dev`."""
    from guassianhand_amd import lpips as LP
    from guassianhand_amd import perceptual as P
    _, kind, prm = case
    if kind == "conv3x3":
        N, H, W, Cin, Cout, relu, ch = prm
        x, w, b, g = (t.to(dev) for t in conv_inputs(N, H, W, Cin, Cout, 3))
        wf, wb = P.pack_weights(w)
        y, gate = P._conv_forward(x, wf, b, Cout, bool(relu), ch)
        out = dict(y=y, dx=P._conv_backward(g, gate, wb, Cin, bool(relu), ch))
        if relu:
            out["gate"] = gate
        return out
    if kind == "conv2d":
        (Cin, Cout, K, s, p, N, H, W), full, ch = prm
        x, w, b, _ = (t.to(dev) for t in conv_inputs(N, H, W, Cin, Cout, K))
        return dict(y=LP.conv2d(x, w, b if full else None, s, p, relu=bool(full), chunk=ch))
    if kind == "pool2x2":
        x, g = (t.to(dev) for t in pool2x2_input(*prm))
        y, choice = P._pool_forward(x)
        return dict(y=y, choice=choice, dx=P._pool_backward(g, choice, x.shape[1], x.shape[2]))
    H, W, Cn = prm
    return dict(y=LP.max_pool3x3s2(pool3x3_input(H, W, Cn).to(dev)))


def hashes(case, dev):
    return {k: sha(v) for k, v in run_case(case, dev).items()}
