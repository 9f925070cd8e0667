"""Shared cases of the LPIPS tests (test_lpips_cpu.py, test_gpu_lpips.py): the convolution, pooling and head shapes, the end-to-end
networks and images, and the guard every head and end-to-end case asserts on its float64 reference before anything is compared.

The guard. LPIPS divides every feature row by its norm, so a pixel whose norm is tiny turns float32 rounding of the features into
an O(1) change of its unit vector, in the kernels and in torch's float32 alike. A case is fit to compare only where, per tap, every
pixel's float64 norm is either exactly 0 or at least 2^-10 of that tap's largest norm (`norm_guard`). The seeds below were picked by
the search under __main__ (python -m tests.lpips_cases), which prints each case's margin; the end-to-end seeds have no all-zero pixel
at all, so that no float64 zero hides a float32 value of the other sign.

The tolerance is res_block_cases.three_way: kernel vs float64 <= 4 x (torch float32 vs float64) + 2^-20 max|float64|."""
import numpy as np
import torch
import torch.nn.functional as F

from guassianhand_amd import lpips as LP

GUARD = 2.0 ** -10

# (Cin, Cout, K, stride, padding, N, H, W)
CONV_CASES = (
    (3, 64, 11, 4, 2, 2, 31, 31),
    (3, 8, 11, 4, 2, 1, 35, 32),      # the stride remainder in both directions
    (64, 192, 5, 1, 2, 2, 7, 9),
    (5, 33, 5, 1, 2, 3, 3, 3),
    (37, 40, 3, 1, 1, 2, 1, 1),       # every tap but the centre is padding
    (192, 384, 3, 1, 1, 1, 3, 5),
    (8, 16, 3, 1, 1, 3, 13, 11),      # 429 pixels: tiles straddle images, the last is partial
)
CHUNKS = (0, 32, 64, 128)
POOL_SHAPES = ((7, 7), (3, 3), (8, 6), (4, 9))
POOL_CHANNELS = (1, 7, 64)
HEAD_CHANNELS = (7, 64, 192, 384)
# (widths, N, H, W, seed): the small network at the smallest image, at the stride remainder and at an odd size; the shipped widths once
SMALL = (8, 40, 33, 16, 7)
E2E_CASES = ((SMALL, 2, 31, 31, 0), (SMALL, 2, 35, 32, 0), (SMALL, 2, 67, 45, 3), (LP.WIDTHS, 2, 64, 64, 0))


def case_id(case):
    return "-".join("x".join(str(v) for v in c) if isinstance(c, tuple) else str(c) for c in case)


def make_conv(case, seed=0):
    """x (N, H, W, Cin), weight (Cout, Cin, K, K) scaled to unit output variance, bias (Cout,), on the CPU in float32."""
    Cin, Cout, K, s, p, N, H, W = case
    g = torch.Generator().manual_seed(7000 + seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (Cin * K * K) ** -0.5
    return x, w, torch.randn(Cout, generator=g)


def make_pool(shape, C, seed=0):
    """(3, H, W, C): image 0 random, image 1 of few distinct values (ties) with a window of -inf, image 2 with NaNs and -inf."""
    H, W = shape
    g = torch.Generator().manual_seed(7100 + seed)
    x = torch.randn(3, H, W, C, generator=g)
    x[1] = torch.randint(0, 3, (H, W, C), generator=g).float()
    x[1, :3, :3] = float("-inf")
    x[2, 1, 1] = float("nan")
    x[2, H - 1, W - 1] = float("nan")
    x[2, 0, 0] = float("-inf")
    return x


def make_head(C, seed=0, N=2, h=5, w=7):
    """f (2N, h, w, C) of ReLU'd normal values and lin (C,) >= 0 with exact zeros; pixel (0, 0) of pair 0 is all zeros in both images,
    pixel (1, 2) of pair 1 in the first image only."""
    g = torch.Generator().manual_seed(7200 + seed)
    f = torch.relu(torch.randn(2 * N, h, w, C, generator=g) + 0.5)
    f[0, 0, 0] = 0.0
    f[N, 0, 0] = 0.0
    f[1, 1, 2] = 0.0
    lin = torch.rand(C, generator=g)
    lin[::3] = 0.0
    return f, lin


def make_images(N, H, W, seed=0):
    """Two (N, 3, H, W) stacks in [-1, 1]: smooth-ish random images and a perturbed copy, so that the distance is neither 0 nor large."""
    g = torch.Generator().manual_seed(7300 + seed)
    x0 = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    x1 = (x0 + 0.5 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    return x0, x1


def quantiser_ties():
    """{k: v}: float32 values v whose float32 product v * 255 is exactly k + 1/2, found by walking the neighbours of (k + 1/2) / 255."""
    found = {}
    for k in range(255):
        v = np.float32((k + 0.5) / 255.0)
        cands = [v]
        for _ in range(4):
            cands = [np.nextafter(cands[0], np.float32(-1)), *cands, np.nextafter(cands[-1], np.float32(2))]
        for c in cands:
            if np.float32(c * np.float32(255.0)) == np.float32(k + 0.5):
                found[k] = float(c)
                break
    return found


def quantiser_values():
    """One float32 vector for the quantiser: every tie, values under 0 and over 1, both infinities, a NaN, and the 8-bit grid."""
    ties = quantiser_ties()
    edge = [-0.3, -1e-9, 0.0, 1.0, 1.0 + 1e-3, 1.7, float("inf"), float("-inf"), float("nan")]
    return torch.cat([torch.tensor([ties[k] for k in sorted(ties)] + edge, dtype=torch.float32), torch.arange(256, dtype=torch.float32) / 255.0])


def make_net(widths, seed=0):
    return LP.AlexLPIPS.synthetic(seed, widths)


def tap_norms(net, x0, x1):
    """The float64 norms of every pixel of the five taps, both images: five (2N, h, w) tensors."""
    dt = torch.float64
    shift, scale = net.shift.to(dt).view(1, 3, 1, 1), net.scale.to(dt).view(1, 3, 1, 1)
    h = torch.cat([(x0.to(dt) - shift) / scale, (x1.to(dt) - shift) / scale])
    out = []
    for (_, K, s, p, pool), conv in zip(LP.CONVS, net.convs()):
        if pool:
            h = F.max_pool2d(h, 3, 2)
        h = torch.relu(F.conv2d(h, conv.weight.to(dt), conv.bias.to(dt), stride=s, padding=p))
        out.append(h.pow(2).sum(dim=1).sqrt())
    return out


def norm_margin(norms):
    """(the smallest non-zero norm over the largest, the number of exactly-zero pixels), the worst tap."""
    worst, zeros = float("inf"), 0
    for n in norms:
        nz = n[n > 0]
        zeros += int((n == 0).sum())
        if nz.numel():
            worst = min(worst, float(nz.min() / n.max()))
    return worst, zeros


def norm_guard(norms, tag=""):
    """The condition on the float64 reference alone: every pixel's norm is exactly 0 or >= 2^-10 of its tap's largest."""
    m, zeros = norm_margin(norms)
    print(f"{tag} norm guard: min non-zero norm / max norm = {m:.3e} ({zeros} all-zero pixels)")
    assert m >= GUARD, (tag, m)


def head_norms(f):
    return [f.double().pow(2).sum(dim=3).sqrt()]


if __name__ == "__main__":                                   # the seed search: prints, per case, the margins of the first seeds
    for C in HEAD_CHANNELS:
        m, z = norm_margin(head_norms(make_head(C)[0]))
        print(f"head C={C}: margin {m:.3e}, {z} zero pixels {'ok' if m >= GUARD else 'TOO CLOSE'}")
    for widths, N, H, W, _ in E2E_CASES:
        for seed in range(4):
            m, z = norm_margin(tap_norms(make_net(widths, seed), *make_images(N, H, W, seed)))
            print(f"e2e {widths} {N}x{H}x{W} seed {seed}: margin {m:.3e}, {z} zero pixels {'ok' if m >= GUARD and z == 0 else 'no'}")
