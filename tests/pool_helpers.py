"""Shared by tests/test_pool_cpu.py and tests/test_gpu_pool.py: the fixture, and the rounding bound of a float32 sum.

The bound. A float32 sum of n terms, added in any order, lies within gamma_(n-1) * sum|terms| of the exact sum, and
gamma_(n-1) = (n-1) u / (1 - (n-1) u) <= n u for n <= 4096 with u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2). Dividing by the count scales that error and adds one rounding of the quotient, u * |result|. So an
element computed as (sum of n terms) / count is within

    n * u * sum|terms| / count + u * |result|

of the exact value (count = 1 where nothing is divided). `sum|terms| / count` is the same reduction applied to |terms|, so the
tests get it from the float64 restatement run on the absolute values."""
import os

import numpy as np
import torch

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_fixture.npz")


def load_fixture():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def fixture_weights(fx):
    return {k[2:]: v for k, v in fx.items() if k.startswith("w.")}


def fixture_cfg(fx, kind):
    T, D, hid, cdim, plane, blocks = (int(v) for v in fx["dims"])
    return dict(input_channels=D, c_dim=cdim, hidden_dim=hid, scatter_type=kind, plane_size=plane, n_blocks=blocks,
                radius=float(fx["radius"]))


def assert_within(got, exact, bound, what, slack=1.0):
    """|got - exact| <= slack * bound elementwise (exact, bound: float64). Prints the worst ratio before asserting."""
    got, exact, bound = got.detach().double().cpu(), exact.detach().double().cpu(), bound.detach().double().cpu()
    err = (got - exact).abs()
    ratio = (err / (slack * bound).clamp(min=1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max |err| {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    bad = err > slack * bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, worst err / bound {ratio:.3f}"


def mean_pool_bound(absx_pooled64, result64, counts_per_point):
    """pool 'mean' forward / backward: n = the cell's population, terms = the cell's rows."""
    return counts_per_point.double().unsqueeze(1) * U * absx_pooled64 + U * result64.abs()


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()
