"""What tests/test_knn_oracle.py and tests/test_gpu_knn_edges.py share: the dense numpy restatement of the brute-force kNN, the seeded
clouds of the edge sweep and its (N, K) pairs. The chain is numpy_knn (float64 intermediates, lexsort) -> gho_knn (the C oracle, on
the CPU) -> gh_knn_indices (the device), every link bit for bit."""
import functools

import numpy as np
import torch


def numpy_knn(p: np.ndarray, K: int):
    """Dense restatement: squared L2 in float32 accumulated x, y, z with fused multiply-adds, lexsort by (distance, index)."""
    d = p[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)          # differences are exact in f64
    d32 = d.astype(np.float32)                                                        # == the f32 subtraction (correctly rounded)
    acc = (d32[..., 0].astype(np.float64) ** 2).astype(np.float32)                    # dx*dx rounded to f32
    acc = (d32[..., 1].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)   # fma: one rounding (exact in f64)
    acc = (d32[..., 2].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
    idx = np.lexsort((np.broadcast_to(np.arange(p.shape[0]), acc.shape), acc), axis=-1)[:, :K]
    return idx.astype(np.int32), np.take_along_axis(acc, idx, axis=-1)


# (N, K): N = 1, 3, 5 end in a part-filled workgroup of four queries, N <= 15 sorts 3-bit cell keys (two cells per axis), 63 / 64 / 65
# and 127 / 129 sit around one and two waves of candidates, K = 2 .. 128 walks the two 64-entry halves of the candidate list and the
# rank the stop rule reads, K = N below the list's capacity ends with every point visited.
PAIRS = ((1, 1), (2, 1), (2, 2), (3, 2), (5, 5), (8, 8), (9, 3), (16, 16), (27, 27), (63, 63), (64, 64), (65, 64), (65, 65), (127, 127),
         (129, 127), (129, 128), (200, 65), (257, 100), (700, 2), (700, 63), (700, 100))

CLOUDS = ("uniform", "signed", "dyadic", "offset", "plane", "line", "two_clusters", "identical")


def cloud(name: str, N: int, seed: int) -> torch.Tensor:
    """The (N, 3) float32 cloud `name`, drawn from a generator seeded with `seed`."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(N, 3, generator=g)
    if name == "uniform":                      # [0, 1)^3
        return u
    if name == "signed":                       # [-1, 1)^3 with both zeros among the coordinates
        p = u * 2.0 - 1.0
        p[::7, 0] = -0.0
        p[::11, 1] = 0.0
        return p
    if name == "dyadic":                       # multiples of 1/64: every difference and squared distance is exact in float32, ties abound
        return torch.randint(0, 64, (N, 3), generator=g).float() / 64.0
    if name == "offset":                       # far from the origin: the coordinates quantise to 2^-14
        return u * 0.2 + 1000.0
    if name == "plane":
        p = u.clone()
        p[:, 2] = 0.25
        return p
    if name == "line":
        p = torch.zeros(N, 3)
        p[:, 0] = torch.linspace(0, 1, N)
        return p
    if name == "two_clusters":                 # N // 10 points near (100, 0, 0), the rest within 0.01 of the origin on every axis
        p = u * 0.01
        p[:N // 10, 0] += 100.0
        return p
    if name == "identical":
        return torch.full((N, 3), 0.7)
    raise KeyError(name)


def case_cloud(name: str, N: int) -> torch.Tensor:
    """The sweep's cloud for (name, N): one seed per N, the same on the CPU and on the device side."""
    return cloud(name, N, 1000 + N)


@functools.lru_cache(maxsize=None)
def dense_knn(name: str, N: int):
    """numpy_knn of case_cloud(name, N) with K = N (every K of PAIRS is a prefix of it), computed once."""
    return numpy_knn(case_cloud(name, N).numpy(), N)


def float64_knn(p: torch.Tensor, K: int):
    """Stable argsort of the float64 squared distances (sum in float64, no fma modelled): the answer for clouds whose distances are exact."""
    p64 = p.double()
    d = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
    idx = torch.argsort(d, dim=-1, stable=True)[:, :K]
    return idx.to(torch.int32), torch.gather(d, 1, idx)
