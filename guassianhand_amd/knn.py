"""K nearest neighbours and the interaction mask — host side of gh_knn_* (include/gh_raster.h).

Reference call site, infer_one_shot.py:247-250 (knn_points = pytorch3d.ops.knn_points, a third-party dependency that
is not part of the reference tree):

    _, mink_idxs_world, _   = knn_points(pointclouds, pointclouds, K=100)
    _, mink_idxs_texture, _ = knn_points(t_point, t_point, K=100)
    mink_idxs_inter = (mink_idxs_world == mink_idxs_texture).sum(-1) < 10
    mink_idxs_inter = mink_idxs_inter.unsqueeze(-1)

`knn_points(p, p, K)` mirrors the reference call for the self-query case and returns the same 3-tuple shape
(dists (B,N,K), idx (B,N,K) int64, None); `interaction_mask` is the whole four-line block. ROCm tensors only: the
kernels raise if the library is missing and there is no CPU path.

Where "exact" holds. The index lists and squared distances are bit-equal to a brute-force float32 computation (ties by ascending
index) whenever the squared distance between any two DISTINCT points is a normal float32 number, i.e. no two distinct points are
closer than about 1e-19 (sqrt(FLT_MIN)); identical points are always exact, at any number of copies. Hands are in metres, so every
real cloud is inside this domain by some fifteen orders of magnitude. Below it (a cloud so small that squared distances underflow
to 0) the lists are still in range and unique per row, but they are not the brute-force lists, which order the tied zeros by
index: the query kernel's stop rule compares the K-th squared distance with ((r - 0.001) * h)^2, which underflows
with it, so `0 <= 0` ends the walk as soon as K candidates exist, before the cells holding the lowest indices are visited. The fix is
two lines in gh_knn_query_kernel, recorded here for the next change that touches csrc/: never stop at r = 0 unless h = 0, and for
r > 0 stop only when rg * rg >= FLT_MIN. Non-finite points are contained: the walk is bounded by the grid, a NaN or infinite point
never enters the list of a finite point while K finite points exist, and its own row holds in-range indices.
tests/test_gpu_knn_edges.py checks all of this (scalings by 2^+-40 inside the domain, 2^-100 below it).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._call import launch, lib, ptr


def _check(points: torch.Tensor) -> torch.Tensor:
    if not points.is_cuda:
        raise RuntimeError("gh_knn_* runs on a ROCm device only (there is no CPU path)")
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("points must be (B, N, 3)")
    return points.detach().float().contiguous()


def knn_indices(points: torch.Tensor, K: int, return_dists: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """points (B,N,3) -> idx (B,N,K) int32 sorted by (squared distance, index) [, dists (B,N,K)]."""
    p = _check(points)
    B, N, _ = p.shape
    idx = torch.empty(B, N, K, dtype=torch.int32, device=p.device)
    dists = torch.empty(B, N, K, dtype=torch.float32, device=p.device) if return_dists else None
    nbytes = int(lib().gh_knn_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    for b in range(B):
        launch("gh_knn_indices", p.device, ptr(p[b]), N, K, ptr(idx[b]), ptr(dists[b]) if return_dists else None, ptr(ws), nbytes,
               detail=f" (N={N}, K={K})")
    return idx, dists


def knn_points(p1: torch.Tensor, p2: torch.Tensor, K: int = 1):
    """Drop-in for the reference's two calls (self-query): returns (dists, idx int64, None) like pytorch3d's _KNN."""
    if p1 is not p2 and (p1.shape != p2.shape or p1.data_ptr() != p2.data_ptr()):
        raise NotImplementedError("only the self-query form knn_points(p, p, K) of infer_one_shot.py:247-248 is provided")
    idx, d = knn_indices(p1, K, return_dists=True)
    return d, idx.long(), None


def interaction_mask(pointclouds: torch.Tensor, t_point: torch.Tensor, K: int = 100, min_same: int = 10) -> torch.Tensor:
    """(B,N,3) posed points, (B,N,3) template-pose points -> (B,N,1) bool, True where fewer than `min_same` of the K
    sorted neighbour ranks agree (infer_one_shot.py:247-250)."""
    a, _ = knn_indices(pointclouds, K)
    b, _ = knn_indices(t_point, K)
    B, N, _ = a.shape
    mask = torch.empty(B, N, dtype=torch.uint8, device=a.device)
    for i in range(B):
        launch("gh_knn_mismatch_mask", a.device, ptr(a[i]), ptr(b[i]), N, K, min_same, ptr(mask[i]))
    return mask.bool().unsqueeze(-1)
