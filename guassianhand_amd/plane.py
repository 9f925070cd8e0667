"""The plane fetch: the reference's `query_triplane_texture` (tgs/models/renderer_one_shot.py:420-446) — F.grid_sample(bilinear,
align_corners=True, zeros padding) of a channel-first feature plane at every point's UV — on the device through include/gh_plane.h.

    plane_sample(planes, uv, *, index=None, ops="fused")   planes (B,C,Hp,Wp) or (B,1,C,Hp,Wp), uv (B,N,2) in [-1,1] -> (B,N,C)

The call is differentiable with respect to `planes`, which stay in the reference's layout. The forward transposes the plane into a
channel-last scratch copy and gathers from it (the arithmetic of uvmap.uv_sample, bit for bit). The backward needs, per texel, the
list of (point, corner) pairs that touch it: `PlaneIndex(uv, Hp, Wp)` builds those lists on the device (one small kernel and the
pooling block's counting sort; no host read-back, graph capturable) and the gradient of every texel is then one chain of additions
over its list in ascending pair order. No float atomics: the gradient is bitwise reproducible, and equal bit for bit to
uvmap.uv_sample's backward over its host-built lists.

The index depends on the UVs alone. `plane_sample` keeps the last four it built, keyed on the identity and version of the `uv`
tensor it was given; a caller whose UV tensor is a new object every step but whose values are not passes `index=` (a PlaneIndex, or
one per batch element).

The plain-torch restatement (`_plane_sample_ref`: the reference's own statements, float64 on request) is taken for CPU tensors, for
`ops="torch"`, when `uv.requires_grad` (torch differentiates with respect to the grid, this block does not) and when `planes`
needs a gradient on a plane of more than GH_POOL_MAX_CELLS texels (the counting sort's limit). ROCm tensors otherwise go through the
HIP kernels only.

`query_triplane_texture(self, positions, triplanes)` is the reference's method over `plane_sample`; `fuse_plane_fetch(renderer)`
binds it on an instance — what `guassianhand_amd.tgs_renderer.GS3DRendererFusedFetch` / `...FusedAllFetch` do in `configure()`."""
from __future__ import annotations

import types
import weakref
from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi
from ._call import check_ops, launch, lib, ptr, workspace

MAX_TEXELS = _abi.GH_POOL_MAX_CELLS


def _points(uv: torch.Tensor, name: str = "uv") -> torch.Tensor:
    if uv.dim() != 2 or uv.shape[1] != 2:
        raise ValueError(f"{name}: expected (N, 2), got {tuple(uv.shape)}")
    if uv.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {uv.dtype}")
    return uv.detach().contiguous()


class PlaneIndex:
    """The (point, corner) pairs of N UVs grouped by the texel of an (Hp, Wp) map they touch: `texel_start` (Hp*Wp + 1,) int32,
    `pairs` (4N,) int32 and `w` (4N,) float32. Pair e = 4 * n + corner (nw, ne, sw, se) weighs w[e]; the pairs of texel t = y * Wp + x
    are pairs[texel_start[t]:texel_start[t + 1]] in ascending e; pairs whose corner lies outside the map follow the last texel and are
    read by nothing. Built on uv's device without a read-back; Hp * Wp <= GH_POOL_MAX_CELLS. CPU tensors get the same lists from
    plain torch (`index_contract`)."""

    def __init__(self, uv: torch.Tensor, Hp: int, Wp: int):
        uv = _points(uv)
        self.N, self.Hp, self.Wp, self.device = int(uv.shape[0]), int(Hp), int(Wp), uv.device
        if self.Hp < 1 or self.Wp < 1:
            raise ValueError(f"PlaneIndex needs a map of at least 1 x 1, got {Hp} x {Wp}")
        if self.Hp * self.Wp > MAX_TEXELS:
            raise ValueError(f"PlaneIndex: {Hp} x {Wp} is more than {MAX_TEXELS} texels, the limit of the counting sort")
        if not uv.is_cuda:
            self.texel_start, self.pairs, self.w = index_contract(uv, self.Hp, self.Wp)
            self.workspace = None
            return
        dev, n4 = self.device, 4 * self.N
        self.texel_start = torch.empty(self.Hp * self.Wp + 1, dtype=torch.int32, device=dev)
        self.pairs = torch.empty(n4, dtype=torch.int32, device=dev)
        self.w = torch.empty(n4, dtype=torch.float32, device=dev)
        nbytes = int(lib().gh_plane_workspace(self.N, 1, self.Hp, self.Wp))
        self.workspace = workspace(nbytes, dev)
        launch("gh_plane_index", dev, ptr(uv), self.N, self.Hp, self.Wp, ptr(self.texel_start), ptr(self.pairs), ptr(self.w),
               ptr(self.workspace), nbytes, what=f"gh_plane_index (N={self.N}, {self.Hp} x {self.Wp})")

    def _fits(self, N: int, Hp: int, Wp: int, dev) -> None:
        if (self.N, self.Hp, self.Wp) != (N, Hp, Wp):
            raise ValueError(f"index: built for N={self.N} on {self.Hp} x {self.Wp}, the call has N={N} on {Hp} x {Wp}")
        if self.device != dev:
            raise ValueError(f"index is on {self.device}, the plane on {dev}")


def index_contract(uv: torch.Tensor, Hp: int, Wp: int):
    """The index in plain torch: (texel_start, pairs, w) as PlaneIndex holds them, `pairs` cut after the last texel's list (the
    pairs without a texel are absent). The float32 arithmetic of gh_bilinear, statement for statement."""
    uv = uv.detach().float()
    ix = ((uv[:, 0] + 1.0) * 0.5) * float(Wp - 1)
    iy = ((uv[:, 1] + 1.0) * 0.5) * float(Hp - 1)
    fx, fy = torch.floor(ix), torch.floor(iy)
    x0, y0 = fx.long(), fy.long()
    wx1, wy1 = ix - fx, iy - fy
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    xs = torch.stack([x0, x0 + 1, x0, x0 + 1], 1).reshape(-1)
    ys = torch.stack([y0, y0, y0 + 1, y0 + 1], 1).reshape(-1)
    w = torch.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], 1).reshape(-1).contiguous()
    inside = (xs >= 0) & (xs < Wp) & (ys >= 0) & (ys < Hp)
    e = torch.nonzero(inside).reshape(-1)
    texel = (ys * Wp + xs)[e]
    order = torch.sort(texel, stable=True).indices
    counts = torch.bincount(texel, minlength=Hp * Wp)
    texel_start = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
    return texel_start, e[order].to(torch.int32), w


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def _plane_sample_ref(planes: torch.Tensor, uv: torch.Tensor, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """planes (B,C,Hp,Wp), uv (B,N,2) -> (B,N,C): the reference's statements (renderer_one_shot.py:433-442). acc=torch.float64
    computes (and returns) in double."""
    if acc is not None:
        planes, uv = planes.to(acc), uv.to(acc)
    out = F.grid_sample(planes, uv[:, :, None], align_corners=True, mode="bilinear")
    return out.view(*out.shape[:2], -1).permute(0, 2, 1)


# ---- device path ---------------------------------------------------------------------------------------------------------------
class _PlaneSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plane, uv, index):
        plane = plane.detach().contiguous()
        Cc, Hp, Wp = plane.shape
        N, dev = uv.shape[0], plane.device
        out = torch.empty(N, Cc, dtype=torch.float32, device=dev)
        if N > 0:
            nbytes = int(lib().gh_plane_workspace(0, Cc, Hp, Wp))
            ws = workspace(nbytes, dev)
            launch("gh_plane_sample_forward", dev, ptr(plane), ptr(uv), ptr(out), N, Cc, Hp, Wp, ptr(ws), nbytes,
                   what=f"gh_plane_sample_forward (N={N}, C={Cc}, {Hp} x {Wp})")
        ctx.index, ctx.dims = index, (N, Cc, Hp, Wp)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        N, Cc, Hp, Wp = ctx.dims
        ix = ctx.index
        if N == 0:
            return torch.zeros(Cc, Hp, Wp, dtype=torch.float32, device=g.device), None, None
        g = g.float().contiguous()
        grad = torch.empty(Cc, Hp, Wp, dtype=torch.float32, device=g.device)
        launch("gh_plane_sample_backward", g.device, ptr(g), ptr(ix.texel_start), ptr(ix.pairs), ptr(ix.w), ptr(grad), N, Cc, Hp, Wp,
               what=f"gh_plane_sample_backward (N={N}, C={Cc}, {Hp} x {Wp})")
        return grad, None, None


_index_cache = []      # [(weakref to the caller's uv tensor, its version, batch element, Hp, Wp, PlaneIndex)], most recent first


def _index_of(uv: torch.Tensor, b: int, Hp: int, Wp: int) -> PlaneIndex:
    for ref, ver, bb, h, w, ix in _index_cache:
        if ref() is uv and ver == uv._version and (bb, h, w) == (b, Hp, Wp):
            return ix
    ix = PlaneIndex(uv[b], Hp, Wp)
    _index_cache.insert(0, (weakref.ref(uv), uv._version, b, Hp, Wp, ix))
    del _index_cache[4:]
    return ix


def plane_sample(planes: torch.Tensor, uv: torch.Tensor, *, index: Union[None, PlaneIndex, Sequence[PlaneIndex]] = None,
                 ops: str = "fused") -> torch.Tensor:
    """planes (B,C,Hp,Wp) or (B,1,C,Hp,Wp), uv (B,N,2) in [-1,1] and finite, float32 -> (B,N,C): every point's bilinear sample of
    its batch element's plane, zeros outside the map. Differentiable with respect to `planes` (and, through torch, to `uv`).
    index: the PlaneIndex of uv[b] on (Hp, Wp) — one, or a sequence of B — when the caller holds it; otherwise built when `planes`
    needs a gradient and kept for the same `uv` tensor. ops="torch" runs the plain-torch restatement on the tensors' device."""
    check_ops(ops)
    if planes.dim() == 5:
        if planes.shape[1] != 1:
            raise ValueError(f"planes: expected (B, 1, C, Hp, Wp), got {tuple(planes.shape)}")
        planes = planes.squeeze(1)
    if planes.dim() != 4:
        raise ValueError(f"planes: expected (B, C, Hp, Wp) or (B, 1, C, Hp, Wp), got {tuple(planes.shape)}")
    if uv.dim() != 3 or uv.shape[2] != 2 or uv.shape[0] != planes.shape[0]:
        raise ValueError(f"uv: expected ({planes.shape[0]}, N, 2), got {tuple(uv.shape)}")
    if uv.device != planes.device:
        raise ValueError(f"uv is on {uv.device}, planes on {planes.device}")
    B, Cc, Hp, Wp = planes.shape
    N = uv.shape[1]
    if min(Cc, Hp, Wp) < 1:
        raise ValueError(f"planes: every dimension must be at least 1, got {tuple(planes.shape)}")
    grad_on = torch.is_grad_enabled()
    need_grad = grad_on and planes.requires_grad
    if (ops == "torch" or not planes.is_cuda or (grad_on and uv.requires_grad) or (need_grad and Hp * Wp > MAX_TEXELS)):
        return _plane_sample_ref(planes, uv)
    if planes.dtype != torch.float32 or uv.dtype != torch.float32:
        raise TypeError(f"plane_sample takes float32 tensors, got {planes.dtype} and {uv.dtype}")
    if isinstance(index, PlaneIndex):
        index = [index] * B if B == 1 else None
        if index is None:
            raise ValueError(f"index: one PlaneIndex given for a batch of {B}; pass a sequence of {B}")
    if index is not None and len(index) != B:
        raise ValueError(f"index: {len(index)} given for a batch of {B}")
    outs = []
    for b in range(B):
        ub = _points(uv[b])
        ix = None
        if index is not None:
            ix = index[b]
            ix._fits(N, Hp, Wp, planes.device)
        elif need_grad and N > 0:
            ix = _index_of(uv, b, Hp, Wp)
        outs.append(_PlaneSampleFn.apply(planes[b], ub, ix) if need_grad else _PlaneSampleFn.apply(planes[b].detach(), ub, None))
    return outs[0].unsqueeze(0) if B == 1 else torch.stack(outs)


# ---- the reference's method ----------------------------------------------------------------------------------------------------------
def query_triplane_texture(self, positions: torch.Tensor, triplanes: torch.Tensor) -> torch.Tensor:
    """GS3DRenderer.query_triplane_texture (renderer_one_shot.py:420-446) over plane_sample: positions (*B,N,2) within
    +-self.cfg.radius_texture, triplanes (*B,1,Cp,Hp,Wp) -> (*B,N,Cp). The rescale to [-1,1] is scale_tensor's two statements.
    `self.plane_ops` ("fused" | "torch") and `self.plane_index` (a held PlaneIndex, or a sequence of B) are read when present."""
    batched = positions.ndim == 3
    if not batched:
        triplanes = triplanes[None, ...]
        positions = positions[None, ...]
    r = self.cfg.radius_texture
    positions = (positions - (-r)) / (r - (-r))
    positions = positions * (1 - (-1)) + (-1)
    out = plane_sample(triplanes, positions, index=getattr(self, "plane_index", None), ops=getattr(self, "plane_ops", "fused"))
    if not batched:
        out = out.squeeze(0)
    return out


def fuse_plane_fetch(renderer):
    """Bind query_triplane_texture on this renderer instance: `forward`'s texture-code lookup then runs the plane fetch. Nothing
    else of the object changes. Returns the renderer."""
    bound = types.MethodType(query_triplane_texture, renderer)
    object.__setattr__(renderer, "query_triplane_texture", bound)
    return renderer
