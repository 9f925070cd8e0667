"""Per-cell pooling of point features: the work the reference's LocalPoolPointnet (tgs/models/pointclouds/pointnet_texture.py)
hands to torch_scatter, on the device through include/gh_pool.h.

Every point carries a UV-cell index that is fixed for a whole encoder forward. `PoolPlan(index, n_cells)` groups the points by
cell once (a counting sort); the five calls of a forward then reduce over contiguous runs of that order:

    pool_local(x, plan, reduce)   (T,C) -> (T,C): every point receives its cell's per-channel max / mean (pool_local, :68-81)
    pool_cat(net, plan, reduce)   (T,C) -> (T,2C): torch.cat([net, pool_local(net)], dim=1) with the pooled half written in place (:107)
    plane_mean(c, plan)           (T,C) -> (C, n_cells): the mean per cell, 0 for empty cells (generate_plane_features, :55-66)

Ties of a maximum go to the lowest point index, in the value's argmax and in the gradient (torch_scatter leaves them to a race on
the GPU). A NaN never wins a maximum, wherever it sits in its cell; a cell whose rows are all NaN in a channel behaves like an
empty cell for that channel (value 0, argmax T, gradient nowhere). -inf is an ordinary value: a cell that is all -inf returns -inf
with its first point as argmax. Means propagate NaN and infinities as arithmetic does. Sums have a fixed order, so values and
gradients are bitwise reproducible. A point whose index is outside [0, n_cells)
is skipped — it contributes nothing and receives zeros — and `PoolPlan.check()` raises for it on request (the reference asserts
with a host synchronisation on every forward).

CPU tensors go through `_pool_local_ref` / `_plane_mean_ref`, a plain-torch restatement with the same tie rule, no atomics and
float64 accumulation on request (the yardstick of the GPU tests; `ops="torch"` runs it on any device). ROCm tensors go through the
HIP kernels only. `scatter_max` / `scatter_mean` carry torch_scatter's signatures for the call forms the reference makes;
`LocalPoolPointnet` is the encoder itself with the reference's state-dict keys, `fused_pointnet_cls(base)` the same forward grafted
on the reference's own class for the `pointcloud_encoder_*_cls` config lines."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import _abi, _seam
from ._call import check_ops, launch, lib, ptr, row_stride, rows, workspace
from .cond import PointRows

_REDUCE = {"max": _abi.GH_POOL_MAX, "mean": _abi.GH_POOL_MEAN}


def _features(t: torch.Tensor, name: str) -> torch.Tensor:
    """A (T,C) float32 tensor, as the kernels can read it in place (_call.rows)."""
    if t.dim() != 2:
        raise ValueError(f"{name}: expected (T, C), got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return rows(t)


class PoolPlan:
    """The points of one cloud grouped by cell: `cell_start` (n_cells+1,) int32 and `order` (T,) int32, the points of cell c
    being order[cell_start[c]:cell_start[c+1]] in ascending point index; points with an index outside [0, n_cells) follow the
    last cell. Built once per encoder forward; never synchronises on a ROCm device (graph capturable)."""

    def __init__(self, index: torch.Tensor, n_cells: int):
        index = index.detach().reshape(-1)
        if index.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"index: expected int32 or int64, got {index.dtype}")
        self.T, self.n_cells, self.device = int(index.shape[0]), int(n_cells), index.device
        if self.T < 1 or self.n_cells < 1:
            raise ValueError(f"PoolPlan needs at least one point and one cell, got T={self.T}, n_cells={self.n_cells}")
        self.index = index.contiguous()
        if not index.is_cuda:
            idx = self.index.long()
            bad = (idx < 0) | (idx >= self.n_cells)
            key = torch.where(bad, torch.full_like(idx, self.n_cells), idx)
            self.order = torch.argsort(key, stable=True).to(torch.int32)
            counts = torch.bincount(key, minlength=self.n_cells + 1)
            self.cell_start = torch.cat([counts.new_zeros(1), counts.cumsum(0)])[:self.n_cells + 1].to(torch.int32)
            self.flag = bad.any().to(torch.int32).reshape(1)
            return
        dev = self.device
        self.cell_start = torch.empty(self.n_cells + 1, dtype=torch.int32, device=dev)
        self.order = torch.empty(self.T, dtype=torch.int32, device=dev)
        self.flag = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = int(lib().gh_pool_plan_workspace(self.T, self.n_cells))
        ws = workspace(nbytes, dev)
        launch("gh_pool_plan", dev, ptr(self.index), int(index.dtype == torch.int64), self.T, self.n_cells, ptr(self.cell_start),
               ptr(self.order), ptr(self.flag), ptr(ws), nbytes, what=f"gh_pool_plan (T={self.T}, n_cells={self.n_cells})")

    def check(self) -> None:
        """Raise if some point's index was outside [0, n_cells) (one device-to-host copy; the reference's assert)."""
        if int(self.flag.item()) != 0:
            raise IndexError(f"PoolPlan: a cell index is outside [0, {self.n_cells}); such points are skipped by every pooling call")

    def counts(self) -> torch.Tensor:
        return (self.cell_start[1:] - self.cell_start[:-1])

    def _fits(self, x: torch.Tensor, name: str) -> None:
        if x.shape[0] != self.T:
            raise ValueError(f"{name}: {x.shape[0]} rows, the plan has {self.T} points")
        if x.device != self.device:
            raise ValueError(f"{name} is on {x.device}, the plan on {self.device}")


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def _valid(plan: PoolPlan):
    """(idx int64 with skipped points clamped to cell 0, mask of the points that have a cell or None when all have one)"""
    idx = plan.index.long()
    ok = (idx >= 0) & (idx < plan.n_cells)
    if bool(ok.all()):
        return idx, None
    return torch.where(ok, idx, torch.zeros_like(idx)), ok


def _cell_sums(x: torch.Tensor, idx: torch.Tensor, ok, n_cells: int) -> torch.Tensor:
    src = x if ok is None else torch.where(ok.unsqueeze(1), x, torch.zeros_like(x))      # not x * ok: a skipped NaN stays unseen
    return x.new_zeros(n_cells, x.shape[1]).index_add(0, idx, src)


def _cell_max(x: torch.Tensor, plan: PoolPlan):
    """(values (n_cells,C) with 0 for empty cells — differentiable, the gradient goes to the argmax row only —,
    argmax (n_cells,C) int64: the lowest point index attaining the maximum, T for empty cells). A NaN never wins; a cell of
    NaNs alone is empty for that channel (gh_pool.h)."""
    T, Cc = x.shape
    idx, ok = _valid(plan)
    xd = x.detach()
    seen = ~torch.isnan(xd) if ok is None else ~torch.isnan(xd) & ok.unsqueeze(1)
    xd = torch.where(seen, xd, torch.full_like(xd, float("-inf")))
    col = idx.unsqueeze(1).expand(T, Cc)
    amax = torch.full((plan.n_cells, Cc), float("-inf"), dtype=x.dtype, device=x.device).scatter_reduce(0, col, xd, "amax", include_self=True)
    pts = torch.arange(T, device=x.device).unsqueeze(1).expand(T, Cc)
    hit = (xd == amax[idx]) & seen                 # a cell that is all -inf ties at -inf: its first point
    cand = torch.where(hit, pts, torch.full_like(pts, T))
    arg = torch.full((plan.n_cells, Cc), T, dtype=torch.int64, device=x.device).scatter_reduce(0, col, cand, "amin", include_self=True)
    empty = arg == T
    vals = x.gather(0, arg.clamp(max=T - 1))
    return torch.where(empty, torch.zeros_like(vals), vals), arg


def _pool_local_ref(x: torch.Tensor, plan: PoolPlan, reduce: str = "max", acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """pool_local in plain torch, differentiable. acc=torch.float64 computes (and returns) in double."""
    if acc is not None:
        x = x.to(acc)
    idx, ok = _valid(plan)
    if reduce == "max":
        cells, _ = _cell_max(x, plan)
    elif reduce == "mean":
        cnt = plan.counts().to(x.dtype).clamp(min=1).unsqueeze(1)
        cells = _cell_sums(x, idx, ok, plan.n_cells) / cnt
    else:
        raise ValueError(f"reduce must be 'max' or 'mean', got {reduce!r}")
    out = cells.index_select(0, idx)
    return out if ok is None else torch.where(ok.unsqueeze(1), out, torch.zeros_like(out))


def _plane_mean_ref(c: torch.Tensor, plan: PoolPlan, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    if acc is not None:
        c = c.to(acc)
    idx, ok = _valid(plan)
    cnt = plan.counts().to(c.dtype).clamp(min=1).unsqueeze(1)
    return (_cell_sums(c, idx, ok, plan.n_cells) / cnt).t()


# ---- device path ---------------------------------------------------------------------------------------------------------------
def _launch_pool_forward(x, plan, reduce, out, out_col, argmax):
    T, Cc = x.shape
    launch("gh_pool_forward", x.device, ptr(x), row_stride(x), T, Cc, plan.n_cells, ptr(plan.cell_start), ptr(plan.order),
           _REDUCE[reduce], ptr(out), row_stride(out), out_col, ptr(argmax))


def _launch_pool_backward(g, g_col, Cc, plan, reduce, argmax, gx, accumulate):
    launch("gh_pool_backward", g.device, ptr(g), row_stride(g), g_col, g.shape[0], Cc, plan.n_cells, ptr(plan.cell_start),
           ptr(plan.order), _REDUCE[reduce], ptr(argmax), ptr(gx), row_stride(gx), int(accumulate))


class _PoolLocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan, reduce):
        x = _features(x.detach(), "x")
        T, Cc = x.shape
        out = torch.empty(T, Cc, dtype=torch.float32, device=x.device)
        argmax = torch.empty(plan.n_cells, Cc, dtype=torch.int32, device=x.device) if reduce == "max" else None
        _launch_pool_forward(x, plan, reduce, out, 0, argmax)
        ctx.plan, ctx.reduce, ctx.argmax = plan, reduce, argmax
        return out

    @staticmethod
    def backward(ctx, g):
        g = _features(g, "grad")
        gx = torch.empty(g.shape, dtype=torch.float32, device=g.device)
        _launch_pool_backward(g, 0, g.shape[1], ctx.plan, ctx.reduce, ctx.argmax, gx, False)
        return gx, None, None


class _PoolCatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, plan, reduce):
        net = _features(net.detach(), "net")
        T, Cc = net.shape
        cat = torch.empty(T, 2 * Cc, dtype=torch.float32, device=net.device)
        cat[:, :Cc].copy_(net)
        argmax = torch.empty(plan.n_cells, Cc, dtype=torch.int32, device=net.device) if reduce == "max" else None
        _launch_pool_forward(cat[:, :Cc], plan, reduce, cat[:, Cc:], 0, argmax)      # reads the left half, writes the right half
        ctx.plan, ctx.reduce, ctx.argmax, ctx.C = plan, reduce, argmax, Cc
        return cat

    @staticmethod
    def backward(ctx, g):
        g = _features(g, "grad")
        Cc = ctx.C
        gx = g[:, :Cc].clone(memory_format=torch.contiguous_format)       # the left half's gradient; the pooled half's is added into it
        _launch_pool_backward(g, Cc, Cc, ctx.plan, ctx.reduce, ctx.argmax, gx, True)
        return gx, None, None


class _PlaneMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, plan):
        c = _features(c.detach(), "c")
        T, Cc = c.shape
        plane = torch.empty(Cc, plan.n_cells, dtype=torch.float32, device=c.device)
        launch("gh_plane_mean_forward", c.device, ptr(c), row_stride(c), T, Cc, plan.n_cells, ptr(plan.cell_start), ptr(plan.order),
               ptr(plane))
        ctx.plan, ctx.T = plan, T
        return plane

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        Cc, plan = g.shape[0], ctx.plan
        gx = torch.empty(ctx.T, Cc, dtype=torch.float32, device=g.device)
        launch("gh_plane_mean_backward", g.device, ptr(g), ctx.T, Cc, plan.n_cells, ptr(plan.cell_start), ptr(plan.order), ptr(gx), Cc)
        return gx, None


def _check_reduce(reduce: str) -> None:
    if reduce not in _REDUCE:
        raise ValueError(f"reduce must be 'max' or 'mean', got {reduce!r}")


def pool_local(x: torch.Tensor, plan: PoolPlan, reduce: str = "max", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (T,C) float32 -> (T,C): every point's row is its cell's per-channel max / mean. `out`: a (T,C) float32 view with unit
    column stride to write instead of a new tensor, e.g. the right half of a (T,2C) buffer whose left half is x; that form is
    not differentiable (pool_cat is the differentiable cat-buffer form)."""
    _check_reduce(reduce)
    plan._fits(x, "x")
    if out is not None:
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("pool_local(out=...) records no gradient: use pool_cat(net, plan) for the cat buffer, or detach x")
        if tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32 or out.device != x.device or (x.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError("out must be a float32 (T, C) view of x's shape and device with unit column stride")
        if not x.is_cuda:
            out.copy_(_pool_local_ref(x.detach(), plan, reduce))
            return out
        xr = _features(x.detach(), "x")
        argmax = torch.empty(plan.n_cells, x.shape[1], dtype=torch.int32, device=x.device) if reduce == "max" else None
        _launch_pool_forward(xr, plan, reduce, out, 0, argmax)
        return out
    if not x.is_cuda:
        return _pool_local_ref(x, plan, reduce)
    return _PoolLocalFn.apply(x, plan, reduce)


def pool_cat(net: torch.Tensor, plan: PoolPlan, reduce: str = "max") -> torch.Tensor:
    """torch.cat([net, pool_local(net, plan, reduce)], dim=1) as one (T,2C) buffer: the pooled values are written where the next
    layer reads them, and the backward adds the pooled half's gradient into the left half's in one pass."""
    _check_reduce(reduce)
    plan._fits(net, "net")
    if not net.is_cuda:
        return torch.cat([net, _pool_local_ref(net, plan, reduce)], dim=1)
    return _PoolCatFn.apply(net, plan, reduce)


def plane_mean(c: torch.Tensor, plan: PoolPlan) -> torch.Tensor:
    """c (T,C) float32 -> (C, n_cells): the mean of each cell's rows, 0 for empty cells, channel-first."""
    plan._fits(c, "c")
    if not c.is_cuda:
        return _plane_mean_ref(c, plan)
    return _PlaneMeanFn.apply(c, plan)


def pool_argmax(x: torch.Tensor, plan: PoolPlan) -> torch.Tensor:
    """(n_cells, C) int64: per cell and channel the lowest point index attaining the maximum, T for empty cells."""
    plan._fits(x, "x")
    if not x.is_cuda:
        return _cell_max(x.detach(), plan)[1]
    xr = _features(x.detach(), "x")
    out = torch.empty_like(xr, memory_format=torch.contiguous_format)
    argmax = torch.empty(plan.n_cells, x.shape[1], dtype=torch.int32, device=x.device)
    _launch_pool_forward(xr, plan, "max", out, 0, argmax)
    return argmax.long()


# ---- torch_scatter's two functions, for the call forms the reference makes ---------------------------------------------------------
def _scatter_args(src, index, dim, out, dim_size, name):
    if src.dim() != 3 or index.dim() != 3 or index.shape[1] != 1 or index.shape[0] != src.shape[0] or index.shape[2] != src.shape[2]:
        raise NotImplementedError(f"{name}: only src (B,C,T) with index (B,1,T) is provided (pointnet_texture.py:63,75), got "
                                  f"src {tuple(src.shape)}, index {tuple(index.shape)}")
    if dim not in (-1, 2):
        raise NotImplementedError(f"{name}: only the last dimension is provided, got dim={dim}")
    if out is not None:
        if out.dim() != 3 or out.shape[:2] != src.shape[:2]:
            raise NotImplementedError(f"{name}: out must be (B,C,n_cells), got {tuple(out.shape)}")
        return int(out.shape[2])
    if dim_size is None:
        raise NotImplementedError(f"{name}: give dim_size= or out= (sizing the output by index.max() needs a host synchronisation)")
    return int(dim_size)


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    """torch_scatter.scatter_max for src (B,C,T), index (B,1,T) along the last dim with dim_size= : returns (out (B,C,dim_size),
    argmax (B,C,dim_size) int64), 0 and T for empty cells; ties go to the lowest point index."""
    n = _scatter_args(src, index, dim, out, dim_size, "scatter_max")
    if out is not None:
        raise NotImplementedError("scatter_max: out= is not provided (the reference passes dim_size=, pointnet_texture.py:75)")
    vals, args = [], []
    for b in range(src.shape[0]):
        x = src[b].t()
        plan = PoolPlan(index[b, 0], n)
        if x.is_cuda:
            arg = pool_argmax(x, plan)
            T = x.shape[0]
            v = x.gather(0, arg.clamp(max=T - 1))
            v = torch.where(arg == T, torch.zeros_like(v), v)
        else:
            v, arg = _cell_max(x, plan)
        vals.append(v.t())
        args.append(arg.t())
    return torch.stack(vals), torch.stack(args)


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    """torch_scatter.scatter_mean for src (B,C,T), index (B,1,T) along the last dim with dim_size= or out=. With out= the means
    are added into it and it is returned (the reference hands in zeros, pointnet_texture.py:61-63)."""
    n = _scatter_args(src, index, dim, out, dim_size, "scatter_mean")
    res = torch.stack([plane_mean(src[b].t(), PoolPlan(index[b, 0], n)) for b in range(src.shape[0])])
    if out is None:
        return res
    out.add_(res)
    return out


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------
class ResnetBlockFC(nn.Module):
    """Fully connected ResNet block with the reference's parameter names (tgs/models/networks.py:162-204): fc_0, fc_1, shortcut."""

    def __init__(self, size_in: int, size_out: Optional[int] = None, size_h: Optional[int] = None):
        super().__init__()
        size_out = size_in if size_out is None else size_out
        size_h = min(size_in, size_out) if size_h is None else size_h
        self.fc_0 = nn.Linear(size_in, size_h)
        self.fc_1 = nn.Linear(size_h, size_out)
        self.shortcut = None if size_in == size_out else nn.Linear(size_in, size_out, bias=False)
        nn.init.zeros_(self.fc_1.weight)

    def forward(self, x):
        net = self.fc_0(torch.relu(x))
        dx = self.fc_1(torch.relu(net))
        return (x if self.shortcut is None else self.shortcut(x)) + dx


def cell_index(p: torch.Tensor, radius: float, plane_size: int) -> torch.Tensor:
    """(B,T,D) points -> (B,T) int64 UV-cell index, the reference's arithmetic step for step (pointnet_texture.py:83-100 and
    scale_tensor): clamp the first two columns to +-(radius - 1e-6), scale to [0, 1), x + plane_size * y."""
    pos = torch.clamp(p[..., :2], -radius + 1e-6, radius - 1e-6)
    pos = (pos - (-radius)) / (radius - (-radius))
    pos = pos * (1 - 0) + 0
    xi = (pos * plane_size).long()
    return xi[..., 0] + plane_size * xi[..., 1]


def pointnet_forward(self, p, ops: Optional[str] = None, blocks: Optional[str] = None) -> torch.Tensor:
    """LocalPoolPointnet.forward(p) (pointnet_texture.py:89-114) over one PoolPlan per cloud: (B,T,D) -> (B, c_dim, plane, plane).
    Reads self.cfg.{radius, plane_size, scatter_type}, self.fc_pos, self.blocks, self.fc_c. ops="torch" runs the plain-torch
    restatement of the pooling on p's device instead of the kernels. A list in self.pool_record receives every pooled tensor.
    `p` may be a cond.PointRows standing for the (B,T,D) concatenation: the cell index then comes from its uv columns and the first
    layer from PointRows.linear(self.fc_pos); the concatenation is not built.
    blocks (or self.block_ops) = "folded" runs the ResNet blocks with the pooled half folded per cell and fc_c over the per-cell
    means (res_block.folded_cloud): the (T,2H) cat buffers and the (T,c_dim) tensor are not built, and self.pool_record then
    receives the pooled cell rows (n_cells, H) of every block instead of the (T,H) tensors. None or "torch": the statements below."""
    ops = ops or getattr(self, "pool_ops", "fused")
    check_ops(ops)
    blocks = blocks or getattr(self, "block_ops", None) or "torch"
    if blocks not in ("torch", "folded"):
        raise ValueError(f"blocks must be None, 'torch' or 'folded', got {blocks!r}")
    given = isinstance(p, PointRows)
    if not given and p.dim() != 3:
        raise ValueError(f"p: expected (B, T, D), got {tuple(p.shape)}")
    cfg = self.cfg
    reduce, ps = str(cfg.scatter_type), int(cfg.plane_size)
    _check_reduce(reduce)
    record = getattr(self, "pool_record", None)
    if given:
        n_clouds = p.B
        index = cell_index(p.uv_columns(), float(cfg.radius), ps)
        first = p.linear(self.fc_pos, ops)
    else:
        n_clouds = p.shape[0]
        index = cell_index(p, float(cfg.radius), ps)
        first = self.fc_pos(p)
    if blocks == "folded":
        from .res_block import folded_cloud
        fea = torch.stack([folded_cloud(self, first[b], PoolPlan(index[b], ps * ps), reduce, ops, record) for b in range(n_clouds)])
        return fea.reshape(n_clouds, fea.shape[1], ps, ps)
    net = self.blocks[0](first)
    planes = []
    for b in range(n_clouds):
        plan = PoolPlan(index[b], ps * ps)
        nb = net[b]
        for block in self.blocks[1:]:
            if ops == "fused":
                cat = pool_cat(nb, plan, reduce)
            else:
                cat = torch.cat([nb, _pool_local_ref(nb, plan, reduce)], dim=1)
            if record is not None:
                record.append(cat[:, nb.shape[1]:].detach())
            nb = block(cat)
        c = self.fc_c(nb)
        planes.append(plane_mean(c, plan) if ops == "fused" else _plane_mean_ref(c, plan))
    fea = torch.stack(planes)
    return fea.reshape(n_clouds, fea.shape[1], ps, ps)


class LocalPoolPointnet(nn.Module):
    """The reference's point encoder (both `pointcloud_encoder_texture_cls` and `pointcloud_encoder_shade_cls` of every shipped
    config) with its state-dict keys — fc_pos, blocks.N.{fc_0, fc_1, shortcut}, fc_c — so a reference checkpoint loads unchanged.
    Takes the reference's config mapping (`LocalPoolPointnet({"input_channels": 53, ...})`) or keywords. blocks="folded" selects
    the folded ResNet blocks (pointnet_forward)."""

    DEFAULTS = dict(input_channels=3, c_dim=128, hidden_dim=128, scatter_type="max", plane_size=32, n_blocks=5, radius=1.0)

    def __init__(self, cfg=None, ops: str = "fused", blocks: Optional[str] = None, **kw):
        super().__init__()
        given = dict(cfg or {})
        given.update(kw)
        given.pop("weights", None)
        given.pop("freeze", None)
        unknown = set(given) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"LocalPoolPointnet: unknown config keys {sorted(unknown)}")
        self.cfg = SimpleNamespace(**{**self.DEFAULTS, **given})
        if self.cfg.scatter_type not in _REDUCE:
            raise ValueError("incorrect scatter type")
        h = int(self.cfg.hidden_dim)
        self.fc_pos = nn.Linear(int(self.cfg.input_channels), 2 * h)
        self.blocks = nn.ModuleList([ResnetBlockFC(2 * h, h) for _ in range(int(self.cfg.n_blocks))])
        self.fc_c = nn.Linear(h, int(self.cfg.c_dim))
        self.pool_ops = ops
        self.block_ops = blocks          # None / "torch": the reference's statements; "folded": res_block (pointnet_forward)
        self.pool_record = None

    def forward(self, p: torch.Tensor) -> torch.Tensor:
        return pointnet_forward(self, p)


def fused_pointnet_cls(base):
    """For the `pointcloud_encoder_texture_cls` / `pointcloud_encoder_shade_cls` config lines, as renderer.fused_renderer_cls is for
    `renderer_cls`: a subclass of the reference's LocalPoolPointnet whose forward is pointnet_forward; configure(), the
    parameters and the config handling stay the base class's. `guassianhand_amd.tgs_pointnet.LocalPoolPointnet` is this class
    over tgs.models.pointclouds.pointnet_texture.LocalPoolPointnet (importing the base needs a module named torch_scatter:
    INTEGRATION.md)."""
    return _seam.graft((__name__, "fused_pointnet_cls"), base, {"forward": lambda self, p: pointnet_forward(self, p)}, "pooling")
