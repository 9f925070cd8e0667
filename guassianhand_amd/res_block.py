"""The point encoders' ResNet blocks with the pooled half folded per cell, through include/gh_res.h.

LocalPoolPointnet feeds blocks 1.. with torch.cat([net, pooled], dim=1), whose right half repeats one row per cell in every point's
row. With W0 = [W0a | W0b] and Ws = [Wsa | Wsb] split at column H (H the hidden width) and m[c] the cell's pooled row:

    fc_0(relu(cat))[p] = W0a . relu(net[p]) + (W0b . relu(m[c(p)]) + b0)
    shortcut(cat)[p]   = Wsa . net[p]       +  Wsb . m[c(p)]

The bracketed terms are one row per cell: `folded_block` computes them in plain torch over the cell rows (autograd carries their
gradients to m and to the parameters) and `res_rows` does what is left per point:

    h[p]   = u[r(p)] + W0 . relu(x[p])
    out[p] = s[r(p)] + Ws . x[p] + W1 . relu(h[p])

`cell_max` is the per-cell maximum as (n_cells + 1, H) rows — the last row zeros, the row of a point without a cell — and
`plane_linear` the encoder's last two statements with the mean taken first: mean_c(fc_c(net)) = fc_c(mean_c(net)).

`res_rows` runs the HIP row kernels for float32 ROCm tensors with H in {32, 64, 96, 128}, Cin in {H, 2H} and no weight that requires a
gradient; everything else (the CPU, float64, other widths, trainable blocks, ops="torch") runs `_res_rows_ref`, the plain-torch
restatement, which differentiates with respect to everything. The folded algebra is the same either way."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._call import check_ops, launch, ptr, row_stride, rows
from .pool import PoolPlan, _cell_max, _plane_mean_ref, plane_mean

WIDTHS = (32, 64, 96, 128)


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def _res_rows_ref(x, u, s, row_of, W0, Ws, W1, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """res_rows in plain torch, differentiable in everything. acc=torch.float64 computes (and returns) in double."""
    if acc is not None:
        x, u, s, W0, Ws, W1 = (t.to(acc) for t in (x, u, s, W0, Ws, W1))
    if row_of is None:
        ur, sr = u[:1], s[:1]
    else:
        ur, sr = u.index_select(0, row_of.long()), s.index_select(0, row_of.long())
    h = ur + F.linear(torch.relu(x), W0)
    return sr + F.linear(x, Ws) + F.linear(torch.relu(h), W1)


# ---- device path ---------------------------------------------------------------------------------------------------------------
def _cell_sum(x: torch.Tensor, plan: PoolPlan, tail: bool) -> torch.Tensor:
    """(n_cells + tail, C): the fixed-order sum of x's rows per cell; with `tail` the last row sums the points without a cell."""
    x = rows(x)
    y = torch.empty(plan.n_cells + int(tail), x.shape[1], dtype=torch.float32, device=x.device)
    launch("gh_res_cell_sum", x.device, ptr(x), row_stride(x), x.shape[0], x.shape[1], plan.n_cells, ptr(plan.cell_start), ptr(plan.order),
           int(tail), ptr(y))
    return y


def _launch_forward(x, u, s, row_of, W0, Ws, W1):
    """(out (T,H), mask (T,H/32) int32) of gh_res_forward; x, W0, Ws as _call.rows leaves them, u, s, W1 contiguous."""
    T, Cin = x.shape
    H, R = W1.shape[0], u.shape[0]
    out = torch.empty(T, H, dtype=torch.float32, device=x.device)
    mask = torch.empty(T, H // 32, dtype=torch.int32, device=x.device)
    launch("gh_res_forward", x.device, ptr(x), row_stride(x), T, Cin, H, ptr(u), ptr(s), R, ptr(row_of), ptr(W0), row_stride(W0), ptr(Ws),
           row_stride(Ws), ptr(W1), ptr(out), H, ptr(mask), what=f"gh_res_forward (T={T}, Cin={Cin}, H={H}, R={R})")
    return out, mask


def _launch_backward(g, x, mask, W0, Ws, W1, want_dh: bool):
    """(dx (T,Cin), dh (T,H) or None) of gh_res_backward."""
    T, Cin = x.shape
    H = W1.shape[0]
    dx = torch.empty(T, Cin, dtype=torch.float32, device=x.device)
    dh = torch.empty(T, H, dtype=torch.float32, device=x.device) if want_dh else None
    launch("gh_res_backward", x.device, ptr(g), row_stride(g), ptr(x), row_stride(x), T, Cin, H, ptr(mask), ptr(W0), row_stride(W0), ptr(Ws),
           row_stride(Ws), ptr(W1), ptr(dx), Cin, ptr(dh), what=f"gh_res_backward (T={T}, Cin={Cin}, H={H})")
    return dx, dh


def _launch_cell_max(net, plan):
    """(m (n_cells + 1, C) with the last row zeros, argmax (n_cells, C) int32) of gh_res_cell_max."""
    T, Cc = net.shape
    m = torch.empty(plan.n_cells + 1, Cc, dtype=torch.float32, device=net.device)
    m[plan.n_cells].zero_()
    argmax = torch.empty(plan.n_cells, Cc, dtype=torch.int32, device=net.device)
    launch("gh_res_cell_max", net.device, ptr(net), row_stride(net), T, Cc, plan.n_cells, ptr(plan.cell_start), ptr(plan.order), ptr(m),
           ptr(argmax))
    return m, argmax


class _ResRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, s, row_of, plan, W0, Ws, W1):
        x, W0, Ws = rows(x.detach()), rows(W0.detach()), rows(Ws.detach())
        u, s, W1 = u.detach().contiguous(), s.detach().contiguous(), W1.detach().contiguous()
        out, mask = _launch_forward(x, u, s, row_of, W0, Ws, W1)
        ctx.save_for_backward(x, W0, Ws, W1, mask)
        ctx.row_of, ctx.plan, ctx.R = row_of, plan, u.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        x, W0, Ws, W1, mask = ctx.saved_tensors
        need_x, need_u, need_s = ctx.needs_input_grad[:3]
        g = rows(g.float())
        dx, dh = _launch_backward(g, x, mask, W0, Ws, W1, need_u)
        du = ds = None
        if need_u or need_s:
            plan, tail = ctx.plan, True
            if plan is None:           # the rows grouped by table row: the same fixed-order sums
                row_of = ctx.row_of if ctx.row_of is not None else torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
                plan, tail = PoolPlan(row_of, ctx.R), False
            du = _cell_sum(dh, plan, tail) if need_u else None
            ds = _cell_sum(g, plan, tail) if need_s else None
        return dx if need_x else None, du, ds, None, None, None, None, None


def _kernel_ok(x, u, s, row_of, W0, Ws, W1) -> bool:
    every = (x, u, s, W0, Ws, W1)
    H = W1.shape[0]
    return (x.is_cuda and all(t.dtype == torch.float32 and t.device == x.device for t in every) and H in WIDTHS
            and x.shape[1] in (H, 2 * H) and x.shape[0] >= 1
            and (row_of is None or (row_of.dtype == torch.int32 and row_of.device == x.device))
            and not (torch.is_grad_enabled() and any(w.requires_grad for w in (W0, Ws, W1))))


def res_rows(x, u, s, row_of, W0, Ws, W1, ops: str = "fused", plan: Optional[PoolPlan] = None) -> torch.Tensor:
    """x (T,Cin), tables u, s (R,H), row_of int32 (T,) with values in [0, R) or None (row 0 for every point), W0, Ws (H,Cin) — views
    with a row stride are read in place —, W1 (H,H) -> (T,H). Gradients go to x, u and s on the kernel path, to everything on the
    torch path. `plan`: the PoolPlan whose cells are the table's rows (row R-1 = n_cells being the row of the points without a cell),
    when the caller has one; without it the backward groups the rows by table row itself."""
    check_ops(ops)
    H = W1.shape[0]
    if x.dim() != 2 or tuple(W0.shape) != (H, x.shape[1]) or tuple(Ws.shape) != (H, x.shape[1]) or tuple(W1.shape) != (H, H):
        raise ValueError(f"res_rows: x {tuple(x.shape)}, W0 {tuple(W0.shape)}, Ws {tuple(Ws.shape)}, W1 {tuple(W1.shape)} do not fit")
    if u.dim() != 2 or u.shape != s.shape or u.shape[1] != H or u.shape[0] < 1:
        raise ValueError(f"res_rows: tables u {tuple(u.shape)}, s {tuple(s.shape)}: expected (R, {H})")
    if row_of is not None and tuple(row_of.shape) != (x.shape[0],):
        raise ValueError(f"res_rows: row_of {tuple(row_of.shape)}, x has {x.shape[0]} rows")
    if plan is not None and (plan.T != x.shape[0] or plan.n_cells + 1 != u.shape[0]):
        raise ValueError(f"res_rows: the plan has {plan.T} points and {plan.n_cells} cells, x {x.shape[0]} rows and the tables {u.shape[0]}")
    if ops == "torch" or not _kernel_ok(x, u, s, row_of, W0, Ws, W1):
        return _res_rows_ref(x, u, s, row_of, W0, Ws, W1)
    return _ResRowsFn.apply(x, u, s, row_of, plan, W0, Ws, W1)


class _CellMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, plan):
        net = rows(net.detach())
        m, ctx.argmax = _launch_cell_max(net, plan)
        ctx.T = net.shape[0]
        return m

    @staticmethod
    def backward(ctx, gm):
        gm = gm.float().contiguous()
        n_cells, Cc = ctx.argmax.shape
        gx = torch.zeros(ctx.T, Cc, dtype=torch.float32, device=gm.device)
        launch("gh_res_cell_max_backward", gm.device, ptr(gm), ptr(ctx.argmax), ctx.T, Cc, n_cells, ptr(gx), Cc)
        return gx, None


def cell_max(net: torch.Tensor, plan: PoolPlan, ops: str = "fused") -> torch.Tensor:
    """net (T,H) -> (n_cells + 1, H): per cell and channel the maximum under pool's rules (ties to the lowest point index, a NaN never
    wins, 0 for an empty cell), the last row zeros. Differentiable: a cell's gradient goes to its argmax row. No (T,H) tensor is
    written on the kernel path; on the CPU and for ops="torch" it is pool._cell_max."""
    check_ops(ops)
    plan._fits(net, "net")
    if ops == "torch" or not net.is_cuda or net.dtype != torch.float32:
        vals, _ = _cell_max(net, plan)
        return torch.cat([vals, vals.new_zeros(1, vals.shape[1])])
    return _CellMaxFn.apply(net, plan)


def cell_mean(net: torch.Tensor, plan: PoolPlan, ops: str = "fused") -> torch.Tensor:
    """The mean-pooling counterpart of cell_max: plane_mean(net, plan).t() with the zero row appended."""
    mean = (_plane_mean_ref(net, plan) if ops == "torch" or net.dtype != torch.float32 else plane_mean(net, plan)).t()
    return torch.cat([mean, mean.new_zeros(1, mean.shape[1])])


def row_index(plan: PoolPlan) -> torch.Tensor:
    """int32 (T,): a point's cell, n_cells — the zero row — for a point whose index is out of range (pool_cat gives it zeros)."""
    idx = plan.index
    ok = (idx >= 0) & (idx < plan.n_cells)
    return torch.where(ok, idx, torch.full_like(idx, plan.n_cells)).to(torch.int32)


def folded_block(block: nn.Module, net: torch.Tensor, m: Optional[torch.Tensor], row_of: Optional[torch.Tensor], ops: str = "fused",
                 plan: Optional[PoolPlan] = None) -> torch.Tensor:
    """block(torch.cat([net, m[row_of]], dim=1)) for a module with fc_0, fc_1 and shortcut (pool.ResnetBlockFC), without the
    concatenation: net (T,H), m (R,H) the pooled rows. m=None: `net` is the block's whole (T,2H) input (block 0) and the tables are
    the two biases."""
    check_ops(ops)
    if block.shortcut is None:                            # the reference's identity shortcut has no weight to fold
        return block(net if m is None else torch.cat([net, m.index_select(0, row_of.long())], dim=1))
    W0, Ws, W1 = block.fc_0.weight, block.shortcut.weight, block.fc_1.weight
    if m is None:
        return res_rows(net, block.fc_0.bias.unsqueeze(0), block.fc_1.bias.unsqueeze(0), None, W0, Ws, W1, ops)
    H = net.shape[1]
    u = F.linear(torch.relu(m), W0[:, H:], block.fc_0.bias)
    s = F.linear(m, Ws[:, H:], block.fc_1.bias)
    return res_rows(net, u, s, row_of, W0[:, :H], Ws[:, :H], W1, ops, plan=plan)


def plane_linear(net: torch.Tensor, plan: PoolPlan, fc_c: nn.Module, ops: str = "fused") -> torch.Tensor:
    """plane_mean(fc_c(net), plan) as fc_c over the per-cell means: (c_dim, n_cells), exact zeros for empty cells."""
    check_ops(ops)
    mean = (_plane_mean_ref(net, plan) if ops == "torch" or net.dtype != torch.float32 else plane_mean(net, plan)).t()
    out = fc_c(mean)
    return torch.where((plan.counts() > 0).unsqueeze(1), out, torch.zeros_like(out)).t()


def folded_cloud(self, x0: torch.Tensor, plan: PoolPlan, reduce: str, ops: str, record) -> torch.Tensor:
    """One cloud of pool.pointnet_forward under blocks="folded": x0 (T,2H) = fc_pos's rows -> the plane (c_dim, n_cells). `record`
    receives the pooled cell rows m[:n_cells] of every block (not the (T,H) tensors of the unfolded path)."""
    nb = folded_block(self.blocks[0], x0, None, None, ops)
    row_of = row_index(plan)
    for block in self.blocks[1:]:
        m = cell_max(nb, plan, ops) if reduce == "max" else cell_mean(nb, plan, ops)
        if record is not None:
            record.append(m[:plan.n_cells].detach())
        nb = folded_block(block, nb, m, row_of, ops, plan=plan)
    return plane_linear(nb, plan, self.fc_c, ops)
