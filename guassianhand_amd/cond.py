"""The point conditioning: the rows the reference's TGS._forward concatenates per point (infer_one_shot.py:241-274) and their two kinds
of consumer, without the columns that repeat a batch-wide vector in every row — through include/gh_cond.h.

    PointRows(uv, xyz, flag, code, broadcast=(pose_feats, ...), levels=4)     stands for
        torch.cat([uv, sp(uv), xyz, sp(xyz), flag, code, *[b.repeat(1, N, 1) for b in broadcast]], dim=-1)
    with sp = SpatialEncoder(sp_level=levels) (spatial.py:25-40), every segment optional, without building it.

    rows.dense()            that concatenation in plain torch: the fallback and the yardstick
    rows.varying()          its first Dv columns (everything but the broadcast vectors): one HIP launch (gh_cond_rows)
    rows.linear(fc)         fc(rows.dense()) as a Dv-wide GEMM over varying() plus a per-batch bias from the broadcast vectors
    rows.uv_columns()       the first two columns, for pool.cell_index
    cond_mlp(rows, params)  fc2(relu(fc1(LayerNorm(rows.dense())))) — the reference's additional_features_fc in eval() — with the
                            broadcast columns folded into per-batch constants (gh_cond_fold) and the rows built in LDS
                            (gh_cond_mlp_forward / _backward); `code` is the only differentiable input of that path

`pool.pointnet_forward` takes a PointRows for `p` (cell index from uv_columns(), first layer through linear()).
`AdditionalFeaturesFC` is the module with the reference's state-dict keys; `additional_features(...)` is the seam for `_forward`.

The kernels are taken for float32 ROCm tensors when only `code` may need a gradient, 1 <= levels <= 8, Cc <= 64 and Hd <= 64.
Anything else — a gradient wanted for uv, xyz, a broadcast vector or a parameter, another dtype, CPU tensors, `ops="torch"` — runs
the plain-torch restatement (dense() + F.layer_norm + F.linear), which works wherever the reference's statements did; it takes
acc=torch.float64 for the tests. Dropout: MLP_block holds two nn.Dropout(0.1); the kernels are taken only when the module is not in
training mode or both p are 0, otherwise the module's own layers run over dense(), dropout included."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi
from ._call import check_ops, cotangent, launch, lib, ptr, row_stride, rows as _rows_in_place, struct
from ._mlp_block import _MLPBlock, block_params as _block_params, dropout_live, init_linears

PARAMS = _abi.COND_PARAMS                                        # the order of cond_mlp's `params` (GhCondParams)
MAX_LEVELS, MAX_CODE, MAX_HD = _abi.GH_COND_MAX_LEVELS, _abi.GH_COND_MAX_CODE, _abi.GH_COND_MAX_HD


def spatial_encode(x: torch.Tensor, levels: int) -> torch.Tensor:
    """SpatialEncoder(sp_level=levels)(x) for x (B,N,C): cat([x, sin/cos levels]) with f_l = float32(pi * 2^l), statement for
    statement (spatial.py:25-48). In another dtype than float32 the frequencies are still the float32 values."""
    if levels <= 0:
        return x
    vec = torch.from_numpy(np.asarray([math.pi * (1 << l) for l in range(levels)], dtype=np.float32)).to(x.device)
    if x.dtype != torch.float32:
        vec = vec.to(x.dtype)
    B, N, Cx = x.shape
    y = x[:, :, None, :] * vec[None, None, :, None]
    z = torch.cat((torch.sin(y), torch.cos(y)), dim=-1).view(B, N, 2 * Cx * levels)     # (the reference's view(B, N, -1), spelled out: N = 0 is allowed)
    return torch.cat([x, z], -1)


def _desc(uv, xyz, flag, code, levels):
    """The GhCondRows of (P,.) tensors (or None), and the tensors it points into (to be kept alive by the caller)."""
    code = None if code is None or code.shape[1] == 0 else code
    return _abi.GhCondRows(*[None if t is None else t.data_ptr() for t in (uv, xyz, flag, code)],
                           0 if code is None else row_stride(code), 0 if code is None else code.shape[1], int(levels))


def _flat(t, width=None):
    """(B,N,C) -> (B*N,C) float32 contiguous, detached (flag: (B,N,1) or (B,N), any dtype -> (B*N,) float32)."""
    if t is None:
        return None
    t = t.detach()
    if width is None:
        return t.reshape(-1).to(torch.float32).contiguous()
    return t.reshape(-1, width).contiguous()


class _RowsFn(torch.autograd.Function):
    """gh_cond_rows over flat tensors; the gradient of `code` is the last Cc columns of the incoming gradient."""

    @staticmethod
    def forward(ctx, code, uv, xyz, flag, levels, Dv):
        dev = next(t for t in (code, uv, xyz, flag) if t is not None).device
        P = next(t for t in (code, uv, xyz, flag) if t is not None).shape[0]
        codes = None if code is None else _rows_in_place(code.detach())
        out = torch.empty(P, Dv, dtype=torch.float32, device=dev)
        if P > 0:
            d = _desc(uv, xyz, flag, codes, levels)
            launch("gh_cond_rows", dev, C.byref(d), P, ptr(out), Dv, what=f"gh_cond_rows (P={P}, Dv={Dv})")
        ctx.Cc = 0 if code is None else code.shape[1]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (g[:, g.shape[1] - ctx.Cc:] if ctx.Cc and ctx.needs_input_grad[0] else None), None, None, None, None, None


class _CondMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, code, uv, xyz, flag, e, cfg, *params):
        N, levels, eps, Dv = cfg
        ctx.set_materialize_grads(False)
        first = next(t for t in (code, uv, xyz, flag) if t is not None)
        dev, P = first.device, first.shape[0]
        B = P // N if N > 0 else 0
        codes = None if code is None else _rows_in_place(code.detach())
        params = [p.detach().contiguous() for p in params]
        Hd, De = params[2].shape[0], 0 if e is None else e.shape[1]
        out = torch.empty(P, Hd, dtype=torch.float32, device=dev)
        fold = None
        if P > 0:
            nbytes = int(lib().gh_cond_fold_bytes(B, Dv, Hd))
            fold = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            ps = struct(_abi.GhCondParams, params)
            d = _desc(uv, xyz, flag, codes, levels)
            what = f"(B={B}, N={N}, Dv={Dv}, De={De}, Hd={Hd})"
            launch("gh_cond_fold", dev, ptr(e), B, De, Dv, Hd, C.byref(ps), ptr(fold), nbytes, what="gh_cond_fold " + what)
            launch("gh_cond_mlp_forward", dev, C.byref(d), P, N, De, Hd, C.byref(ps), ptr(fold), float(eps), ptr(out),
                   what="gh_cond_mlp_forward " + what)
        ctx.cfg, ctx.dims = cfg, (P, De, Hd)
        # the inputs, and the fold's constants (Hd * (Dv + 1) + B * (2 + 2 Hd) floats): what gh_cond_fold would write again
        ctx.save_for_backward(codes, uv, xyz, flag, fold, params[4])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        codes, uv, xyz, flag, fold, w2 = ctx.saved_tensors
        N, levels, eps, Dv = ctx.cfg
        P, De, Hd = ctx.dims
        dcode = None
        if codes is not None and ctx.needs_input_grad[0]:
            dcode = torch.empty(P, codes.shape[1], dtype=torch.float32, device=codes.device)
            if P > 0:
                g = cotangent(g_out)
                ps = struct(_abi.GhCondParams, [w2] * 6)              # (the backward reads fc2_weight; the rest reach it through fold)
                d = _desc(uv, xyz, flag, codes, levels)
                launch("gh_cond_mlp_backward", codes.device, C.byref(d), P, N, De, Hd, C.byref(ps), ptr(fold), float(eps), ptr(g),
                       ptr(dcode), codes.shape[1], what=f"gh_cond_mlp_backward (P={P}, N={N}, Dv={Dv}, De={De}, Hd={Hd})")
        return (dcode, None, None, None, None, None) + (None,) * 6


class PointRows:
    """The per-point conditioning rows of a batch without the concatenation: uv (B,N,2), xyz (B,N,3), flag (B,N,1) or (B,N) of any
    dtype (the reference's is bool), code (B,N,Cc), each optional, then the (B,1,.) vectors of `broadcast`, every one repeated over
    the N points. `levels` is the SpatialEncoder's sp_level, applied to uv and to xyz."""

    def __init__(self, uv=None, xyz=None, flag=None, code=None, broadcast: Sequence[torch.Tensor] = (), levels: int = 4):
        self.uv, self.xyz, self.code, self.levels = uv, xyz, code, int(levels)
        self.broadcast = tuple(broadcast)
        given = [t for t in (uv, xyz, flag, code) if t is not None]
        if not given:
            raise ValueError("PointRows needs at least one of uv, xyz, flag, code")
        self.B, self.N = int(given[0].shape[0]), int(given[0].shape[1])
        self.device = given[0].device
        floats = [t for t in (uv, xyz, code) + self.broadcast if t is not None]
        self.dtype = floats[0].dtype if floats else torch.float32
        if flag is not None:
            flag = flag.reshape(self.B, self.N, 1)
            if flag.dtype != self.dtype:
                flag = flag.to(self.dtype)                         # the reference's bool mask, converted once
        self.flag = flag
        for name, t, w in (("uv", uv, 2), ("xyz", xyz, 3), ("flag", flag, 1), ("code", code, None)):
            if t is not None and (t.dim() != 3 or tuple(t.shape[:2]) != (self.B, self.N) or (w is not None and t.shape[2] != w)):
                raise ValueError(f"{name}: expected ({self.B}, {self.N}, {w if w is not None else 'Cc'}), got {tuple(t.shape)}")
        for i, b in enumerate(self.broadcast):
            if b.dim() != 3 or b.shape[0] != self.B or b.shape[1] != 1:
                raise ValueError(f"broadcast[{i}]: expected ({self.B}, 1, C), got {tuple(b.shape)}")
        L = self.levels
        pe = lambda c: c * (2 + 2 * max(L, 0))                      # x, then sp(x) = (x, sin / cos levels); sp(x) = x for L <= 0
        self.Cc = 0 if code is None else int(code.shape[2])
        self.Dv = (pe(2) if uv is not None else 0) + (pe(3) if xyz is not None else 0) + (1 if flag is not None else 0) + self.Cc
        self.De = sum(int(b.shape[2]) for b in self.broadcast)

    # ---- plain torch -----------------------------------------------------------------------------------------------------------
    def _varying_ref(self, acc: Optional[torch.dtype] = None) -> torch.Tensor:
        c = (lambda t: t.to(acc)) if acc is not None else (lambda t: t)
        parts = []
        for t in (self.uv, self.xyz):
            if t is not None:
                parts += [c(t), spatial_encode(c(t), self.levels)]
        parts += [c(t) for t in (self.flag, self.code) if t is not None]
        return torch.cat(parts, dim=-1)

    def shared(self, acc: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
        """(B,1,De): the broadcast vectors side by side, or None without any."""
        if not self.broadcast:
            return None
        e = torch.cat(self.broadcast, dim=-1) if len(self.broadcast) > 1 else self.broadcast[0]
        return e if acc is None else e.to(acc)

    def dense(self, acc: Optional[torch.dtype] = None) -> torch.Tensor:
        """The reference's torch.cat, (B,N,Dv+De)."""
        c = (lambda t: t.to(acc)) if acc is not None else (lambda t: t)
        return torch.cat([self._varying_ref(acc)] + [c(b).repeat(1, self.N, 1) for b in self.broadcast], dim=-1)

    def uv_columns(self) -> torch.Tensor:
        """(B,N,2): the first two columns of the row, what pool.cell_index reads."""
        if self.uv is not None:
            return self.uv
        return self._varying_ref()[..., :2]

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def _kernel_rows_ok(self) -> bool:
        every = [t for t in (self.uv, self.xyz, self.flag, self.code) if t is not None]
        return (self.device.type == "cuda" and all(t.dtype == torch.float32 and t.device == self.device for t in every)
                and 1 <= self.levels <= MAX_LEVELS and self.Cc <= MAX_CODE
                and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (self.uv, self.xyz, self.flag))))

    def _flat_inputs(self):
        code = None if self.code is None or self.Cc == 0 else self.code.reshape(-1, self.Cc)     # (a view where the layout allows)
        return code, _flat(self.uv, 2), _flat(self.xyz, 3), _flat(self.flag)

    def varying(self, ops: str = "fused") -> torch.Tensor:
        """(B,N,Dv): the row without the broadcast vectors; differentiable in `code` on the kernel path, in everything otherwise."""
        if ops == "torch" or not self._kernel_rows_ok():
            return self._varying_ref()
        code, uv, xyz, flag = self._flat_inputs()
        return _RowsFn.apply(code, uv, xyz, flag, self.levels, self.Dv).reshape(self.B, self.N, self.Dv)

    def linear(self, fc: nn.Linear, ops: str = "fused") -> torch.Tensor:
        """fc(self.dense()) as W[:, :Dv] over the varying rows plus, per batch element, W[:, Dv:] . broadcast + bias. Plain torch on
        the kernel's rows: weights, bias, broadcast vectors and `code` get their gradients from autograd."""
        W, Dv = fc.weight, self.Dv
        if W.shape[1] != Dv + self.De:
            raise ValueError(f"fc takes {W.shape[1]} inputs, the rows have {Dv} + {self.De}")
        rows = self.varying(ops)
        e = self.shared()
        if e is None:
            return F.linear(rows, W, fc.bias)
        bias = F.linear(e.to(rows.dtype), W[:, Dv:], fc.bias)                           # (B,1,H)
        return torch.baddbmm(bias, rows, W[:, :Dv].t().unsqueeze(0).expand(self.B, Dv, W.shape[0]))


# ---- the LayerNorm + MLP -------------------------------------------------------------------------------------------------------------
def _cond_mlp_ref(rows: PointRows, params, eps: float = 1e-6, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """LayerNorm, fc1 + ReLU, fc2 over rows.dense() in plain torch, differentiable, statement for statement MLP_block in eval mode.
    acc=torch.float64 computes (and returns) in double."""
    x = rows.dense(acc)
    if acc is not None:
        params = [p.to(acc) for p in params]
    g, b, w1, b1, w2, b2 = params
    x = F.layer_norm(x, (x.shape[-1],), g, b, eps)
    return F.linear(F.relu(F.linear(x, w1, b1)), w2, b2)


def _mlp_kernel_ok(rows: PointRows, params) -> bool:
    grad = torch.is_grad_enabled()
    e = rows.broadcast
    return (rows._kernel_rows_ok()
            and all(isinstance(p, torch.Tensor) and p.dtype == torch.float32 and p.device == rows.device for p in params)
            and all(b.dtype == torch.float32 and b.device == rows.device for b in e)
            and params[2].shape[0] <= MAX_HD
            and not (grad and any(t.requires_grad for t in tuple(params) + tuple(e))))


def cond_mlp(rows: PointRows, params: Sequence[torch.Tensor], eps: float = 1e-6, ops: str = "fused") -> torch.Tensor:
    """rows -> (B,N,Hd): fc2(relu(fc1(LayerNorm(rows.dense())))) with params in PARAMS order: LayerNorm weight and bias (D = Dv + De),
    fc1 (Hd,D) and its bias, fc2 (Hd,Hd) and its bias. ops="torch" runs the plain-torch restatement on the rows' device."""
    check_ops(ops)
    params = tuple(params)
    if len(params) != len(PARAMS):
        raise ValueError(f"params: expected the {len(PARAMS)} tensors {PARAMS}, got {len(params)}")
    D, Hd = rows.Dv + rows.De, params[2].shape[0]
    for name, p, shape in zip(PARAMS, params, ((D,), (D,), (Hd, D), (Hd,), (Hd, Hd), (Hd,))):
        if tuple(p.shape) != shape:
            raise ValueError(f"{name}: expected {shape} for Dv + De = {rows.Dv} + {rows.De}, Hd = {Hd}, got {tuple(p.shape)}")
    if ops == "torch" or not _mlp_kernel_ok(rows, params):
        return _cond_mlp_ref(rows, list(params), eps=float(eps))
    code, uv, xyz, flag = rows._flat_inputs()
    e = rows.shared()
    e = None if e is None else e.detach().reshape(rows.B, rows.De).contiguous()
    out = _CondMlpFn.apply(code, uv, xyz, flag, e, (rows.N, rows.levels, float(eps), rows.Dv), *params)
    return out.reshape(rows.B, rows.N, Hd)


# ---- the module and the seam ---------------------------------------------------------------------------------------------------------
def module_forward(module, rows: PointRows, ops: str = "fused") -> torch.Tensor:
    """additional_features_fc.forward over a PointRows. With dropout live (train mode, p > 0) the module's own forward runs over
    rows.dense(), exactly the reference's statements; otherwise cond_mlp over the module's own parameters."""
    ff = module.ff1
    if dropout_live(module, ff):
        return module(rows.dense())
    return cond_mlp(rows, _block_params(ff), eps=float(ff.layer_norm.eps), ops=ops)


class AdditionalFeaturesFC(nn.Module):
    """The reference's additional_features_fc (verts_refinement.py:119-131) with its state-dict keys (ff1.layer_norm.*, ff1.fc1.*,
    ff1.fc2.*) and initialisation (Xavier-uniform weights, zero biases; LayerNorm's ones and zeros). Takes the concatenated tensor
    as the reference does, or a PointRows."""

    def __init__(self, f_dim_in: int, f_dim_out: int, ops: str = "fused"):
        super().__init__()
        self.ff1 = _MLPBlock(int(f_dim_in), int(f_dim_out))
        self.cond_ops = ops
        init_linears(self)

    def forward(self, verts_f):
        if isinstance(verts_f, PointRows):
            return module_forward(self, verts_f, self.cond_ops)
        return self.ff1(verts_f)


def additional_features(fc_module, vert_uv, pointclouds, mink_idxs_inter, identity_code_vert, pose_feats, levels: int = 4,
                        ops: str = "fused") -> torch.Tensor:
    """The two statements of TGS._forward (infer_one_shot.py:273-274): the 852-column concatenation and additional_features_fc over
    it, reading fc_module's own parameters (the reference's module or AdditionalFeaturesFC)."""
    rows = PointRows(uv=vert_uv, xyz=pointclouds, flag=mink_idxs_inter, code=identity_code_vert, broadcast=(pose_feats,), levels=levels)
    return module_forward(fc_module, rows, ops)
