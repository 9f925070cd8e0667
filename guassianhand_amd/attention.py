"""The interaction attention: the reference's SelfAttn (tgs/models/self_attn.py:36-85), which GS3DRenderer.forward applies to the
points `mink_idxs_inter` flags (renderer_one_shot.py:554-574), with its attention core — `matmul(q, k^T) / norm`, `softmax`,
`matmul(attn, v)` (`:70-74`) — as HIP kernels through include/gh_attn.h.

    attention(q, k, v, *, norm=None, ops="fused")   q, k, v (BS, V, H, D) float32 -> (BS, V, H * D)

The kernels stream the keys past every query row with a running maximum and sum: nothing of size V x V exists, forward or backward
(the reference's form holds 4 x V x V floats twice and autograd keeps one of them). The call is differentiable in q, k and v. Saved
for the backward: q, k, v, the output and one float per (batch, head, row). The backward is two kernels — one owns dk and dv of a key
block, one owns dq of a query block — and runs only the one `needs_input_grad` asks for. No atomics: every result is bitwise
reproducible, and a row's output does not depend on the other rows of the launch, on BS, on the head index or on the strides.
q, k and v are read in place through their batch, row and head strides (`w_qs(x).view(BS, V, H, D)`, or three column windows of one
(BS, V, 3 * H * D) tensor); only a tensor whose last stride is not 1 is copied, once.

CPU tensors, `ops="torch"`, any D other than 32 and any dtype other than float32 go through `attention_ref`: the reference's three
statements, in float64 on request (the yardstick of the tests). ROCm float32 tensors with D = 32 go through the HIP kernels only.

`SelfAttn` is the module itself with the reference's state-dict keys (`w_qs`, `w_ks`, `w_vs`, `layer_norm`, `fc`, `ff.layer_norm`,
`ff.fc1`, `ff.fc2`, each with weight and bias) and default initialisation, so a reference checkpoint loads unchanged.
`fused_self_attn_cls(base)` grafts `self_attn(x)` onto the reference's own class — the module's own `w_qs`, `w_ks`, `w_vs`, then
`attention`, then its own `fc`; `forward` (LayerNorm, residual, `ff`) stays the base class's — and `fuse_self_attn(renderer)` swaps
the class of `renderer.self_attn_layer` for it (module object, parameters and state dict untouched): what the config strings
`guassianhand_amd.tgs_renderer.GS3DRendererFusedAttn` / `...FusedAllFetchAttn` (and their `Edit` forms) do in `configure()`.

Dropout. `dropout1` acts on the probabilities, which the fused form never holds. The kernels are taken only when `not self.training`
or both attention dropouts have p = 0; otherwise a grafted module calls the base class's `self_attn` unchanged (and SelfAttn runs the
reference's statements in plain torch, dropout included)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam
from ._call import check_ops, launch, lib, ptr, workspace

HEAD_DIM = _abi.GH_ATTN_D


def _norm_of(q: torch.Tensor, norm) -> float:
    return float(q.shape[-1]) ** 0.5 if norm is None else float(norm)


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, norm=None, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """q, k (BS, V, H, D), v (BS, V, H, Dv) -> (BS, V, H * Dv): the reference's statements (self_attn.py:66-74 after the projections,
    dropout inactive), differentiable. acc=torch.float64 computes (and returns) in double."""
    norm = _norm_of(q, norm)
    if acc is not None:
        q, k, v = q.to(acc), k.to(acc), v.to(acc)
    BS, V, width = q.shape[0], q.shape[1], v.shape[2] * v.shape[3]
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    attn = torch.matmul(q, k.transpose(-1, -2)) / norm
    attn = F.softmax(attn, dim=-1)
    return torch.matmul(attn, v).transpose(1, 2).contiguous().view(BS, V, width)


# ---- device path ---------------------------------------------------------------------------------------------------------------
def _in_place(t: torch.Tensor) -> torch.Tensor:
    """The tensor as the kernels read it: unit last stride, anything else in the other three dimensions; otherwise one copy."""
    t = t.detach()
    return t if t.shape[-1] == 1 or t.stride(-1) == 1 else t.contiguous()


def _tensor(t: torch.Tensor) -> _abi.GhAttnTensor:
    return _abi.GhAttnTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _dims(q: torch.Tensor, norm: float) -> _abi.GhAttnDims:
    BS, V, H, D = q.shape
    return _abi.GhAttnDims(BS, V, H, D, norm)


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, norm):
        q, k, v = _in_place(q), _in_place(k), _in_place(v)
        BS, V, H, D = q.shape
        dev = q.device
        out = torch.empty(BS, V, H * D, dtype=torch.float32, device=dev)
        lse = torch.empty(BS, H, V, dtype=torch.float32, device=dev)
        if BS > 0 and V > 0:
            dims, tq, tk, tv = _dims(q, norm), _tensor(q), _tensor(k), _tensor(v)
            launch("gh_attn_forward", dev, C.byref(dims), C.byref(tq), C.byref(tk), C.byref(tv), ptr(out), ptr(lse),
                   what=f"gh_attn_forward (BS={BS}, V={V}, H={H}, D={D})")
        ctx.norm = norm
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_lse):
        q, k, v, out, lse = ctx.saved_tensors
        BS, V, H, D = q.shape
        dev = q.device
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        new = lambda: torch.empty(BS, V, H, D, dtype=torch.float32, device=dev)
        dq, dk, dv = (new() if need else None for need in (need_q, need_k, need_v))
        if BS > 0 and V > 0 and (need_q or need_k or need_v):
            g = _in_place(g_out.float().reshape(BS, V, H, D))
            dims = _dims(q, ctx.norm)
            nbytes = int(lib().gh_attn_workspace_bytes(C.byref(dims)))
            ws = workspace(nbytes, dev)
            tq, tk, tv, tg = _tensor(q), _tensor(k), _tensor(v), _tensor(g)
            launch("gh_attn_backward", dev, C.byref(dims), C.byref(tq), C.byref(tk), C.byref(tv), ptr(out), ptr(lse), C.byref(tg),
                   ptr(dq), ptr(dk), ptr(dv), ptr(ws), nbytes, what=f"gh_attn_backward (BS={BS}, V={V}, H={H}, D={D})")
        return dq, dk, dv, None


def _check(q, k, v) -> None:
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dim() != 4:
            raise ValueError(f"{name}: expected (BS, V, H, D), got {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name} is on {t.device}, q on {q.device}")
        if t.dtype != q.dtype:
            raise TypeError(f"{name} is {t.dtype}, q {q.dtype}")
    if k.shape != q.shape:
        raise ValueError(f"k: expected {tuple(q.shape)} as q, got {tuple(k.shape)}")
    if v.shape[:3] != q.shape[:3]:
        raise ValueError(f"v: expected {tuple(q.shape[:3])} + (Dv,), got {tuple(v.shape)}")


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, norm=None, ops: str = "fused", return_lse: bool = False):
    """q, k, v (BS, V, H, D) -> (BS, V, H * D): softmax((q k^T) / norm) v per (batch, head), norm = sqrt(D) unless given.
    Differentiable in q, k and v. ops="torch" runs attention_ref on the tensors' device; CPU tensors, D != 32 and any dtype other
    than float32 (float64, or the half types a module yields under autocast) always take it.
    return_lse=True also returns ln sum exp(score) per row, (BS, H, V), not differentiable: what the kernels keep for the backward,
    exposed so that the tests can check its bits under a permutation of the rows."""
    check_ops(ops)
    _check(q, k, v)
    norm = _norm_of(q, norm)
    if not norm > 0:
        raise ValueError(f"norm must be > 0, got {norm}")
    BS, V, H, D = q.shape
    if ops == "torch" or not q.is_cuda or D != HEAD_DIM or v.shape[3] != HEAD_DIM or q.dtype != torch.float32:
        out = attention_ref(q, k, v, norm)
        if return_lse:
            with torch.no_grad():
                s = torch.matmul(q.transpose(1, 2), k.transpose(1, 2).transpose(-1, -2)) / norm
            return out, torch.logsumexp(s, dim=-1)
        return out
    if BS * H > _abi.GH_ATTN_MAX_BH or V > _abi.GH_ATTN_MAX_V:
        raise ValueError(f"attention: BS * H = {BS * H} (limit {_abi.GH_ATTN_MAX_BH}) or V = {V} (limit {_abi.GH_ATTN_MAX_V}) is too large")
    out, lse = _AttentionFn.apply(q, k, v, norm)
    return (out, lse) if return_lse else out


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _attn_dropout_active(self) -> bool:
    return bool(self.training) and any(float(getattr(d, "p", 0.0)) > 0 for d in (self.dropout1, self.dropout2))


def self_attn_core(self, x: torch.Tensor, ops: str = "fused") -> torch.Tensor:
    """SelfAttn.self_attn (self_attn.py:63-76) with dropout inactive: the module's own w_qs, w_ks, w_vs, then attention on their
    outputs read in place, then the module's own fc."""
    BS, V, _ = x.shape
    q = self.w_qs(x).view(BS, -1, self.n_heads, self.d_q)
    k = self.w_ks(x).view(BS, -1, self.n_heads, self.d_q)
    v = self.w_vs(x).view(BS, -1, self.n_heads, self.d_v)
    out = attention(q, k, v, norm=self.norm, ops=ops)
    return self.fc(out)


class _MLPResBlock(nn.Module):
    """The reference's MLP_res_block (self_attn.py:17-33): the sub-module names are its state-dict keys."""

    def __init__(self, in_dim: int, hid_dim: int, dropout: float = 0.1):
        super().__init__()
        self.layer_norm = nn.LayerNorm(in_dim, eps=1e-6)
        self.fc1 = nn.Linear(in_dim, hid_dim)
        self.fc2 = nn.Linear(hid_dim, in_dim)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, x):
        return x + self.dropout2(self.fc2(self.dropout1(F.relu(self.fc1(self.layer_norm(x))))))


class SelfAttn(nn.Module):
    """The reference's SelfAttn with its state-dict keys and default initialisation (nn.Linear's and nn.LayerNorm's own: the
    reference applies no weights_init here). eval(), or dropout p = 0: the attention core runs the HIP kernels on ROCm tensors.
    train() with p > 0: the reference's statements in plain torch, dropout on the probabilities included."""

    def __init__(self, f_dim, hid_dim=None, n_heads=4, d_q=None, d_v=None, dropout=0.1):
        super().__init__()
        d_q = f_dim // n_heads if d_q is None else d_q
        d_v = f_dim // n_heads if d_v is None else d_v
        hid_dim = f_dim if hid_dim is None else hid_dim
        self.n_heads, self.d_q, self.d_v, self.norm, self.f_dim = n_heads, d_q, d_v, d_q ** 0.5, f_dim
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.w_qs = nn.Linear(f_dim, n_heads * d_q)
        self.w_ks = nn.Linear(f_dim, n_heads * d_q)
        self.w_vs = nn.Linear(f_dim, n_heads * d_v)
        self.layer_norm = nn.LayerNorm(f_dim, eps=1e-6)
        self.fc = nn.Linear(n_heads * d_v, f_dim)
        self.ff = _MLPResBlock(f_dim, hid_dim, dropout)

    def _torch_self_attn(self, x):
        """The reference's self_attn, statement for statement (dropout included): the train-mode path."""
        BS, V, _ = x.shape
        q = self.w_qs(x).view(BS, -1, self.n_heads, self.d_q).transpose(1, 2)
        k = self.w_ks(x).view(BS, -1, self.n_heads, self.d_q).transpose(1, 2)
        v = self.w_vs(x).view(BS, -1, self.n_heads, self.d_v).transpose(1, 2)
        attn = torch.matmul(q, k.transpose(-1, -2)) / self.norm
        attn = self.dropout1(F.softmax(attn, dim=-1))
        out = torch.matmul(attn, v).transpose(1, 2).contiguous().view(BS, V, -1)
        return self.dropout2(self.fc(out))

    def self_attn(self, x):
        if _attn_dropout_active(self):
            return self._torch_self_attn(x)
        return self_attn_core(self, x)

    def forward(self, x):
        assert x.shape[-1] == self.f_dim
        x = x + self.self_attn(self.layer_norm(x))
        return self.ff(x)


_SEAM = (__name__, "fused_self_attn_cls")


def fused_self_attn_cls(base):
    """A subclass of the given class (the reference's own tgs.models.self_attn.SelfAttn) whose self_attn(x) is self_attn_core while
    the attention dropouts are inactive, and the base class's own self_attn, unchanged, in train mode with p > 0. forward stays
    the base class's."""
    def self_attn(self, x):
        if _attn_dropout_active(self):
            return base.self_attn(self, x)
        return self_attn_core(self, x)

    return _seam.graft(_SEAM, base, {"self_attn": self_attn}, "attention core")


def fuse_self_attn(renderer):
    """Swap the class of `renderer.self_attn_layer` for fused_self_attn_cls of its own class: forward's refinement of the flagged
    points then runs the HIP attention core. The module object, its parameters and its state dict are untouched; it may be called on
    a renderer that is already built, and again. Returns the renderer."""
    m = renderer.self_attn_layer
    if not isinstance(m, SelfAttn):
        _seam.swap(_SEAM, m)
    return renderer
