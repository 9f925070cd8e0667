"""The interaction attention block whole: the reference's SelfAttn.forward (tgs/models/self_attn.py:78-85) — LayerNorm, the three
projections, the attention core, `fc`, the residual, the feed-forward block and its residual — and the loop that applies it to the
flagged points (renderer_one_shot.py:554-574), with everything around the core as two HIP launches each way through
include/gh_attn_rows.h and the core through include/gh_attn.h.

    attn_block(x, params, *, n_heads=4, eps=1e-6, idx=None, out=None, ops="fused")     x (BS, V, F) -> (BS, V, F)
    refine_flagged(features, flags, module, *, part_rows=30000, n_part=8, ops="fused") (B, N, F), (B, N) -> a new (B, N, F)

`params` are the module's sixteen tensors in state-dict order (`KEYS`), as a sequence or as a mapping with those keys. The block is
differentiable in x and in nothing else: the one-shot fit freezes every network parameter, and the kernels produce no parameter
gradient. One autograd.Function: its forward enqueues gh_attn_rows_pre_forward, gh_attn_forward and gh_attn_rows_post_forward, its
backward gh_attn_rows_post_backward, gh_attn_backward and gh_attn_rows_pre_backward. Saved for the backward: x, qkv, the core's out
and lse, y, four floats per row (the two LayerNorms' mean and rstd) and the ReLU's mask, (hid + 31) / 32 words per row.

With `idx` (int32, distinct rows of x's second dimension) only the listed rows attend, among themselves, and are refined; the other
rows of the result are copies of x (or, with `out`, what `out` held) and their gradient is the cotangent passed through.

`attn_block_ref` is the reference's statements in plain torch, in float64 on request: the CPU path and the yardstick of the tests.
CPU tensors, ops="torch", any dtype other than float32, widths outside 1 <= F, hid <= 192, 1 <= H <= 8 and a head width other than 32
always take it; it differentiates with respect to the parameters too.

`refine_flagged` is the reference's loop as a function, with the reference's rules: nothing happens when no row is flagged; a batch
element or a range without a flagged row is skipped; above `part_rows` points the ranges are [p L, (p + 1) L) with L = int(N / n_part),
each range attends among its own flagged rows, and rows at or beyond n_part L are never refined even when flagged (the reference's
quirk, kept). One compacted index over the flattened (B N) rows, one host read of the per-range counts, one launch ahead of the cores
and one behind over all listed rows, one core call per non-empty range on its window of the shared qkv buffer. Where the kernels do not
apply (below) it runs the loop over `module` itself.

`fused_attn_block_cls(base)` grafts `forward(x)` onto a SelfAttn class and `fuse_attn_block(renderer)` swaps the class of
`renderer.self_attn_layer` for it. The kernels are taken only while the four dropouts are inactive, autograd asks no parameter of the
module for a gradient, and the sizes are supported; otherwise the call goes to the forward the module had before the graft (the
`fuse_self_attn` class's if that graft is present, else the base class's)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam
from ._call import check_ops, launch, lib, ptr, struct, workspace
from .attention import HEAD_DIM, attention_ref

KEYS = tuple(f"{m}.{p}" for m in ("w_qs", "w_ks", "w_vs", "layer_norm", "fc", "ff.layer_norm", "ff.fc1", "ff.fc2") for p in ("weight", "bias"))
MAX_F, MAX_H = _abi.GH_ATTN_ROWS_MAX_F, _abi.GH_ATTN_ROWS_MAX_H


def _params(params) -> tuple:
    if hasattr(params, "keys"):
        params = [params[k] for k in KEYS]
    params = tuple(params)
    if len(params) != 16:
        raise ValueError(f"params: expected the {len(KEYS)} tensors {', '.join(KEYS)}, got {len(params)}")
    return params


def _eps(eps):
    return (float(eps[0]), float(eps[1])) if isinstance(eps, (tuple, list)) else (float(eps), float(eps))


def module_params(m) -> tuple:
    """The sixteen tensors of a SelfAttn module in state-dict order."""
    return (m.w_qs.weight, m.w_qs.bias, m.w_ks.weight, m.w_ks.bias, m.w_vs.weight, m.w_vs.bias, m.layer_norm.weight, m.layer_norm.bias,
            m.fc.weight, m.fc.bias, m.ff.layer_norm.weight, m.ff.layer_norm.bias, m.ff.fc1.weight, m.ff.fc1.bias, m.ff.fc2.weight,
            m.ff.fc2.bias)


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def attn_block_ref(x: torch.Tensor, params, *, n_heads: int = 4, eps=1e-6, norm=None, idx=None, out=None,
                   acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """SelfAttn.forward with dropout inactive, statement for statement, differentiable in x and in the parameters.
    acc=torch.float64 computes (and returns) in double."""
    wq, bq, wk, bk, wv, bv, g1, b1, wf, bf, g2, b2, w1, c1, w2, c2 = _params(params)
    eps1, eps2 = _eps(eps)
    if acc is not None:
        x = x.to(acc)
        wq, bq, wk, bk, wv, bv, g1, b1, wf, bf, g2, b2, w1, c1, w2, c2 = (t.to(acc) for t in (wq, bq, wk, bk, wv, bv, g1, b1, wf, bf, g2, b2,
                                                                                              w1, c1, w2, c2))
    whole = x
    if idx is not None:
        x = x.index_select(1, idx.long())
    BS, V, f = x.shape
    d_q, d_v = wq.shape[0] // n_heads, wv.shape[0] // n_heads
    xn = F.layer_norm(x, (f,), g1, b1, eps1)
    q = F.linear(xn, wq, bq).view(BS, -1, n_heads, d_q)
    k = F.linear(xn, wk, bk).view(BS, -1, n_heads, d_q)
    v = F.linear(xn, wv, bv).view(BS, -1, n_heads, d_v)
    y = x + F.linear(attention_ref(q, k, v, d_q ** 0.5 if norm is None else norm), wf, bf)
    z = y + F.linear(F.relu(F.linear(F.layer_norm(y, (f,), g2, b2, eps2), w1, c1)), w2, c2)
    if idx is None and out is None:
        return z
    if out is None:
        return whole.index_copy(1, idx.long(), z)
    if idx is None:
        return out.copy_(z)
    return out.index_copy_(1, idx.long(), z)


# ---- device path ---------------------------------------------------------------------------------------------------------------
def _supported(F_: int, HD: int, hid: int, n_heads: int, d_q: int, d_v: int) -> bool:
    return d_q == HEAD_DIM and d_v == HEAD_DIM and 1 <= n_heads <= MAX_H and HD == n_heads * HEAD_DIM and 1 <= F_ <= MAX_F and 1 <= hid <= MAX_F


def _shapes_ok(x: torch.Tensor, P: tuple, n_heads: int) -> bool:
    """x's last dimension and the sixteen shapes fit each other and the kernels' sizes; all float32 on x's device."""
    f = x.shape[-1]
    HD, hid = P[0].shape[0], P[12].shape[0]
    if n_heads < 1 or HD % n_heads:
        return False
    want = ((HD, f), (HD,), (HD, f), (HD,), (HD, f), (HD,), (f,), (f,), (f, HD), (f,), (f,), (f,), (hid, f), (hid,), (f, hid), (f,))
    if any(t is None or tuple(t.shape) != w or t.dtype != torch.float32 or t.device != x.device for t, w in zip(P, want)):
        return False
    return _supported(f, HD, hid, n_heads, HD // n_heads, HD // n_heads)


def _window(t: torch.Tensor, off: int, BS: int, V: int, HD: int, stride_v: int, col: int = 0) -> _abi.GhAttnTensor:
    """(BS, V, H, 32) of the rows [off, off + BS * V) of a (rows, stride_v) float32 buffer, from column col."""
    return _abi.GhAttnTensor(t.data_ptr() + 4 * (off * stride_v + col), V * stride_v, stride_v, HEAD_DIM)


def _at(t: torch.Tensor, elements: int):
    return C.c_void_p(t.data_ptr() + 4 * elements)


class _AttnBlockFn(torch.autograd.Function):
    """x2 (R, F) rows with a row stride; idx int32 (Vt,) or None (every row, in order); segs: the core's calls as (offset into the
    listed rows, BS, V), covering them all; P: the sixteen tensors, contiguous; out2: None or the (R, F) tensor to write the rows to."""

    @staticmethod
    def forward(ctx, x2, idx, segs, P, n_heads, eps1, eps2, norm, out2):
        dev, f = x2.device, x2.shape[1]
        HD, hid = P[0].shape[0], P[12].shape[0]
        Vt = x2.shape[0] if idx is None else idx.numel()
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        if out2 is None:
            out2 = new(x2.shape[0], f) if idx is None else x2.clone(memory_format=torch.contiguous_format)
        else:
            ctx.mark_dirty(out2)
        qkv, a, lse, y = new(Vt, 3 * HD), new(Vt, HD), new(n_heads * Vt), new(Vt, f)
        st1, st2, mask = new(Vt, 2), new(Vt, 2), new(Vt, (hid + 31) // 32, dt=torch.int32)
        dims = _abi.GhAttnRowsDims(Vt, f, n_heads, hid, eps1, eps2, _row_stride(x2), _row_stride(out2), f, f)
        pm = struct(_abi.GhAttnRowsParams, P)
        if Vt > 0:
            what = f"(V={Vt}, F={f}, H={n_heads}, hid={hid})"
            launch("gh_attn_rows_pre_forward", dev, C.byref(dims), C.byref(pm), ptr(x2), ptr(idx), ptr(qkv), ptr(st1),
                   what=f"gh_attn_rows_pre_forward {what}")
            for off, BS, V in segs:
                cd = _abi.GhAttnDims(BS, V, n_heads, HEAD_DIM, norm)
                tq, tk, tv = (_window(qkv, off, BS, V, HD, 3 * HD, c * HD) for c in range(3))
                launch("gh_attn_forward", dev, C.byref(cd), C.byref(tq), C.byref(tk), C.byref(tv), _at(a, off * HD), _at(lse, off * n_heads),
                       what=f"gh_attn_forward (BS={BS}, V={V}, H={n_heads}, D={HEAD_DIM})")
            launch("gh_attn_rows_post_forward", dev, C.byref(dims), C.byref(pm), ptr(x2), ptr(idx), ptr(a), ptr(out2), ptr(y), ptr(st2),
                   ptr(mask), what=f"gh_attn_rows_post_forward {what}")
        ctx.save_for_backward(x2, qkv, a, lse, y, st1, st2, mask, *P)
        ctx.idx, ctx.segs, ctx.cfg = idx, segs, (n_heads, eps1, eps2, norm)
        return out2

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 9
        x2, qkv, a, lse, y, st1, st2, mask, *P = ctx.saved_tensors
        idx, segs, (n_heads, eps1, eps2, norm) = ctx.idx, ctx.segs, ctx.cfg
        dev, f = x2.device, x2.shape[1]
        HD, hid, Vt = P[0].shape[0], P[12].shape[0], qkv.shape[0]
        g = g.float().reshape(-1, f)
        if g.stride(1) != 1 or (g.shape[0] > 1 and g.stride(0) < f):
            g = g.contiguous()
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dx = new(x2.shape[0], f) if idx is None else g.clone(memory_format=torch.contiguous_format)
        if Vt > 0:
            dims = _abi.GhAttnRowsDims(Vt, f, n_heads, hid, eps1, eps2, _row_stride(x2), f, _row_stride(g), f)
            pm = struct(_abi.GhAttnRowsParams, P)
            nbytes = int(lib().gh_attn_rows_workspace_bytes(C.byref(dims)))
            ws, da, dq, dk, dv = workspace(nbytes, dev), new(Vt, HD), new(Vt, HD), new(Vt, HD), new(Vt, HD)
            what = f"(V={Vt}, F={f}, H={n_heads}, hid={hid})"
            launch("gh_attn_rows_post_backward", dev, C.byref(dims), C.byref(pm), ptr(g), ptr(idx), ptr(y), ptr(st2), ptr(mask), ptr(da),
                   ptr(ws), nbytes, what=f"gh_attn_rows_post_backward {what}")
            for off, BS, V in segs:
                cd = _abi.GhAttnDims(BS, V, n_heads, HEAD_DIM, norm)
                cbytes = int(lib().gh_attn_workspace_bytes(C.byref(cd)))
                cws = workspace(cbytes, dev)
                tq, tk, tv = (_window(qkv, off, BS, V, HD, 3 * HD, c * HD) for c in range(3))
                tg = _window(da, off, BS, V, HD, HD)
                launch("gh_attn_backward", dev, C.byref(cd), C.byref(tq), C.byref(tk), C.byref(tv), _at(a, off * HD), _at(lse, off * n_heads),
                       C.byref(tg), _at(dq, off * HD), _at(dk, off * HD), _at(dv, off * HD), ptr(cws), cbytes,
                       what=f"gh_attn_backward (BS={BS}, V={V}, H={n_heads}, D={HEAD_DIM})")
            launch("gh_attn_rows_pre_backward", dev, C.byref(dims), C.byref(pm), ptr(x2), ptr(idx), ptr(st1), ptr(dq), ptr(dk), ptr(dv),
                   ptr(ws), nbytes, ptr(dx), what=f"gh_attn_rows_pre_backward {what}")
        return (dx,) + (None,) * 8


def _rows2(x: torch.Tensor) -> torch.Tensor:
    """(B, N, F) as (B N, F) rows the kernels read in place: contiguous, or one batch element with unit column stride and any row
    stride >= F; anything else is copied once."""
    B, N, f = x.shape
    if B == 1 and (f == 1 or x.stride(2) == 1) and (N <= 1 or x.stride(1) >= f):
        return x[0]                                                  # a column window of a wider tensor stays where it is
    return x.contiguous().view(B * N, f)


def _row_stride(t: torch.Tensor) -> int:
    return int(t.stride(-2)) if t.shape[-2] > 1 else int(t.shape[-1])


def _frozen(P) -> bool:
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in P))


def _kernel_ok(x: torch.Tensor, P: tuple, n_heads: int) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and _shapes_ok(x, P, n_heads) and _frozen(P)


def _run(x, idx, segs, P, n_heads, eps, norm, out):
    """The Function over x (B, N, F) with a flat row list; returns (B, N, F)."""
    B, N, f = x.shape
    eps1, eps2 = _eps(eps)
    norm = float(HEAD_DIM) ** 0.5 if norm is None else float(norm)
    P = tuple(t.detach().contiguous() for t in P)
    res = _AttnBlockFn.apply(_rows2(x), idx, tuple(segs), P, n_heads, eps1, eps2, norm, out)
    return res if out is not None else res.view(B, N, f)


def attn_block(x: torch.Tensor, params, *, n_heads: int = 4, eps=1e-6, norm=None, idx: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, ops: str = "fused") -> torch.Tensor:
    """x (BS, V, F) -> (BS, V, F): the whole SelfAttn.forward with dropout inactive, differentiable in x. eps: the LayerNorms' (one
    value, or a pair for the first and the feed-forward block's); norm: the scores' divisor, sqrt(32) unless given.
    idx: int32 (n,), distinct rows of the second dimension — they attend among themselves and are refined, per batch element; the other
    rows of the result copy x. The list is a set: it is sorted first, so the keys are summed in ascending row order and the result does
    not depend, in any bit, on the order in which the rows are listed. out: a contiguous float32 (BS, V, F) tensor that requires no gradient, written in the refined rows and
    returned (its other rows stay). On the kernel path no gradient reaches the parameters: it is taken only while autograd asks none of
    them for one."""
    check_ops(ops)
    P = _params(params)
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"x: expected (BS, V, F), got {tuple(getattr(x, 'shape', ()))}")
    if out is not None and (tuple(out.shape) != tuple(x.shape) or out.dtype != x.dtype or out.device != x.device or out.requires_grad
                            or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous tensor of x's shape, dtype and device that requires no gradient")
    if idx is not None and (idx.dim() != 1 or idx.dtype not in (torch.int32, torch.int64) or idx.device != x.device):
        raise ValueError("idx: expected a one-dimensional int32 tensor on x's device")
    if idx is not None:
        idx = torch.sort(idx)[0]              # the listed rows attend in ascending row order, whatever order they are listed in
    if ops == "torch" or not _kernel_ok(x, P, n_heads):
        return attn_block_ref(x, P, n_heads=n_heads, eps=eps, norm=norm, idx=idx, out=out)
    BS, N, _ = x.shape
    if BS * n_heads > _abi.GH_ATTN_MAX_BH or BS * N >= 2 ** 31:
        raise ValueError(f"attn_block: BS * H = {BS * n_heads} (limit {_abi.GH_ATTN_MAX_BH}) or BS * V = {BS * N} is too large")
    flat, V = None, N
    if idx is not None:
        V = idx.numel()
        flat = (torch.arange(BS, device=x.device, dtype=torch.int32).unsqueeze(1) * N + idx.to(torch.int32).unsqueeze(0)).reshape(-1)
    segs = [(0, BS, V)] if BS * V > 0 else []
    return _run(x, flat, segs, P, n_heads, eps, norm, out)


# ---- the loop over the flagged rows ------------------------------------------------------------------------------------------------
def _module_cfg(m):
    """(the sixteen tensors, n_heads, (eps1, eps2), norm) of a SelfAttn module, or None where it is not built as the reference's."""
    try:
        P = module_params(m)
        if any(t is None for t in P) or int(m.d_q) != HEAD_DIM or int(m.d_v) != HEAD_DIM:
            return None
        return P, int(m.n_heads), (float(m.layer_norm.eps), float(m.ff.layer_norm.eps)), float(m.norm)
    except AttributeError:
        return None


def _dropout_active(m) -> bool:
    return bool(m.training) and any(float(getattr(d, "p", 0.0)) > 0 for d in (m.dropout1, m.dropout2, m.ff.dropout1, m.ff.dropout2))


def _module_kernel_cfg(m, x: torch.Tensor):
    """_module_cfg where the kernels apply to module m and input x (…, F), else None."""
    cfg = _module_cfg(m)
    if cfg is None or _dropout_active(m) or not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
        return None
    return cfg if _shapes_ok(x, cfg[0], cfg[1]) and _frozen(cfg[0]) else None


def _ranges(N: int, part_rows: int, n_part: int):
    """(range length, number of ranges): the reference's rule."""
    return (int(N / n_part), n_part) if N > part_rows else (N, 1)


def _refine_loop(features, flags, module, L, nr):
    """The reference's loop over `module`, on a copy of the features."""
    feat = features.clone()
    for b in range(features.shape[0]):
        if not bool(flags[b].any()):
            continue
        for p in range(nr):
            part = torch.zeros_like(flags[b])
            part[L * p:L * (p + 1)] = flags[b, L * p:L * (p + 1)]
            if not bool(part.any()):
                continue
            feat[b, part] = module(feat[b, part].unsqueeze(0)).squeeze(0)
    return feat


def refine_flagged(features: torch.Tensor, flags: torch.Tensor, module, *, part_rows: int = 30000, n_part: int = 8,
                   ops: str = "fused") -> torch.Tensor:
    """features (B, N, F), flags (B, N) or (B, N, 1), nonzero = flagged -> a new (B, N, F): the flagged rows refined by `module` (a
    SelfAttn) under the rules of renderer_one_shot.py:554-574, the other rows copies. Differentiable in the features."""
    check_ops(ops)
    if flags.dim() == 3:
        flags = flags.squeeze(-1)
    if features.dim() != 3 or tuple(flags.shape) != tuple(features.shape[:2]):
        raise ValueError(f"refine_flagged: features {tuple(features.shape)} and flags {tuple(flags.shape)} do not fit")
    flags = flags != 0
    B, N, f = features.shape
    L, nr = _ranges(N, part_rows, n_part)
    cfg = None if ops == "torch" else _module_kernel_cfg(module, features)
    if cfg is None or B * N >= 2 ** 31:
        if B * N == 0 or not bool(flags.any()):
            return features.clone()
        return _refine_loop(features, flags, module, L, nr)
    if B * N == 0 or L == 0:
        return features.clone()
    elig = flags if nr * L == N else torch.cat([flags[:, :nr * L], torch.zeros_like(flags[:, nr * L:])], dim=1)
    idx = torch.nonzero(elig.reshape(-1)).reshape(-1).to(torch.int32)
    if idx.numel() == 0:
        return features.clone()
    counts = elig[:, :nr * L].reshape(B * nr, L).sum(1).tolist()           # the one host read
    segs, off = [], 0
    for n in counts:
        if n:
            segs.append((off, 1, int(n)))
        off += int(n)
    P, n_heads, eps, norm = cfg
    return _run(features, idx, segs, P, n_heads, eps, norm, None)


# ---- the graft ---------------------------------------------------------------------------------------------------------------------
def _block_forward(self, x: torch.Tensor, before):
    cfg = _module_kernel_cfg(self, x) if isinstance(x, torch.Tensor) else None
    if cfg is None or x.shape[0] * cfg[1] > _abi.GH_ATTN_MAX_BH or x.shape[0] * x.shape[1] >= 2 ** 31:
        return before(self, x)
    P, n_heads, eps, norm = cfg
    BS, V, _ = x.shape
    return _run(x, None, [(0, BS, V)] if BS * V > 0 else [], P, n_heads, eps, norm, None)


_SEAM = (__name__, "fused_attn_block_cls")


def fused_attn_block_cls(base):
    """A subclass of the given SelfAttn class (the reference's own, or what fuse_self_attn made of it) whose forward(x) is the fused
    block while the kernels apply, and the given class's own forward, unchanged, otherwise."""
    def forward(self, x):
        return _block_forward(self, x, base.forward)

    return _seam.graft(_SEAM, base, {"forward": forward}, "attention block")


def fuse_attn_block(renderer):
    """Swap the class of `renderer.self_attn_layer` for fused_attn_block_cls of its own class. The module object, its parameters and
    its state dict are untouched; it may be called on a renderer that is already built, and again. Returns the renderer."""
    _seam.swap(_SEAM, renderer.self_attn_layer)
    return renderer
