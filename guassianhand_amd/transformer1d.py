"""The Transformer1D backbones (tgs/models/transformers.py:673-908, called at infer_one_shot.py:256-264): a GroupNorm, proj_in, a stack
of blocks — self-attention, a second attention over the same tokens where `attn2` exists, a GEGLU feed-forward, each behind a
LayerNorm and added to the stream — and proj_out back to channel-first plus the input. In HIP through include/gh_xf.h: the forward,
and opt-in the backward to the input with every weight frozen:

    transformer1d(module_or_params, x, ops="fused", grad="none")     x (B, C, N) float32 -> (B, C, N)

The kernel path is for frozen inference: one host call enqueues the whole stack (4 + 11 launches per layer), float32 throughout, no
atomics, bitwise reproducible. It runs when `kernel_reason` finds nothing against it: float32 tensors on a ROCm device outside
autocast, no gradient wanted (grad mode off, or neither x nor any parameter requires one), no encoder_hidden_states and no mask,
LayerNorm blocks with affine norms, GEGLU, no attention bias, no only_cross_attention, no gated fuser, no feed-forward chunking,
dropout inactive, and sizes the kernels take (D in {32, 64}, M = heads * D <= 1024, C a multiple of the group count and of 32,
C <= 1024). In every other case the forward is the base class's own (`fuse_transformer1d`, the config seam) or `transformer1d_ref`
(the standalone module, the function form), with every gradient.

grad="input" (the keyword of `transformer1d`, `kernel_reason`, `Transformer1D.forward`, `fused_transformer1d_cls` and
`fuse_transformer1d`) adds the case the one-shot fit needs, which trains the identity code through the frozen texture backbone: where
grad mode is on, x requires a gradient and no parameter does, the call is a torch.autograd.Function whose forward is
gh_xf_forward_tape (the same kernels, `out` bitwise the same, plus a tape of about 11 M T floats a layer) and whose backward is
gh_xf_backward: 5 + 13 launches per layer, float32, no atomics, bitwise reproducible, once differentiable. It takes M <= 512
(GH_XF_GRAD_MAX_M). A parameter that requires a gradient is the reason "a parameter wants a gradient" and the torch path; with nothing
requiring a gradient the plain untaped kernels run. grad="none", the default, is the forward-only behaviour exactly.

grad="params" adds training: where a parameter requires a gradient the call is a second torch.autograd.Function over x and the
parameter tensors, whose forward is the same gh_xf_forward_tape and whose backward is gh_xf_backward_params: gh_xf_backward's chain (dx
bitwise the same) with, beside each step, the backward-weight products, the bias sums and the norms' scale and shift sums of the
parameters that want a gradient, and of those alone. The gradients of to_q, to_k and to_v are the row blocks of one stacked gradient.
With only x requiring a gradient it is grad="input"'s function, with nothing requiring one the plain kernels; M <= 512 as there.

`transformer1d_ref(params, x, acc=None)` is the plain-torch restatement with an explicit softmax, so that it runs in float64 (the
yardstick of the GPU tests); it is written from transformers.py and the attribute layout of diffusers' Attention and is not pinned
against a recorded run of the reference. `params_of(module)` reads the nested parameter dict off any module with that layout.
`Transformer1D` is the module standalone with the reference's state-dict keys. `fuse_transformer1d(module)` swaps a built module's
class for `fused_transformer1d_cls` of its own class; the concatenated [Wq; Wk; Wv] are cached per module and rebuilt when a
parameter's version counter (or storage) changes, and so are the transposed copies the backward's data products read, built when a
backward first needs them; `refresh(module)` drops them by hand. `linear`, `group_moments` and `attention` are the forward's single
launches; `attention_lse`, `attention_backward`, `geglu_backward`, `layernorm_backward` and `group_norm_backward` the backward's;
`linear_wgrad`, `layernorm_param_grads` and `group_norm_param_grads` those of the parameters' gradients."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi, _seam
from ._call import check_ops, cotangent, launch, lib, ptr, row_stride, rows, workspace

HEAD_DIMS = (32, 64)
MAX_M, MAX_C, MAX_T, GRAD_MAX_M = _abi.GH_XF_MAX_M, _abi.GH_XF_MAX_C, _abi.GH_XF_MAX_T, _abi.GH_XF_GRAD_MAX_M
GRADS = ("none", "input", "params")
PROLOGUES = {"none": _abi.GH_XF_PRO_NONE, "ln": _abi.GH_XF_PRO_LN, "gn": _abi.GH_XF_PRO_GN, "cf": _abi.GH_XF_PRO_CF}
EPILOGUES = {"plain": _abi.GH_XF_EPI_PLAIN, "bias_res": _abi.GH_XF_EPI_BIAS_RES, "geglu": _abi.GH_XF_EPI_GEGLU,
             "bias_res_cf": _abi.GH_XF_EPI_BIAS_RES_CF}
GN_EPS, LN_EPS = 1e-6, 1e-5


def sizes_supported(C_: int, G: int, heads: int, D: int) -> bool:
    return D in HEAD_DIMS and 1 <= heads and heads * D <= MAX_M and 1 <= G and C_ % G == 0 and C_ % 32 == 0 and 32 <= C_ <= MAX_C


# ---- the parameters as a nested dict -----------------------------------------------------------------------------------------------
def _attn_params(a):
    return {"q": a.to_q.weight, "k": a.to_k.weight, "v": a.to_v.weight, "o_w": a.to_out[0].weight, "o_b": a.to_out[0].bias,
            "q_b": a.to_q.bias, "k_b": a.to_k.bias, "v_b": a.to_v.bias}


def params_of(module) -> dict:
    """{"groups", "heads", "gn_eps", "norm": (w, b), "proj_in": (w, b), "proj_out": (w, b), "blocks": [{"norm1", "attn1", "norm2",
    "attn2" (None where absent), "norm3", "ff1": (w, b), "ff2": (w, b), "ln_eps"}]} of a module with the reference's attribute
    layout. The tensors are the module's own parameters."""
    blocks = []
    for b in module.transformer_blocks:
        has2 = getattr(b, "attn2", None) is not None
        blocks.append({"norm1": (b.norm1.weight, b.norm1.bias), "attn1": _attn_params(b.attn1),
                       "norm2": (b.norm2.weight, b.norm2.bias) if has2 else None, "attn2": _attn_params(b.attn2) if has2 else None,
                       "norm3": (b.norm3.weight, b.norm3.bias), "ff1": (b.ff.net[0].proj.weight, b.ff.net[0].proj.bias),
                       "ff2": (b.ff.net[2].weight, b.ff.net[2].bias), "ln_eps": float(b.norm1.eps)})
    heads = int(module.transformer_blocks[0].attn1.heads) if len(module.transformer_blocks) else int(module.num_attention_heads)
    return {"groups": int(module.norm.num_groups), "heads": heads, "gn_eps": float(module.norm.eps), "norm": (module.norm.weight, module.norm.bias),
            "proj_in": (module.proj_in.weight, module.proj_in.bias), "proj_out": (module.proj_out.weight, module.proj_out.bias), "blocks": blocks}


def _tensors(params):
    """Every tensor of a parameter dict, in a fixed order."""
    out = [*params["norm"], *params["proj_in"], *params["proj_out"]]
    for b in params["blocks"]:
        for k in ("norm1", "norm2", "norm3", "ff1", "ff2"):
            if b[k] is not None:
                out += list(b[k])
        for k in ("attn1", "attn2"):
            if b[k] is not None:
                out += [t for t in b[k].values() if t is not None]
    return [t for t in out if t is not None]


def _map(params, f):
    g = lambda t: None if t is None else f(t)
    pair = lambda p: None if p is None else (g(p[0]), g(p[1]))
    att = lambda a: None if a is None else {k: g(v) for k, v in a.items()}
    out = dict(params, norm=pair(params["norm"]), proj_in=pair(params["proj_in"]), proj_out=pair(params["proj_out"]))
    out["blocks"] = [dict(b, norm1=pair(b["norm1"]), norm2=pair(b["norm2"]), norm3=pair(b["norm3"]), ff1=pair(b["ff1"]), ff2=pair(b["ff2"]),
                          attn1=att(b["attn1"]), attn2=att(b["attn2"])) for b in params["blocks"]]
    return out


# ---- plain-torch restatement ---------------------------------------------------------------------------------------------------------
def _mask_bias(mask, dtype):
    """The reference's conversion (transformers.py:845-858): a 2-D keep mask becomes an additive bias with a query dimension."""
    if mask is not None and mask.ndim == 2:
        mask = ((1 - mask.to(dtype)) * -10000.0).unsqueeze(1)
    return mask


def _attention_ref(h, a, heads, ctx=None, bias=None):
    B, N, M = h.shape
    ctx = h if ctx is None else ctx
    D = M // heads
    split = lambda t: t.reshape(B, -1, heads, D).transpose(1, 2)
    q, k, v = split(F.linear(h, a["q"], a.get("q_b"))), split(F.linear(ctx, a["k"], a.get("k_b"))), split(F.linear(ctx, a["v"], a.get("v_b")))
    s = torch.matmul(q, k.transpose(-1, -2)) * (D ** -0.5)
    if bias is not None:
        s = s + bias.to(s.dtype)[:, None]
    o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, N, M)
    return F.linear(o, a["o_w"], a["o_b"])


def transformer1d_ref(params, x, acc: Optional[torch.dtype] = None, *, encoder_hidden_states=None, attention_mask=None,
                      encoder_attention_mask=None):
    """The module's statements in plain torch, differentiable with respect to everything: F.group_norm, F.layer_norm, F.linear, an
    explicit softmax over (q k^T) * D^-0.5, the exact-erf GELU. acc=torch.float64 computes (and returns) in double."""
    if acc is not None:
        params, x = _map(params, lambda t: t.to(acc)), x.to(acc)
        encoder_hidden_states = None if encoder_hidden_states is None else encoder_hidden_states.to(acc)
    heads = params["heads"]
    bias1, bias2 = _mask_bias(attention_mask, x.dtype), _mask_bias(encoder_attention_mask, x.dtype)
    B, Cc, N = x.shape
    h = F.group_norm(x, params["groups"], *params["norm"], eps=params.get("gn_eps", GN_EPS))
    h = F.linear(h.permute(0, 2, 1).reshape(B, N, Cc), *params["proj_in"])
    M = h.shape[-1]
    for b in params["blocks"]:
        eps = b.get("ln_eps", LN_EPS)
        h = h + _attention_ref(F.layer_norm(h, (M,), *b["norm1"], eps=eps), b["attn1"], heads, None, bias1)
        if b["attn2"] is not None:
            h = h + _attention_ref(F.layer_norm(h, (M,), *b["norm2"], eps=eps), b["attn2"], heads, encoder_hidden_states, bias2)
        a, g = F.linear(F.layer_norm(h, (M,), *b["norm3"], eps=eps), *b["ff1"]).chunk(2, dim=-1)
        h = h + F.linear(a * F.gelu(g), *b["ff2"])
    h = F.linear(h, *params["proj_out"])
    return h.reshape(B, N, Cc).permute(0, 2, 1).contiguous() + x


# ---- the single launches ---------------------------------------------------------------------------------------------------------------
def group_moments(x: torch.Tensor, groups: int) -> torch.Tensor:
    """x (B, C, N) float32 on the device, unit stride along N -> (B, groups, 2): the mean and the sum of squared deviations."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"group_moments: expected a (B, C, N) float32 device tensor, got {tuple(x.shape)} {x.dtype} on {x.device}")
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    B, Cc, N = x.shape
    out = torch.empty(B, groups, 2, dtype=torch.float32, device=x.device)
    nbytes = int(lib().gh_xf_group_moments_workspace_bytes(B, Cc, N, groups))
    ws = workspace(nbytes, x.device)
    launch("gh_xf_group_moments", x.device, ptr(x), int(x.stride(0)), int(x.stride(1)), B, Cc, N, groups, ptr(out), ptr(ws), nbytes,
           detail=f" (B={B}, C={Cc}, N={N}, G={groups})")
    return out


def linear(x, w, *, prologue="none", epilogue="plain", bias=None, gamma=None, beta=None, eps=LN_EPS, moments=None, groups=0, res=None,
           rows_per_batch=0):
    """One gh_xf_linear call. x: (T, K) rows read in place through their row stride, or under prologue="gn" and "cf" the
    channel-first (B, K, N). dX = dY W is linear(dY, W.t().contiguous()). Returns (T, N_out), or under epilogue="bias_res_cf" the channel-first (B, N_out, N) (res likewise)."""
    pro, epi = PROLOGUES[prologue], EPILOGUES[epilogue]
    a = _abi.GhXfLinear()
    keep = [w.contiguous()]
    if prologue in ("gn", "cf"):
        if x.shape[2] > 1 and x.stride(2) != 1:
            x = x.contiguous()
        B, K, N = x.shape
        T, rows_per_batch = B * N, N
        a.x_stride, a.x_stride_b = int(x.stride(1)), int(x.stride(0))
    else:
        x = rows(x)
        T, K = x.shape
        a.x_stride = row_stride(x)
    n_out = w.shape[0] // 2 if epilogue == "geglu" else w.shape[0]
    dev = x.device
    if epilogue == "bias_res_cf":
        B = T // rows_per_batch if rows_per_batch else 0
        y = torch.empty(B, n_out, rows_per_batch, dtype=torch.float32, device=dev)
        a.y_stride, a.y_stride_b = rows_per_batch, n_out * rows_per_batch
        if res is not None:
            res = res.contiguous()
            a.res_stride, a.res_stride_b = rows_per_batch, n_out * rows_per_batch
    else:
        y = torch.empty(T, n_out, dtype=torch.float32, device=dev)
        a.y_stride = n_out
        if res is not None:
            res = rows(res)
            a.res_stride = row_stride(res)
    for t in (bias, gamma, beta, moments):
        keep.append(None if t is None else t.contiguous())
    a.T, a.K, a.N_out, a.prologue, a.epilogue, a.rows_per_batch, a.groups, a.eps = T, K, n_out, pro, epi, int(rows_per_batch), int(groups), float(eps)
    a.x, a.w, a.y = x.data_ptr(), keep[0].data_ptr(), y.data_ptr()
    a.bias, a.gamma, a.beta, a.moments = (None if t is None else t.data_ptr() for t in keep[1:])
    a.res = None if res is None else res.data_ptr()
    nbytes = int(lib().gh_xf_linear_workspace_bytes(T, pro))
    ws = workspace(nbytes, dev)
    launch("gh_xf_linear", dev, C.byref(a), ptr(ws), nbytes, detail=f" (T={T}, K={K}, N_out={n_out}, {prologue}, {epilogue})")
    return y


def attention(qkv: torch.Tensor, B: int, N: int, heads: int, D: int) -> torch.Tensor:
    """qkv (B N, 3 heads D) rows read in place -> (B N, heads D): softmax(q k^T D^-0.5) v per (batch, head)."""
    qkv = rows(qkv)
    out = torch.empty(B * N, heads * D, dtype=torch.float32, device=qkv.device)
    launch("gh_xf_attention", qkv.device, ptr(qkv), row_stride(qkv), B, N, heads, D, ptr(out), heads * D,
           detail=f" (B={B}, N={N}, heads={heads}, D={D})")
    return out


# ---- the single launches of the backward ---------------------------------------------------------------------------------------------
def gelu_grad(g: torch.Tensor) -> torch.Tensor:
    """gelu'(g) as the kernels state it: 0.5 (1 + erf(g * 0.70710678)) + g * 0.39894228 * exp(-0.5 g^2)."""
    return 0.5 * (1 + torch.erf(g * 0.70710678)) + g * 0.39894228 * torch.exp(-0.5 * g * g)


def attention_lse(qkv: torch.Tensor, B: int, N: int, heads: int, D: int):
    """`attention` that also returns lse (B, heads, N), the logarithm of each query's sum of exp((q.k) D^-0.5)."""
    qkv = rows(qkv)
    out = torch.empty(B * N, heads * D, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, heads, N, dtype=torch.float32, device=qkv.device)
    launch("gh_xf_attention_lse", qkv.device, ptr(qkv), row_stride(qkv), B, N, heads, D, ptr(out), heads * D, ptr(lse),
           detail=f" (B={B}, N={N}, heads={heads}, D={D})")
    return out, lse


def attention_backward(qkv, out, lse, dout, B: int, N: int, heads: int, D: int, dqkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dqkv (B N, 3 heads D) = [dq | dk | dv] for the cotangent dout (B N, heads D) of `attention_lse`'s out; qkv and dout are read
    in place. dqkv: a buffer to write into (its rows past B N stay as they are)."""
    qkv, out, dout = rows(qkv), rows(out), rows(dout)
    if dqkv is None:
        dqkv = torch.empty(B * N, 3 * heads * D, dtype=torch.float32, device=qkv.device)
    nbytes = int(lib().gh_xf_attention_backward_workspace_bytes(B, N, heads))
    ws = workspace(nbytes, qkv.device)
    launch("gh_xf_attention_backward", qkv.device, ptr(qkv), row_stride(qkv), ptr(out), row_stride(out), ptr(lse.contiguous()), ptr(dout),
           row_stride(dout), B, N, heads, D, ptr(dqkv), 3 * heads * D, ptr(ws), nbytes, detail=f" (B={B}, N={N}, heads={heads}, D={D})")
    return dqkv


def geglu_backward(g, h, moments, gamma, beta, w1, b1, w2t) -> torch.Tensor:
    """[da | dg] (T, 8M) of the feed-forward: g (T, M) the cotangent of its output, h (T, M) its input with the LayerNorm's row
    moments (T, 2) {mean, rstd}, w1 (8M, M), b1 (8M), w2t (4M, M) = W2.t()."""
    g, h = rows(g), rows(h)
    T, M = h.shape
    y = torch.empty(T, 8 * M, dtype=torch.float32, device=h.device)
    keep = [t.contiguous() for t in (moments, gamma, beta, w1, b1, w2t)]
    launch("gh_xf_geglu_backward", h.device, ptr(g), row_stride(g), ptr(h), row_stride(h), *[ptr(t) for t in keep], T, M, ptr(y), 8 * M,
           detail=f" (T={T}, M={M})")
    return y


def layernorm_backward(dn, x, moments, gamma, g) -> torch.Tensor:
    """g (T, K) += the LayerNorm's backward of dn (T, K) at x (T, K) with row moments (T, 2) {mean, rstd}, in place. Returns g."""
    dn, x = rows(dn), rows(x)
    T, K = x.shape
    if not g.is_contiguous():
        raise ValueError("layernorm_backward: g is updated in place and must be contiguous")
    keep = [moments.contiguous(), gamma.contiguous()]
    launch("gh_xf_layernorm_backward", x.device, ptr(dn), row_stride(dn), ptr(x), row_stride(x), ptr(keep[0]), ptr(keep[1]), T, K, ptr(g), K,
           detail=f" (T={T}, K={K})")
    return g


def group_norm_backward(dy, x, moments, gamma, dout, groups: int, eps: float = GN_EPS) -> torch.Tensor:
    """dx (B, C, N) = dout + the GroupNorm's backward of dy at x, with `group_moments`' moments (B, groups, 2)."""
    dy, x, dout = dy.contiguous(), x.contiguous(), dout.contiguous()
    B, Cc, N = x.shape
    dx = torch.empty_like(x)
    nbytes = int(lib().gh_xf_group_norm_backward_workspace_bytes(B, Cc, N, groups))
    ws = workspace(nbytes, x.device)
    keep = [moments.contiguous(), gamma.contiguous()]
    launch("gh_xf_group_norm_backward", x.device, ptr(dy), ptr(x), ptr(keep[0]), ptr(keep[1]), ptr(dout), ptr(dx), B, Cc, N, groups, float(eps),
           ptr(ws), nbytes, detail=f" (B={B}, C={Cc}, N={N}, G={groups})")
    return dx


# ---- the single launches of the parameters' gradients ---------------------------------------------------------------------------------
def linear_wgrad_chunk(T: int, K: int, n_out: int) -> int:
    """Rows per chunk of `linear_wgrad`'s split of T: a function of the three sizes alone."""
    return int(lib().gh_xf_linear_wgrad_chunk(int(T), int(K), int(n_out)))


def linear_wgrad(dy, x, *, prologue="none", gamma=None, beta=None, eps=GN_EPS, moments=None, groups=0, want_w=True, want_b=True):
    """One gh_xf_linear_wgrad call: (dW (N_out, K), db (N_out)) = (dY^T P(X), the column sums of dY) over the T rows; either is None
    where not wanted. x: (T, K) rows read in place, or under prologue="gn" and "cf" the channel-first (B, K, N); dy: (T, N_out) rows
    read in place, or a 3-D channel-first (B, N_out, N). moments: the (T, 2) {mean, rstd} rows under "ln", `group_moments`' under "gn"."""
    a = _abi.GhXfWgrad()
    rpb = 0
    if prologue in ("gn", "cf"):
        if x.shape[2] > 1 and x.stride(2) != 1:
            x = x.contiguous()
        B, K, N = x.shape
        T, rpb = B * N, N
        a.x_stride, a.x_stride_b = int(x.stride(1)), int(x.stride(0))
    else:
        x = rows(x)
        T, K = x.shape
        a.x_stride = row_stride(x)
    if dy.dim() == 3:
        if dy.shape[2] > 1 and dy.stride(2) != 1:
            dy = dy.contiguous()
        n_out, rpb = dy.shape[1], dy.shape[2]
        a.dy_cf, a.dy_stride, a.dy_stride_b = 1, int(dy.stride(1)), int(dy.stride(0))
    else:
        dy = rows(dy)
        n_out = dy.shape[1]
        a.dy_stride = row_stride(dy)
    dev = x.device
    dw = torch.empty(n_out, K, dtype=torch.float32, device=dev) if want_w else None
    db = torch.empty(n_out, dtype=torch.float32, device=dev) if want_b else None
    if T == 0:
        return (None if dw is None else dw.zero_()), (None if db is None else db.zero_())
    keep = [None if t is None else t.contiguous() for t in (gamma, beta, moments)]
    a.T, a.K, a.N_out, a.prologue, a.rows_per_batch, a.groups, a.eps = T, K, n_out, PROLOGUES[prologue], int(rpb), int(groups), float(eps)
    a.x, a.dy = x.data_ptr(), dy.data_ptr()
    a.gamma, a.beta, a.moments = (None if t is None else t.data_ptr() for t in keep)
    a.dw, a.db = (None if t is None else t.data_ptr() for t in (dw, db))
    nbytes = int(lib().gh_xf_linear_wgrad_workspace_bytes(T, K, n_out))
    ws = workspace(nbytes, dev)
    launch("gh_xf_linear_wgrad", dev, C.byref(a), ptr(ws), nbytes, detail=f" (T={T}, K={K}, N_out={n_out}, {prologue})")
    return dw, db


def layernorm_param_grads(dn, x, moments):
    """(dgamma, dbeta) (K) of a LayerNorm whose output's cotangent is dn (T, K), at x (T, K) with row moments (T, 2) {mean, rstd}."""
    dn, x = rows(dn), rows(x)
    T, K = x.shape
    dg, db = torch.zeros(K, dtype=torch.float32, device=x.device), torch.zeros(K, dtype=torch.float32, device=x.device)
    nbytes = int(lib().gh_xf_layernorm_param_grads_workspace_bytes(T, K))
    ws, mom = workspace(nbytes, x.device), moments.contiguous()
    launch("gh_xf_layernorm_param_grads", x.device, ptr(dn), row_stride(dn), ptr(x), row_stride(x), ptr(mom), T, K, ptr(dg), ptr(db), ptr(ws),
           nbytes, detail=f" (T={T}, K={K})")
    return dg, db


def group_norm_param_grads(dy, x, moments, groups: int, eps: float = GN_EPS):
    """(dgamma, dbeta) (C) of the GroupNorm whose output's cotangent is dy (B, C, N), at x with `group_moments`' moments."""
    dy, x = dy.contiguous(), x.contiguous()
    B, Cc, N = x.shape
    dg, db = torch.zeros(Cc, dtype=torch.float32, device=x.device), torch.zeros(Cc, dtype=torch.float32, device=x.device)
    nbytes = int(lib().gh_xf_group_norm_param_grads_workspace_bytes(B, Cc, N, groups))
    ws, mom = workspace(nbytes, x.device), moments.contiguous()
    launch("gh_xf_group_norm_param_grads", x.device, ptr(dy), ptr(x), ptr(mom), B, Cc, N, groups, float(eps), ptr(dg), ptr(db), ptr(ws), nbytes,
           detail=f" (B={B}, C={Cc}, N={N}, G={groups})")
    return dg, db


# ---- the whole stack ------------------------------------------------------------------------------------------------------------------
class _Packed:
    """The parameters as gh_xf_forward reads them: contiguous float32 tensors (kept alive here), the concatenated [Wq; Wk; Wv], and
    the ctypes structs that point at them. `transposed()` adds, on first use, what gh_xf_backward reads: the transposed copies of the
    backward-data products."""

    def __init__(self, params):
        self.keep = []
        self.fields = []                                         # per layer: GhXfLayer's field name -> the tensor it points at
        self._t = None
        self._stem_w = [t.detach().contiguous() for t in (params["norm"][0], params["proj_in"][0], params["proj_out"][0])]
        c = self._c
        self.stem = _abi.GhXfStem(*[c(t) for t in (*params["norm"], *params["proj_in"], *params["proj_out"])])
        self.n_layers = len(params["blocks"])
        self.layers = (_abi.GhXfLayer * max(self.n_layers, 1))()
        for i, b in enumerate(params["blocks"]):
            a1, a2 = b["attn1"], b["attn2"]
            f = {"ln1_w": b["norm1"][0], "ln1_b": b["norm1"][1], "qkv1": torch.cat([a1["q"], a1["k"], a1["v"]], dim=0), "o1_w": a1["o_w"],
                 "o1_b": a1["o_b"], "ln3_w": b["norm3"][0], "ln3_b": b["norm3"][1], "ff1_w": b["ff1"][0], "ff1_b": b["ff1"][1],
                 "ff2_w": b["ff2"][0], "ff2_b": b["ff2"][1]}
            if a2 is not None:
                f.update(ln2_w=b["norm2"][0], ln2_b=b["norm2"][1], qkv2=torch.cat([a2["q"], a2["k"], a2["v"]], dim=0), o2_w=a2["o_w"], o2_b=a2["o_b"])
            f = {k: v.detach().contiguous() for k, v in f.items()}
            self.fields.append(f)
            for name in _abi.XF_LAYER:
                setattr(self.layers[i], name, c(f[name]) if name in f else None)
        self.groups, self.heads = params["groups"], params["heads"]
        self.C, self.M = params["proj_in"][0].shape[1], params["proj_in"][0].shape[0]
        self.gn_eps = float(params.get("gn_eps", GN_EPS))
        self.ln_eps = float(params["blocks"][0].get("ln_eps", LN_EPS)) if params["blocks"] else LN_EPS

    def _c(self, t):
        t = t.detach().contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def transposed(self):
        """(GhXfStemT, GhXfLayerT array) for gh_xf_backward; the copies are made once and kept here."""
        if self._t is None:
            tr = lambda w: self._c(w.t())
            gn_w, in_w, out_w = self._stem_w
            stem = _abi.GhXfStemT(self._c(gn_w), tr(in_w), tr(out_w))
            layers = (_abi.GhXfLayerT * max(self.n_layers, 1))()
            for i, f in enumerate(self.fields):
                v = {"ln1_w": self._c(f["ln1_w"]), "qkv1_t": tr(f["qkv1"]), "o1_t": tr(f["o1_w"]), "ln3_w": self._c(f["ln3_w"]),
                     "ln3_b": self._c(f["ln3_b"]), "ff1_w": self._c(f["ff1_w"]), "ff1_b": self._c(f["ff1_b"]), "ff1_t": tr(f["ff1_w"]),
                     "ff2_t": tr(f["ff2_w"])}
                if "qkv2" in f:
                    v.update(ln2_w=self._c(f["ln2_w"]), qkv2_t=tr(f["qkv2"]), o2_t=tr(f["o2_w"]))
                for name in _abi.XF_LAYER_T:
                    setattr(layers[i], name, v.get(name))
            self._t = (stem, layers)
        return self._t


def _run(packed: _Packed, x: torch.Tensor) -> torch.Tensor:
    B, Cc, N = x.shape
    x = x.detach().contiguous()
    out = torch.empty_like(x)
    if B == 0 or N == 0:
        return out
    dims = _dims(packed, x)
    nbytes = int(lib().gh_xf_workspace_bytes(C.byref(dims)))
    ws = workspace(nbytes, x.device)
    launch("gh_xf_forward", x.device, C.byref(dims), C.byref(packed.stem), packed.layers, ptr(x), ptr(out), ptr(ws), nbytes, detail=_detail(packed, x))
    return out


def _dims(packed: _Packed, x) -> "_abi.GhXfDims":
    B, Cc, N = x.shape
    return _abi.GhXfDims(B, Cc, N, packed.groups, packed.heads, packed.M // packed.heads, packed.n_layers, packed.gn_eps, packed.ln_eps)


def _detail(packed: _Packed, x) -> str:
    B, Cc, N = x.shape
    return f" (B={B}, C={Cc}, N={N}, heads={packed.heads}, D={packed.M // packed.heads}, layers={packed.n_layers})"


def _run_tape(packed: _Packed, x: torch.Tensor):
    """gh_xf_forward_tape: (out, the tape as a uint8 tensor)."""
    out = torch.empty_like(x)
    dims = _dims(packed, x)
    nbytes, tbytes = int(lib().gh_xf_workspace_bytes(C.byref(dims))), int(lib().gh_xf_tape_bytes(C.byref(dims)))
    ws, tape = workspace(nbytes, x.device), workspace(tbytes, x.device)
    launch("gh_xf_forward_tape", x.device, C.byref(dims), C.byref(packed.stem), packed.layers, ptr(x), ptr(out), ptr(tape), tbytes, ptr(ws), nbytes,
           detail=_detail(packed, x))
    return out, tape


def _run_backward(packed: _Packed, x: torch.Tensor, tape: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    dx = torch.empty_like(x)
    dims = _dims(packed, x)
    stem, layers = packed.transposed()
    nbytes = int(lib().gh_xf_backward_workspace_bytes(C.byref(dims)))
    ws = workspace(nbytes, x.device)
    launch("gh_xf_backward", x.device, C.byref(dims), C.byref(stem), layers, ptr(x), ptr(tape), ptr(dout), ptr(dx), ptr(ws), nbytes,
           detail=_detail(packed, x))
    return dx


def _grad_slots(params):
    """Parallel to `_tensors(params)`: where each tensor's gradient lies among gh_xf_backward_params' buffers, as (layer index or None
    for the stem, the GhXfStemG / GhXfLayerG field, the row block of a stacked [Wq; Wk; Wv] gradient or None)."""
    out = [(None, n, None) for n in _abi.XF_STEM]
    for i, b in enumerate(params["blocks"]):
        for k, names in (("norm1", ("ln1_w", "ln1_b")), ("norm2", ("ln2_w", "ln2_b")), ("norm3", ("ln3_w", "ln3_b")), ("ff1", ("ff1_w", "ff1_b")),
                         ("ff2", ("ff2_w", "ff2_b"))):
            if b[k] is not None:
                out += [(i, n, None) for n in names]
        for k, n in (("attn1", "1"), ("attn2", "2")):
            if b[k] is not None:
                out += [(i, "qkv" + n, 0), (i, "qkv" + n, 1), (i, "qkv" + n, 2), (i, f"o{n}_w", None), (i, f"o{n}_b", None)]
    return out


def _run_backward_params(packed: _Packed, x, tape, dout, slots, shapes, needs, want_dx: bool):
    """gh_xf_backward_params: (dx or None, the gradients parallel to `slots`, None where `needs` says so). Buffers exist only for what
    is wanted; the three attention weights share one stacked buffer."""
    dims = _dims(packed, x)
    stem_t, layers_t = packed.transposed()
    M, dev = packed.M, x.device
    bufs = {}
    for (layer, field, block), shape, need in zip(slots, shapes, needs):
        if need and (layer, field) not in bufs:
            bufs[(layer, field)] = torch.empty((3 * M, M) if block is not None else shape, dtype=torch.float32, device=dev)
    gstem = _abi.GhXfStemG(*[bufs[(None, n)].data_ptr() if (None, n) in bufs else None for n in _abi.XF_STEM])
    glayers = (_abi.GhXfLayerG * max(packed.n_layers, 1))()
    for (layer, field), t in bufs.items():
        if layer is not None:
            setattr(glayers[layer], field, t.data_ptr())
    dx = torch.empty_like(x) if want_dx else None
    nbytes = int(lib().gh_xf_backward_params_workspace_bytes(C.byref(dims)))
    ws = workspace(nbytes, dev)
    launch("gh_xf_backward_params", dev, C.byref(dims), C.byref(stem_t), layers_t, C.byref(packed.stem), packed.layers, C.byref(gstem), glayers,
           ptr(x), ptr(tape), ptr(dout), ptr(dx), ptr(ws), nbytes, detail=_detail(packed, x))
    grads = []
    for (layer, field, block), need in zip(slots, needs):
        t = bufs[(layer, field)] if need else None
        grads.append(t if t is None or block is None else t[block * M:(block + 1) * M])
    return dx, grads


class _ParamGrad(torch.autograd.Function):
    """The stack with its backward to x and to every parameter that wants a gradient: gh_xf_forward_tape, then gh_xf_backward_params.
    The inputs behind `packed` are the parameter tensors in `_tensors` order."""

    @staticmethod
    def forward(ctx, x, packed, slots, *tensors):
        xc = x.detach().contiguous()
        ctx.packed, ctx.slots, ctx.shapes = packed, slots, [tuple(t.shape) for t in tensors]
        if xc.shape[0] == 0 or xc.shape[2] == 0:
            ctx.save_for_backward(xc)
            return torch.empty_like(xc)
        out, tape = _run_tape(packed, xc)
        ctx.save_for_backward(xc, tape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        needs = ctx.needs_input_grad
        xc = ctx.saved_tensors[0]
        if len(ctx.saved_tensors) == 1:
            zeros = [torch.zeros(s, dtype=torch.float32, device=xc.device) if n else None for s, n in zip(ctx.shapes, needs[3:])]
            return (torch.zeros_like(xc) if needs[0] else None, None, None, *zeros)
        dx, grads = _run_backward_params(ctx.packed, xc, ctx.saved_tensors[1], cotangent(dout), ctx.slots, ctx.shapes, needs[3:], needs[0])
        return (dx, None, None, *grads)


class _InputGrad(torch.autograd.Function):
    """The stack with its backward to x: gh_xf_forward_tape, then gh_xf_backward. The weights are constants."""

    @staticmethod
    def forward(ctx, x, packed):
        xc = x.detach().contiguous()
        ctx.packed = packed
        if xc.shape[0] == 0 or xc.shape[2] == 0:
            ctx.save_for_backward(xc)
            return torch.empty_like(xc)
        out, tape = _run_tape(packed, xc)
        ctx.save_for_backward(xc, tape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        if len(ctx.saved_tensors) == 1:
            return torch.zeros_like(ctx.saved_tensors[0]), None
        xc, tape = ctx.saved_tensors
        return _run_backward(ctx.packed, xc, tape, cotangent(dout)), None


def _go(packed: _Packed, x: torch.Tensor, grad: str, params=None) -> torch.Tensor:
    """The kernels for a call kernel_reason let through: plain where nothing wants a gradient, taped with the backward to x where x
    alone does, taped with the parameters' backward (grad="params") where a parameter does."""
    if grad != "none" and torch.is_grad_enabled():
        if grad == "params" and params is not None:
            ts = _tensors(params)
            if any(t.requires_grad for t in ts):
                return _ParamGrad.apply(x, packed, _grad_slots(params), *ts)
        if x.requires_grad:
            return _InputGrad.apply(x, packed)
    return _run(packed, x)


def _check_grad(grad: str) -> None:
    if grad not in GRADS:
        raise ValueError(f"grad must be one of {', '.join(repr(g) for g in GRADS)}, got {grad!r}")


def _params_reason(params, x, grad: str = "none") -> Optional[str]:
    """Why the kernels cannot run these parameters on x, or None."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 3):
        return "x is not a (B, C, N) tensor"
    if not x.is_cuda:
        return "x is not on a ROCm device"
    if torch.is_autocast_enabled():
        return "autocast is on"
    ts = _tensors(params)
    if x.dtype != torch.float32 or any(t.dtype != torch.float32 or t.device != x.device for t in ts):
        return "not float32 on one device"
    taped = False
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in ts)):
        if grad == "none":
            return "a gradient is wanted"
        if grad != "params" and any(t.requires_grad for t in ts):
            return "a parameter wants a gradient"
        taped = True
    M, Cin = params["proj_in"][0].shape
    if taped and M > GRAD_MAX_M:
        return "sizes"
    heads = params["heads"]
    if heads < 1 or M % heads != 0 or not sizes_supported(Cin, params["groups"], heads, M // heads) or x.shape[1] != Cin:
        return "sizes"
    if x.shape[0] * x.shape[2] > MAX_T or tuple(params["proj_out"][0].shape) != (Cin, M):
        return "sizes"
    if any(t is None for t in (*params["norm"], *params["proj_in"], *params["proj_out"])):
        return "a norm without affine parameters or a projection without bias"
    eps = {b.get("ln_eps", LN_EPS) for b in params["blocks"]}
    if len(eps) > 1:
        return "blocks with different LayerNorm eps"
    for b in params["blocks"]:
        for a, n in ((b["attn1"], b["norm1"]), (b["attn2"], b["norm2"])):
            if a is None:
                continue
            if any(a.get(k) is not None for k in ("q_b", "k_b", "v_b")):
                return "attention_bias"
            if a["o_b"] is None or n is None or n[0] is None or n[1] is None:
                return "a norm without affine parameters or to_out without bias"
            if any(tuple(a[k].shape) != (M, M) for k in ("q", "k", "v", "o_w")):
                return "an attention that is not M -> M"
        if b["norm3"][0] is None or b["norm3"][1] is None or b["ff1"][1] is None or b["ff2"][1] is None:
            return "a norm without affine parameters or a feed-forward without bias"
        if tuple(b["ff1"][0].shape) != (8 * M, M) or tuple(b["ff2"][0].shape) != (M, 4 * M):
            return "a feed-forward that is not M -> 8M -> M"
    return None


def _drop_active(m) -> bool:
    return isinstance(m, nn.Dropout) and m.training and m.p > 0


def _module_reason(module) -> Optional[str]:
    """Why the kernels cannot restate this module's forward (its structure alone), or None."""
    if not isinstance(getattr(module, "norm", None), nn.GroupNorm) or not module.norm.affine:
        return "norm is not an affine GroupNorm"
    for b in module.transformer_blocks:
        norms = [b.norm1, b.norm3] + ([b.norm2] if getattr(b, "attn2", None) is not None else [])
        if not all(isinstance(n, nn.LayerNorm) and n.elementwise_affine and n.weight is not None and n.bias is not None for n in norms):
            return "norm_type is not layer_norm with affine norms"
        if any(getattr(b, k, False) for k in ("only_cross_attention", "use_ada_layer_norm", "use_ada_layer_norm_zero", "use_ada_layer_norm_continuous")):
            return "only_cross_attention or an adaptive norm"
        if hasattr(b, "fuser") or getattr(b, "_chunk_size", None) is not None:
            return "a gated fuser or feed-forward chunking"
        net = getattr(b.ff, "net", None)
        if net is None or len(net) != 3 or type(net[0]).__name__ != "GEGLU" or not isinstance(getattr(net[0], "proj", None), nn.Linear) or \
                not isinstance(net[2], nn.Linear):
            return "activation_fn is not geglu"
        if _drop_active(net[1]):
            return "dropout is active"
        for a in (b.attn1, getattr(b, "attn2", None)):
            if a is None:
                continue
            if not all(isinstance(getattr(a, k, None), nn.Linear) for k in ("to_q", "to_k", "to_v")) or not isinstance(a.to_out[0], nn.Linear):
                return "an attention without to_q, to_k, to_v, to_out"
            if len(a.to_out) > 1 and _drop_active(a.to_out[1]):
                return "dropout is active"
            if any(getattr(a, k, None) is not None for k in ("group_norm", "spatial_norm", "added_kv_proj_dim")) or \
                    getattr(a, "residual_connection", False) or getattr(a, "rescale_output_factor", 1.0) != 1.0:
                return "an attention with a norm, added projections or a rescale of its own"
            D = a.to_q.out_features // int(a.heads)
            if abs(float(getattr(a, "scale", D ** -0.5)) - D ** -0.5) > 1e-12:
                return "an attention scale other than D^-0.5"
    return None


_cache = weakref.WeakKeyDictionary()                             # module -> (key, _Packed)


def _packed_of(module, params) -> _Packed:
    key = tuple((id(t), t._version, t.data_ptr()) for t in _tensors(params))
    hit = _cache.get(module)
    if hit is None or hit[0] != key:
        hit = (key, _Packed(params))
        _cache[module] = hit
    return hit[1]


def refresh(module) -> None:
    """Drop the module's cached weights. Needed only after a parameter was changed behind autograd's back (an in-place update through
    `p.data`, which moves neither the version counter nor the storage): the stacked [Wq; Wk; Wv] are copies and would go stale."""
    _cache.pop(module, None)


def kernel_reason(module_or_params, x, *, encoder_hidden_states=None, attention_mask=None, encoder_attention_mask=None,
                  grad: str = "none") -> Optional[str]:
    """None where transformer1d runs the kernels for this call, else the first condition that fails. grad="input": a gradient wanted
    by x alone is no reason. grad="params": nor is one wanted by a parameter."""
    _check_grad(grad)
    if encoder_hidden_states is not None or attention_mask is not None or encoder_attention_mask is not None:
        return "encoder_hidden_states or a mask"
    if isinstance(module_or_params, dict):
        return _params_reason(module_or_params, x, grad)
    return _module_reason(module_or_params) or _params_reason(params_of(module_or_params), x, grad)


def transformer1d(module_or_params, x, *, ops: str = "fused", grad: str = "none", encoder_hidden_states=None, attention_mask=None,
                  encoder_attention_mask=None):
    """x (B, C, N) -> (B, C, N): the backbone's forward. ops="fused" runs the kernels where kernel_reason allows and the restatement
    everywhere else; ops="torch" always the restatement. grad="input": the kernels also carry the gradient to x; grad="params": and to
    every parameter that requires one."""
    check_ops(ops)
    _check_grad(grad)
    is_params = isinstance(module_or_params, dict)
    extra = dict(encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask, encoder_attention_mask=encoder_attention_mask)
    if ops == "fused" and kernel_reason(module_or_params, x, grad=grad, **extra) is None:
        params = module_or_params if is_params else params_of(module_or_params)
        return _go(_Packed(params) if is_params else _packed_of(module_or_params, params), x, grad, params)
    return transformer1d_ref(module_or_params if is_params else params_of(module_or_params), x, **extra)


# ---- the module standalone ------------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, query_dim: int, heads: int, dim_head: int, cross_attention_dim: Optional[int] = None):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(cross_attention_dim or query_dim, inner, bias=False)
        self.to_v = nn.Linear(cross_attention_dim or query_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(0.0)])


class GEGLU(nn.Module):
    def __init__(self, dim_in: int, dim_out: int):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    def __init__(self, dim: int, mult: int = 4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim)])


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim: int, heads: int, dim_head: int, cross_attention_dim: Optional[int] = None):
        super().__init__()
        self.only_cross_attention = False
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, heads, dim_head)
        if cross_attention_dim is not None:
            self.norm2 = nn.LayerNorm(dim)
            self.attn2 = Attention(dim, heads, dim_head, cross_attention_dim)
        else:
            self.norm2 = None
            self.attn2 = None
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)
        self._chunk_size = None


class Transformer1D(nn.Module):
    """The reference's Transformer1D with its state-dict keys (`norm.*`, `proj_in.*`, `transformer_blocks.{i}.norm{1,2,3}.*`,
    `attn{1,2}.to_{q,k,v}.weight`, `attn{1,2}.to_out.0.{weight,bias}`, `ff.net.0.proj.*`, `ff.net.2.*`, `proj_out.*`) and nn.Linear's
    initialisation. attn2 exists where cross_attention_dim is given, as in the reference; with no encoder_hidden_states it attends to
    the stream itself, which takes cross_attention_dim == heads * attention_head_dim."""

    def __init__(self, in_channels: int, num_attention_heads: int, attention_head_dim: int, num_layers: int, norm_num_groups: int = 32,
                 cross_attention_dim: Optional[int] = None):
        super().__init__()
        inner = num_attention_heads * attention_head_dim
        self.in_channels, self.num_attention_heads, self.attention_head_dim = in_channels, num_attention_heads, attention_head_dim
        self.norm = nn.GroupNorm(num_groups=norm_num_groups, num_channels=in_channels, eps=GN_EPS, affine=True)
        self.proj_in = nn.Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, num_attention_heads, attention_head_dim, cross_attention_dim)
                                                 for _ in range(num_layers)])
        self.proj_out = nn.Linear(inner, in_channels)

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, encoder_attention_mask=None, ops: str = "fused",
                grad: str = "none"):
        return transformer1d(self, hidden_states, ops=ops, grad=grad, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                             encoder_attention_mask=encoder_attention_mask)


# ---- the seam: a built module's forward ------------------------------------------------------------------------------------------------
_SEAM = (__name__, "fused_transformer1d_cls")
_SEAM_DOC = {"none": "", "input": " and backward to the input",
             "params": " and backward to the input and to every parameter that requires a gradient (gh_xf_backward_params)"}


def fused_transformer1d_cls(base, grad: str = "none"):
    """A subclass of the given Transformer1D class whose forward runs the kernels where kernel_reason allows and is the base class's
    own forward, with the caller's arguments, everywhere else. grad="input": the kernels also carry the gradient to the input;
    grad="params": and to every parameter that requires one."""
    _check_grad(grad)

    def forward(self, hidden_states, encoder_hidden_states=None, timestep=None, modulation_cond=None, class_labels=None,
                cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None):
        # timestep, modulation_cond and class_labels are read by the adaptive norms alone, which kernel_reason refuses: with plain
        # nn.LayerNorm blocks the base class ignores them (TGS._forward passes modulation_cond to both backbones on every call)
        masks = dict(encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask, encoder_attention_mask=encoder_attention_mask)
        asks = masks if grad == "none" else dict(masks, grad=grad)
        if not cross_attention_kwargs and kernel_reason(self, hidden_states, **asks) is None:
            params = params_of(self)
            return _go(_packed_of(self, params), hidden_states, grad, params)
        kw = dict(masks, timestep=timestep, modulation_cond=modulation_cond, class_labels=class_labels, cross_attention_kwargs=cross_attention_kwargs)
        return base.forward(self, hidden_states, **{k: v for k, v in kw.items() if v is not None})

    return _seam.graft(_SEAM, base, {"forward": forward, "_gh_grad": grad}, "fused forward" + _SEAM_DOC[grad], options=(grad,))


def fuse_transformer1d(module, grad: str = "none"):
    """Swap the module's class for fused_transformer1d_cls of its own class. Module objects, parameters and the state dict are
    untouched; calling it again with the same grad changes nothing, with another it swaps to that class. Returns the module."""
    return _seam.swap(_SEAM, module, grad)
