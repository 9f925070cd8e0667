"""Cases and references shared by tests/test_transformer1d_params_cpu.py and tests/test_gpu_transformer1d_params.py: the parameters'
gradients of the Transformer1D backbones (include/gh_xf.h, transformer1d's grad="params").

The constants the shapes are chosen around: the backward-weight product owns TILE x TILE outputs per workgroup, crosses LDS in slabs of
SLAB rows and splits T into chunks of `X.linear_wgrad_chunk(T, K, N_out)` rows, WGRAD_CHUNK for every shape here; the LayerNorm's
parameter gradients take LNP_ROWS rows per stage-one workgroup, the GroupNorm's GN_CHUNK positions."""
import copy

import torch
import torch.nn.functional as F

from tests import transformer1d_cases as K
from tests.fit_cases import sum_within, three_way

TILE, SLAB, WGRAD_CHUNK, LNP_ROWS, GN_CHUNK = 64, 32, 256, 64, 256
# the forward's row counts, then one row below the chunk, the chunk, one row over it (257 is both) and two chunks plus one
WGRAD_T = (1, 31, 33, 63, 64, 65, 129, 257, WGRAD_CHUNK - 1, WGRAD_CHUNK, 2 * WGRAD_CHUNK + 1)
WGRAD_SHAPES = ((64, 65), (32, 63), (512, 64), (512, 130), (32, 1))        # (K, N_out)
WGRAD_PROLOGUES = (("none", 1), ("ln", 1), ("gn", 1), ("gn", 2), ("cf", 1), ("cf", 2))   # (prologue, batch elements of T rows each)
NORM_K = (32, 64, 512)
GN_N = (1, 255, 256, 257)
LN_EPS, GN_EPS = 1e-5, 1e-6


def wgrad_inputs(T, K_, n_out, pro, B, seed=0, device="cpu"):
    """float32 inputs of one gh_xf_linear_wgrad case: B batch elements of T rows each. x is (B T, K) rows, or (B, K, T) channel first
    under "gn" and "cf"; dy is (B T, N_out) rows; the LayerNorm's row moments are the float64 ones rounded."""
    gen = torch.Generator().manual_seed(7000 + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    cf = pro in ("gn", "cf")
    d = {"x": r(B, K_, T) if cf else r(B * T, K_), "dy": r(B * T, n_out), "gamma": 1 + 0.1 * r(K_), "beta": 0.1 * r(K_)}
    if pro == "ln":
        x64 = d["x"].double()
        d["moments"] = torch.stack([x64.mean(1), (x64.var(1, unbiased=False) + LN_EPS).rsqrt()], dim=1).float()
    d = {k: v.to(device) for k, v in d.items()}
    d.update(B=B, N=T, G=32)
    return d


def group_norm(x, G, gamma=None, beta=None, eps=GN_EPS):
    """F.group_norm; a group of one value (one channel at N = 1), which F.group_norm refuses, from the same formula."""
    B, C, N = x.shape
    if (C // G) * N > 1:
        return F.group_norm(x, G, gamma, beta, eps)
    g = x.reshape(B, G, -1)
    y = ((g - g.mean(2, keepdim=True)) * (g.var(2, unbiased=False, keepdim=True) + eps).rsqrt()).reshape(B, C, N)
    y = y if gamma is None else y * gamma[None, :, None]
    return y if beta is None else y + beta[None, :, None]


def wgrad_px(d, pro, dtype):
    """P(X) as (rows, K) in `dtype`, with torch's own norms."""
    x = d["x"].to(dtype)
    if pro == "ln":
        return F.layer_norm(x, (x.shape[1],), d["gamma"].to(dtype), d["beta"].to(dtype), LN_EPS)
    if pro == "gn":
        x = group_norm(x, d["G"], d["gamma"].to(dtype), d["beta"].to(dtype), GN_EPS)
    if pro in ("gn", "cf"):
        return x.permute(0, 2, 1).reshape(-1, x.shape[1])
    return x


def wgrad_ref(d, pro, dtype):
    dy = d["dy"].to(dtype)
    return {"dW": dy.t() @ wgrad_px(d, pro, dtype), "db": dy.sum(0)}


def dy_channel_first(d):
    """dy's values as the channel-first (B, N_out, N) the product reads for proj_out."""
    return d["dy"].reshape(d["B"], d["N"], -1).permute(0, 2, 1).contiguous()


def hold(got, t32, f64, fields, abs_sums, n, tag, name=None):
    """The three-way rule per field; a field that misses it is held to the sum bound n U sum|terms| + U |exact| instead (fields that are
    one long float32 sum: abs_sums gives sum|terms| per element, n the documented chain length plus the roundings of a term)."""
    for k in fields:
        try:
            three_way(got, t32, f64, (k,), tag=f"{tag} {k}", name=name)
        except AssertionError:
            print(f"{tag} {k}: past the three-way bound, held to the sum bound with n = {n}")
            sum_within(got[k], f64[k], abs_sums[k], n, f"{tag} {k}", name=name, field=k + "_sum")


def wgrad_chain(rows, chunk):
    """The longest chain of one dW or db element: a chunk's rows, then the chunks' join; 8 more for the roundings inside a term (the
    prologue's four operations, under GN the rstd formed from m2)."""
    return min(rows, chunk) + (rows + chunk - 1) // chunk - 1 + 8


def with_nan_behind(t, pad):
    """t's values at the front of a buffer whose remaining `pad` elements are NaN: (the view, the buffer)."""
    buf = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[:t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def ln_grads_ref(x, dn, dtype):
    g = torch.ones(x.shape[1], dtype=dtype, device=x.device, requires_grad=True)
    b = torch.zeros(x.shape[1], dtype=dtype, device=x.device, requires_grad=True)
    dg, db = torch.autograd.grad(F.layer_norm(x.to(dtype), (x.shape[1],), g, b, LN_EPS), (g, b), dn.to(dtype))
    return {"dgamma": dg, "dbeta": db}


def gn_grads_ref(x, dy, G, dtype):
    g = torch.ones(x.shape[1], dtype=dtype, device=x.device, requires_grad=True)
    b = torch.zeros(x.shape[1], dtype=dtype, device=x.device, requires_grad=True)
    dg, db = torch.autograd.grad(group_norm(x.to(dtype), G, g, b, GN_EPS), (g, b), dy.to(dtype))
    return {"dgamma": dg, "dbeta": db}


def trainable(case, device="cpu"):
    """A StandIn of one whole-stack case with the weights K.stack_case draws, every parameter requiring a gradient, and its x."""
    C, heads, D, layers, B, N, attn2 = case
    m = K.make_module(C, heads, D, layers, attn2=attn2, seed=layers, device=device)
    return m.requires_grad_(True), K.make_x(B, C, N, seed=N, device=device)


def autograd_grads(m, x, dout, dtype):
    """{"dx", parameter name: gradient} of sum(out * dout) by torch's autograd through transformer1d_ref in `dtype`, on a copy of m."""
    from guassianhand_amd import transformer1d as X
    mm = copy.deepcopy(m).to(dtype).requires_grad_(True)
    xx = x.detach().to(dtype).requires_grad_(True)
    names, ps = zip(*mm.named_parameters())
    gs = torch.autograd.grad(X.transformer1d_ref(X.params_of(mm), xx), (xx, *ps), dout.to(dtype))
    return dict(zip(("dx", *names), gs))


def module_grads(f, m, x, dout):
    """{"dx", parameter name: gradient} of sum(f(x) * dout) for the parameters of m that require a gradient (and x where it does)."""
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    ins = ([("dx", x)] if x.requires_grad else []) + named
    out = f(x)
    gs = torch.autograd.grad(out, [t for _, t in ins], dout)
    return dict(zip([n for n, _ in ins], gs)), out
