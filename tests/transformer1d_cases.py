"""Cases and references shared by tests/test_transformer1d_cpu.py and tests/test_gpu_transformer1d.py.

The constants the shapes are chosen around (include/gh_xf.h): the product's workgroup owns ROW_TILE x COL_TILE outputs, a wave 32 x 32,
and K crosses LDS K_SLAB columns at a time; the attention's workgroup owns ATTN_ROWS queries (32 per wave pair) and stages ATTN_KEYS
keys (32 per wave); stage one of the group moments takes GN_CHUNK positions per workgroup; the LayerNorm moments take one wave per row,
LN_ROWS rows per workgroup."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

ROW_TILE, COL_TILE, K_SLAB, WAVE_TILE = 64, 64, 32, 32
ATTN_ROWS, ATTN_KEYS = 64, 64
GN_CHUNK, LN_ROWS = 256, 4

# (T, K, N_out): every T of the issue at one K and a width one past the column tile, then widths one short of it, on it and past two
# of it, the largest K, and a single column
LINEAR_T = (1, 31, 33, 63, 64, 65, 129, 257)
LINEAR_SHAPES = [(T, 64, COL_TILE + 1) for T in LINEAR_T] + [(65, 32, COL_TILE - 1), (129, 512, COL_TILE), (257, 512, 2 * COL_TILE + 2), (33, 32, 1)]
PROLOGUES = ("none", "ln", "gn")
EPILOGUES = ("plain", "bias_res", "geglu", "bias_res_cf")
ATTN_N = (1, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 257)    # 63 .. 65: the stage of 64 keys and the tile of 64 queries; 97: one key in the odd wave's tile
# (C, heads, D, layers, B, N, attn2)
STACKS = [(64, 1, 64, 2, 2, 129, True), (64, 2, 32, 10, 1, 129, True), (512, 8, 64, 1, 2, 257, True), (64, 2, 32, 2, 2, 65, False)]


def batch_of(T):
    """Rows per batch element for the channel-first forms: three batch elements where T divides, else one."""
    return (3, T // 3) if T % 3 == 0 else (1, T)


# ---- a straightforward composition with the reference's attribute layout ---------------------------------------------------------------
class Attn(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.to_q, self.to_k, self.to_v = (nn.Linear(dim, dim, bias=False) for _ in range(3))
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

    def forward(self, h, ctx=None, bias=None):
        B, N, M = h.shape
        ctx = h if ctx is None else ctx
        D = M // self.heads
        q, k, v = (t.view(B, -1, self.heads, D).transpose(1, 2) for t in (self.to_q(h), self.to_k(ctx), self.to_v(ctx)))
        s = q @ k.transpose(-1, -2) * D ** -0.5
        if bias is not None:
            s = s + bias[:, None]
        o = (F.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, N, M)
        return self.to_out[1](self.to_out[0](o))


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, 2 * dim_out)

    def forward(self, x):
        a, g = self.proj(x).chunk(2, dim=-1)
        return a * F.gelu(g)


class FeedForward(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, 4 * dim), nn.Dropout(0.0), nn.Linear(4 * dim, dim)])

    def forward(self, x):
        for m in self.net:
            x = m(x)
        return x


class Block(nn.Module):
    def __init__(self, dim, heads, attn2):
        super().__init__()
        self.only_cross_attention = False
        self.norm1, self.attn1 = nn.LayerNorm(dim), Attn(dim, heads)
        self.norm2, self.attn2 = (nn.LayerNorm(dim), Attn(dim, heads)) if attn2 else (None, None)
        self.norm3, self.ff = nn.LayerNorm(dim), FeedForward(dim)
        self._chunk_size = None

    def forward(self, h, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None):
        h = h + self.attn1(self.norm1(h), None, attention_mask)
        if self.attn2 is not None:
            h = h + self.attn2(self.norm2(h), encoder_hidden_states, encoder_attention_mask)
        return h + self.ff(self.norm3(h))


class StandIn(nn.Module):
    """nn.GroupNorm, nn.LayerNorm, nn.Linear and F.softmax composed as tgs/models/transformers.py:860-908 composes them, with the
    reference's attribute names and its forward's signature."""
    calls = 0

    def __init__(self, C, heads, D, layers, G=32, attn2=True):
        super().__init__()
        M = heads * D
        self.num_attention_heads, self.attention_head_dim, self.in_channels = heads, D, C
        self.norm = nn.GroupNorm(G, C, eps=1e-6, affine=True)
        self.proj_in = nn.Linear(C, M)
        self.transformer_blocks = nn.ModuleList([Block(M, heads, attn2) for _ in range(layers)])
        self.proj_out = nn.Linear(M, C)

    def forward(self, hidden_states, encoder_hidden_states=None, timestep=None, modulation_cond=None, class_labels=None,
                cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None):
        StandIn.calls += 1
        x = hidden_states
        if attention_mask is not None and attention_mask.ndim == 2:
            attention_mask = ((1 - attention_mask.to(x.dtype)) * -10000.0).unsqueeze(1)
        if encoder_attention_mask is not None and encoder_attention_mask.ndim == 2:
            encoder_attention_mask = ((1 - encoder_attention_mask.to(x.dtype)) * -10000.0).unsqueeze(1)
        B, C, N = x.shape
        h = self.proj_in(self.norm(x).permute(0, 2, 1).reshape(B, N, C))
        for b in self.transformer_blocks:
            h = b(h, attention_mask, encoder_hidden_states, encoder_attention_mask)
        return self.proj_out(h).reshape(B, N, C).permute(0, 2, 1).contiguous() + x


def make_module(C, heads, D, layers, G=32, attn2=True, seed=0, device="cpu", dtype=torch.float32):
    """A StandIn with weights ~ N(0, 1 / K) (K the layer's input width, so activations stay O(1)), biases ~ 0.1 N(0, 1) and norm
    scales ~ 1 + 0.1 N(0, 1)."""
    m = StandIn(C, heads, D, layers, G, attn2)
    gen = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if p.dim() == 2:
                p.copy_(r * p.shape[1] ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1 + 0.1 * r)
            else:
                p.copy_(0.1 * r)
    return m.to(device=device, dtype=dtype).eval()


def make_x(B, C, N, seed=0, device="cpu", dtype=torch.float32):
    return torch.randn(B, C, N, generator=torch.Generator().manual_seed(2000 + seed)).to(device=device, dtype=dtype)


# ---- references of the single launches ------------------------------------------------------------------------------------------------
def linear_inputs(T, K, n_out, pro, epi, seed=0, device="cpu"):
    """float32 inputs of one gh_xf_linear case as a dict; x and res in the layout the prologue / epilogue reads."""
    gen = torch.Generator().manual_seed(3000 + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    B, N = batch_of(T)
    G = 32 if K % 32 == 0 else 1
    d = {"x": r(B, K, N) if pro == "gn" else r(T, K), "w": r((2 if epi == "geglu" else 1) * n_out, K) * K ** -0.5,
         "bias": 0.1 * r((2 if epi == "geglu" else 1) * n_out), "gamma": 1 + 0.1 * r(K), "beta": 0.1 * r(K),
         "res": r(B, n_out, N) if epi == "bias_res_cf" else r(T, n_out)}
    d = {k: v.to(device) for k, v in d.items()}
    d.update(B=B, N=N, G=G)
    return d


def linear_ref(d, pro, epi, dtype):
    """What gh_xf_linear computes, with torch's own group_norm / layer_norm / linear / gelu in `dtype`."""
    t = {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    x, B, N = t["x"], t["B"], t["N"]
    if pro == "ln":
        x = F.layer_norm(x, (x.shape[1],), t["gamma"], t["beta"], 1e-5)
    elif pro == "gn":
        K = x.shape[1]
        x = F.group_norm(x, t["G"], t["gamma"], t["beta"], 1e-6).permute(0, 2, 1).reshape(B * N, K)
    if epi == "plain":
        return F.linear(x, t["w"])
    y = F.linear(x, t["w"], t["bias"])
    if epi == "bias_res":
        return y + t["res"]
    if epi == "geglu":
        a, g = y.chunk(2, dim=-1)
        return a * F.gelu(g)
    return y.reshape(B, N, -1).permute(0, 2, 1) + t["res"]


def linear_kernel(d, pro, epi, x=None):
    from guassianhand_amd import transformer1d as X
    kw = dict(prologue=pro, epilogue=epi)
    if pro != "none":
        kw.update(gamma=d["gamma"], beta=d["beta"], eps=1e-6 if pro == "gn" else 1e-5)
    if pro == "gn":
        kw.update(groups=d["G"], moments=X.group_moments(d["x"], d["G"]))
    if epi != "plain":
        kw.update(bias=d["bias"])
    if epi in ("bias_res", "bias_res_cf"):
        kw.update(res=d["res"])
    if epi == "bias_res_cf":
        kw.update(rows_per_batch=d["N"])
    return X.linear(d["x"] if x is None else x, d["w"], **kw)


def attention_ref(qkv, B, N, heads, D, dtype):
    M = heads * D
    q, k, v = (t.reshape(B, N, heads, D).transpose(1, 2) for t in qkv.to(dtype).split(M, dim=1))
    s = q @ k.transpose(-1, -2) * D ** -0.5
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, M)


# ---- references of the backward's single launches: torch's autograd in `dtype` ----------------------------------------------------------
def lse_ref(qkv, B, N, heads, D, dtype):
    M = heads * D
    q, k, _v = (t.reshape(B, N, heads, D).transpose(1, 2) for t in qkv.to(dtype).split(M, dim=1))
    return torch.logsumexp(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)


def attention_grads(qkv, dout, B, N, heads, D, dtype):
    t = qkv.to(dtype).requires_grad_(True)
    g, = torch.autograd.grad(attention_ref(t, B, N, heads, D, dtype), t, dout.to(dtype))
    M = heads * D
    return {"dq": g[:, :M], "dk": g[:, M:2 * M], "dv": g[:, 2 * M:]}


def ln_ref(x, dn, g0, gamma, beta, dtype):
    t = x.to(dtype).requires_grad_(True)
    g, = torch.autograd.grad(F.layer_norm(t, (t.shape[1],), gamma.to(dtype), beta.to(dtype), 1e-5), t, dn.to(dtype))
    return {"g": g0.to(dtype) + g}


def geglu_ref(d, dtype):
    t = {k: v.to(dtype) for k, v in d.items()}
    pre = F.linear(F.layer_norm(t["h"], (t["h"].shape[1],), t["gamma"], t["beta"], 1e-5), t["w1"], t["b1"]).detach().requires_grad_(True)
    a, g = pre.chunk(2, dim=-1)
    y, = torch.autograd.grad(F.linear(a * F.gelu(g), t["w2"]), pre, t["g"])
    return {"dadg": y, "gate": pre.detach()[:, pre.shape[1] // 2:]}


def gn_ref(x, dy, dout, gamma, beta, G, dtype):
    t = x.to(dtype).requires_grad_(True)
    g, = torch.autograd.grad(F.group_norm(t, G, gamma.to(dtype), beta.to(dtype), 1e-6), t, dy.to(dtype))
    return {"dx": dout.to(dtype) + g}


def strided_misaligned(t, pad=5):
    """t's values in a view whose row stride is pad longer than its width and whose pointer is 4 bytes past a 16-byte boundary."""
    T, K = t.shape
    buf = torch.empty(T * (K + pad) + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(T, K + pad)[:, :K]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and (T == 1 or v.stride(0) == K + pad)
    return v


@functools.lru_cache(maxsize=None)
def stack_case(case, device):
    """(module float32, x, the float64 and float32 restatements' outputs) of one whole-stack case, computed once per process."""
    from guassianhand_amd import transformer1d as X
    C, heads, D, layers, B, N, attn2 = case
    m = make_module(C, heads, D, layers, attn2=attn2, seed=layers, device=device)
    x = make_x(B, C, N, seed=N, device=device)
    with torch.no_grad():
        p = X.params_of(m)
        return m, x, X.transformer1d_ref(p, x, acc=torch.float64), X.transformer1d_ref(p, x)
