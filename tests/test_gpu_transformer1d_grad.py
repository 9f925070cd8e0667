"""The Transformer1D backward to the input (include/gh_xf.h, transformer1d's grad="input") on the device. The criterion is
tests/fit_cases.three_way: the kernel, torch's float32 autograd and its float64 autograd run on the device on the same inputs, and per
field max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64|, no element excluded; the three errors are printed. Cotangents are drawn
from seeded generators. Bit equality wherever two paths perform the same float32 operations in the same order.

Whole-stack error ratios (kernel error over the bound) are recorded under the names "xf_grad_stack_*" by fit_cases.three_way."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import transformer1d_cases as K
from tests.fit_cases import bits, three_way
from tests.transformer1d_cases import attention_grads, geglu_ref, gn_ref, ln_ref, lse_ref      # shared with the edge tests

pytestmark = pytest.mark.gpu

BWD_ROWS, BWD_STAGE = 128, 64
ATTN_N = (1, 31, 32, 33, 63, 64, 65, 129, 257)                    # the tile edges of both sweeps: tiles of 32 in stages of 64, blocks of 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert (_abi.GH_XF_ATTN_BWD_ROWS, _abi.GH_XF_ATTN_BWD_STAGE, _abi.GH_XF_GN_CHUNK) == (BWD_ROWS, BWD_STAGE, K.GN_CHUNK)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def X():
    from guassianhand_amd import transformer1d
    return transformer1d


def rnd(dev, *shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(11000 + seed)) * scale).to(dev)


def frozen(dev, C_, heads, D, layers, attn2=True, seed=0):
    m = K.make_module(C_, heads, D, layers, attn2=attn2, seed=seed, device=dev)
    return m.requires_grad_(False)


# ---- the taped forward -------------------------------------------------------------------------------------------------------------------
def tape_layout(B, N, heads, D, G, layers):
    """Byte offsets as include/gh_xf.h lays the tape out: {"gn", ("attn" | "ff", layer, which): {part: offset}}, and the total."""
    al = lambda n: (n + 255) & ~255
    T, M = B * N, heads * D
    parts = [("h", T * M), ("ln", T * 2), ("qkv", T * 3 * M), ("att", T * M), ("lse", T * heads)]
    a_size = sum(al(4 * n) for _, n in parts)
    f_size = al(4 * T * M) + al(4 * T * 2)
    out, at = {"gn": 0}, al(4 * B * G * 2)
    for i in range(layers):
        for which in range(2):
            o, d = at + which * a_size, {}
            for name, n in parts:
                d[name] = o
                o += al(4 * n)
            out[("attn", i, which)] = d
        out[("ff", i)] = {"h": at + 2 * a_size, "ln": at + 2 * a_size + al(4 * T * M)}
        at += 2 * a_size + f_size
    return out, at


def view(tape, off, *shape):
    n = 1
    for s in shape:
        n *= s
    return tape[off:off + 4 * n].view(torch.float32).view(*shape)


@pytest.mark.parametrize("case", K.STACKS, ids=lambda c: "C%d_h%d_D%d_L%d_B%d_N%d_%s" % (*c[:6], "attn2" if c[6] else "noattn2"))
def test_taped_forward_is_bitwise_the_forward_and_its_tape_is_the_layout(dev, X, case):
    Cc, heads, D, layers, B, N, attn2 = case
    m, x, _f64, _t32 = K.stack_case(case, str(dev))
    T, M = B * N, heads * D
    with torch.no_grad():
        p = X.params_of(m)
        packed = X._Packed(p)
        want = X._run(packed, x)
        out, tape = X._run_tape(packed, x)
        assert torch.equal(bits(out), bits(want))
        lay, total = tape_layout(B, N, heads, D, 32, layers)
        from guassianhand_amd._call import lib
        assert int(lib().gh_xf_tape_bytes(C.byref(X._dims(packed, x)))) == total == tape.numel()
        assert torch.equal(bits(view(tape, lay["gn"], B, 32, 2)), bits(X.group_moments(x, 32)))
        # the first layer's first slot: the stream behind proj_in, its LayerNorm moments, qkv, the attention and its lse
        s = lay[("attn", 0, 0)]
        h0 = F.linear(F.group_norm(x, 32, *p["norm"], eps=1e-6).permute(0, 2, 1).reshape(T, Cc), *p["proj_in"])
        th, tln = view(tape, s["h"], T, M), view(tape, s["ln"], T, 2)
        assert float((th - h0).abs().max()) <= 1e-4 * float(h0.abs().max())
        three_way({"mean": tln[:, 0], "rstd": tln[:, 1]}, {"mean": th.mean(1), "rstd": (th.var(1, unbiased=False) + 1e-5).rsqrt()},
                  {"mean": th.double().mean(1), "rstd": (th.double().var(1, unbiased=False) + 1e-5).rsqrt()}, ("mean", "rstd"), tag="tape LN moments")
        qkv = view(tape, s["qkv"], T, 3 * M)
        att, lse = X.attention_lse(qkv, B, N, heads, D)
        assert torch.equal(bits(view(tape, s["att"], T, M)), bits(att)) and torch.equal(bits(att), bits(X.attention(qkv, B, N, heads, D)))
        assert torch.equal(bits(view(tape, s["lse"], B, heads, N)), bits(lse))
        # the feed-forward's slot of the last layer holds the stream the last feed-forward read: out follows from it
        f = lay[("ff", layers - 1)]
        hl = view(tape, f["h"], T, M)
        b = p["blocks"][-1]
        a_, g_ = F.linear(F.layer_norm(hl, (M,), *b["norm3"], eps=1e-5), *b["ff1"]).chunk(2, dim=-1)
        hl = hl + F.linear(a_ * F.gelu(g_), *b["ff2"])
        o2 = F.linear(hl, *p["proj_out"]).reshape(B, N, Cc).permute(0, 2, 1) + x
        assert float((o2 - out).abs().max()) <= 1e-4 * float(out.abs().max())


def make_qkv(dev, B, N, heads, D, seed=0):
    gen = torch.Generator().manual_seed(4000 + seed)
    return (torch.randn(B * N, 3 * heads * D, generator=gen) * torch.tensor([2.0, 1.0, 1.0]).repeat_interleave(heads * D)).to(dev)


@pytest.mark.parametrize("N", [1, 33, 64, 129, 257])
@pytest.mark.parametrize("D,heads", [(32, 2), (64, 1)])
def test_lse(dev, X, D, heads, N):
    qkv = make_qkv(dev, 3, N, heads, D, seed=N)
    out, lse = X.attention_lse(qkv, 3, N, heads, D)
    assert torch.equal(bits(out), bits(X.attention(qkv, 3, N, heads, D)))
    three_way({"lse": lse}, {"lse": lse_ref(qkv, 3, N, heads, D, torch.float32)}, {"lse": lse_ref(qkv, 3, N, heads, D, torch.float64)}, ("lse",),
              tag=f"lse D={D} heads={heads} N={N}")


# ---- gh_xf_attention_backward -------------------------------------------------------------------------------------------------------------
def attention_kernel(X, qkv, dout, B, N, heads, D, dqkv=None):
    out, lse = X.attention_lse(qkv, B, N, heads, D)
    return X.attention_backward(qkv, out, lse, dout, B, N, heads, D, dqkv=dqkv)


@pytest.mark.parametrize("N", ATTN_N)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("D", [32, 64])
def test_attention_backward(dev, X, D, heads, B, N):
    M, T = heads * D, B * N
    qkv, dout = make_qkv(dev, B, N, heads, D, seed=N), rnd(dev, T, M, seed=N + D)
    buf = torch.full((T + 3, 3 * M), 7.0, device=dev)
    got = attention_kernel(X, qkv, dout, B, N, heads, D, dqkv=buf)
    assert got is buf and float((buf[T:] - 7.0).abs().max()) == 0.0    # rows past T keep the sentinel
    k = {"dq": buf[:T, :M].contiguous(), "dk": buf[:T, M:2 * M].contiguous(), "dv": buf[:T, 2 * M:].contiguous()}
    three_way(k, attention_grads(qkv, dout, B, N, heads, D, torch.float32), attention_grads(qkv, dout, B, N, heads, D, torch.float64),
              ("dq", "dk", "dv"), tag=f"attention backward D={D} heads={heads} B={B} N={N}")


@pytest.mark.parametrize("N", [65, 257])
@pytest.mark.parametrize("D", [32, 64])
def test_attention_backward_bitwise_properties(dev, X, D, N):
    heads = 2
    M = heads * D
    qkv, dout = make_qkv(dev, 1, N, heads, D, seed=1), rnd(dev, N, M, seed=1)
    got = attention_kernel(X, qkv, dout, 1, N, heads, D)
    assert torch.equal(bits(attention_kernel(X, qkv, dout, 1, N, heads, D)), bits(got))
    # a batch element's dqkv does not depend on B or on its slot
    q3 = torch.cat([make_qkv(dev, 1, N, heads, D, seed=2), qkv, qkv], dim=0)
    d3 = torch.cat([rnd(dev, N, M, seed=2), dout, dout], dim=0)
    g3 = attention_kernel(X, q3, d3, 3, N, heads, D)
    assert torch.equal(bits(g3[N:2 * N]), bits(got)) and torch.equal(bits(g3[2 * N:]), bits(got))
    # a strided, misaligned qkv (and dout) is read in place
    out, lse = X.attention_lse(qkv, 1, N, heads, D)
    sq, sd = K.strided_misaligned(qkv), K.strided_misaligned(dout)
    assert torch.equal(bits(X.attention_backward(sq, out, lse, sd, 1, N, heads, D)), bits(got))


def test_attention_backward_masks_the_partial_query_tile_whatever_lse_holds(dev, X):
    """N = 33: the second tile of 32 queries holds one. The lse buffer is followed by NaN and by -1e30 (exp(s - lse) = inf) in turn."""
    B, N, heads, D = 1, 33, 1, 32
    qkv, dout = make_qkv(dev, B, N, heads, D, seed=3), rnd(dev, N, D, seed=3)
    out, lse = X.attention_lse(qkv, B, N, heads, D)
    want = X.attention_backward(qkv, out, lse, dout, B, N, heads, D)
    for tail in (float("nan"), -1e30):
        big = torch.full((B * heads * N + 64,), tail, device=dev)
        big[:N] = lse.reshape(-1)
        assert torch.equal(bits(X.attention_backward(qkv, out, big[:N].view(B, heads, N), dout, B, N, heads, D)), bits(want))


# ---- gh_xf_layernorm_backward ---------------------------------------------------------------------------------------------------------------
def ln_case(dev, T, Kc, seed=0):
    x, dn, g0 = rnd(dev, T, Kc, seed=seed) + 0.3, rnd(dev, T, Kc, seed=seed + 1), rnd(dev, T, Kc, seed=seed + 2)
    gamma, beta = 1 + 0.1 * rnd(dev, Kc, seed=seed + 3), 0.1 * rnd(dev, Kc, seed=seed + 4)
    mom = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)
    return x, dn, g0, gamma, beta, mom


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("Kc", [32, 64, 512])
def test_layernorm_backward(dev, X, Kc, T):
    x, dn, g0, gamma, beta, mom = ln_case(dev, T, Kc, seed=T + Kc)
    got = X.layernorm_backward(dn, x, mom, gamma, g0.clone())
    three_way({"g": got}, ln_ref(x, dn, g0, gamma, beta, torch.float32), ln_ref(x, dn, g0, gamma, beta, torch.float64), ("g",),
              tag=f"layernorm backward K={Kc} T={T}")


def test_layernorm_backward_row_does_not_depend_on_its_place(dev, X):
    x, dn, g0, gamma, _beta, mom = ln_case(dev, 257, 512, seed=9)
    full = X.layernorm_backward(dn, x, mom, gamma, g0.clone())
    part = X.layernorm_backward(dn[70:73], x[70:73], mom[70:73], gamma, g0[70:73].clone())
    assert torch.equal(bits(part), bits(full[70:73])) and torch.equal(bits(X.layernorm_backward(dn, x, mom, gamma, g0.clone())), bits(full))
    strided = X.layernorm_backward(K.strided_misaligned(dn), K.strided_misaligned(x), mom, gamma, g0.clone())
    assert torch.equal(bits(strided), bits(full))


# ---- gh_xf_geglu_backward -----------------------------------------------------------------------------------------------------------------
def geglu_case(dev, T, M, seed=0, wide_gate=False):
    d = {"g": rnd(dev, T, M, seed=seed), "h": rnd(dev, T, M, seed=seed + 1) + 0.2, "gamma": 1 + 0.1 * rnd(dev, M, seed=seed + 2),
         "beta": 0.1 * rnd(dev, M, seed=seed + 3), "w1": rnd(dev, 8 * M, M, seed=seed + 4, scale=M ** -0.5), "b1": 0.1 * rnd(dev, 8 * M, seed=seed + 5),
         "w2": rnd(dev, M, 4 * M, seed=seed + 6, scale=(4 * M) ** -0.5)}
    if wide_gate:                                                  # the gate's pre-activation spans [-6, 6]: both tails of gelu'
        d["w1"][4 * M:] *= 0.02
        d["b1"][4 * M:] = torch.linspace(-6.0, 6.0, 4 * M, device=dev)
    h = d["h"]
    d["mom"] = torch.stack([h.mean(1), (h.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)
    return d


@pytest.mark.parametrize("T", [1, 63, 65, 129])
@pytest.mark.parametrize("M", [32, 64])
def test_geglu_backward(dev, X, M, T):
    d = geglu_case(dev, T, M, seed=T + M)
    got = X.geglu_backward(d["g"], d["h"], d["mom"], d["gamma"], d["beta"], d["w1"], d["b1"], d["w2"].t().contiguous())
    three_way({"dadg": got}, geglu_ref(d, torch.float32), geglu_ref(d, torch.float64), ("dadg",), tag=f"geglu backward M={M} T={T}")
    assert torch.equal(bits(X.geglu_backward(K.strided_misaligned(d["g"]), K.strided_misaligned(d["h"]), d["mom"], d["gamma"], d["beta"], d["w1"],
                                             d["b1"], d["w2"].t().contiguous())), bits(got))


def test_geglu_backward_both_tails_of_the_gelu_derivative(dev, X):
    d = geglu_case(dev, 65, 64, seed=7, wide_gate=True)
    f64 = geglu_ref(d, torch.float64)
    assert float(f64["gate"].min()) < -5.5 and float(f64["gate"].max()) > 5.5
    got = X.geglu_backward(d["g"], d["h"], d["mom"], d["gamma"], d["beta"], d["w1"], d["b1"], d["w2"].t().contiguous())
    three_way({"dadg": got}, geglu_ref(d, torch.float32), f64, ("dadg",), tag="geglu backward |g| up to 6")


# ---- gh_xf_group_norm_backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 2 * K.GN_CHUNK + 1])
@pytest.mark.parametrize("Cc", [32, 64])
def test_group_norm_backward(dev, X, Cc, N):
    B, G = 2, 32
    x, dy, dout = K.make_x(B, Cc, N, seed=N, device=dev) + 0.5, rnd(dev, B, Cc, N, seed=N), rnd(dev, B, Cc, N, seed=N + 1)
    gamma, beta = 1 + 0.1 * rnd(dev, Cc, seed=2), 0.1 * rnd(dev, Cc, seed=3)
    mom = X.group_moments(x, G)
    got = X.group_norm_backward(dy, x, mom, gamma, dout, G)
    if Cc == G and N == 1:
        # every group is one value: the norm's term is exactly 0 and dx is dout bit for bit
        assert torch.equal(bits(got), bits(dout))
    else:
        three_way({"dx": got}, gn_ref(x, dy, dout, gamma, beta, G, torch.float32), gn_ref(x, dy, dout, gamma, beta, G, torch.float64), ("dx",),
                  tag=f"group norm backward C={Cc} N={N}")
    assert torch.equal(bits(X.group_norm_backward(dy, x, mom, gamma, dout, G)), bits(got))
    # a batch element's dx does not depend on its slot
    assert torch.equal(bits(X.group_norm_backward(dy[1:], x[1:], mom[1:], gamma, dout[1:], G)), bits(got[1:]))


# ---- the backward-data product and the channel-first read --------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 65, 257])
@pytest.mark.parametrize("Kc", [64, 96, 192, 4096])
def test_backward_data_product_and_the_channel_first_read(dev, X, Kc, T):
    """dX = dY W through a transposed copy of W (n_out, K) -> wt (K columns per row of W^T): K takes the widths M, 3M, 8M of the chain."""
    n_out = 65
    dy, w = rnd(dev, T, Kc, seed=T + Kc), rnd(dev, Kc, n_out, seed=Kc, scale=Kc ** -0.5)     # Y = X W^T with W (K, n_out): dX = dY W
    wt = w.t().contiguous()
    got = X.linear(dy, wt)
    three_way({"dx": got}, {"dx": dy @ w}, {"dx": dy.double() @ w.double()}, ("dx",), tag=f"backward data K={Kc} T={T}")
    B, N = K.batch_of(T)
    cf = dy.reshape(B, N, Kc).permute(0, 2, 1).contiguous()       # the same rows, channel first
    assert torch.equal(bits(X.linear(cf, wt, prologue="cf")), bits(got))


# ---- the whole stack -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_case(case, device):
    """(frozen module, x, dout, the float64 and float32 restatements' dx) of one whole-stack case, computed once per process."""
    from guassianhand_amd import transformer1d as X
    Cc, heads, D, layers, B, N, attn2 = case
    m = frozen(device, Cc, heads, D, layers, attn2=attn2, seed=layers)
    x = K.make_x(B, Cc, N, seed=N, device=device)
    dout = rnd(device, B, Cc, N, seed=N + layers)
    p = X.params_of(m)
    x32 = x.clone().requires_grad_(True)
    g32, = torch.autograd.grad(X.transformer1d_ref(p, x32), x32, dout)
    x64 = x.double().requires_grad_(True)
    g64, = torch.autograd.grad(X.transformer1d_ref(X._map(p, lambda t: t.double()), x64), x64, dout.double())
    return m, x, dout, g64, g32


@pytest.mark.parametrize("case", K.STACKS, ids=lambda c: "C%d_h%d_D%d_L%d_B%d_N%d_%s" % (*c[:6], "attn2" if c[6] else "noattn2"))
def test_whole_stack_backward(dev, X, case):
    Cc, heads, D, layers, B, N, attn2 = case
    m, x, dout, g64, g32 = grad_case(case, str(dev))
    name = "xf_grad_stack_C%d_h%d_D%d_L%d_B%d_N%d" % case[:6] + ("" if attn2 else "_noattn2")
    xr = x.clone().requires_grad_(True)
    assert X.kernel_reason(m, xr, grad="input") is None and X.kernel_reason(m, xr) == "a gradient is wanted"

    def dx_of(f, xin=xr, d=dout):
        out = f(xin)
        assert out.requires_grad
        return torch.autograd.grad(out, xin, d)[0], out

    got, out = dx_of(lambda t: X.transformer1d(X.params_of(m), t, grad="input"))
    with torch.no_grad():
        assert torch.equal(bits(out), bits(X.transformer1d(m, x)))                 # the taped forward is the forward
    three_way({"dx": got}, {"dx": g32}, {"dx": g64}, ("dx",), tag=name, name=name)
    s = X.Transformer1D(Cc, heads, D, layers, cross_attention_dim=heads * D if attn2 else None).to(dev)
    s.load_state_dict(m.state_dict())
    s.requires_grad_(False)
    assert torch.equal(bits(dx_of(lambda t: s(t, grad="input"))[0]), bits(got))
    assert torch.equal(bits(dx_of(lambda t: X.transformer1d(m, t, grad="input"))[0]), bits(got))
    n = K.StandIn.calls
    fused = X.fuse_transformer1d(frozen(dev, Cc, heads, D, layers, attn2=attn2, seed=layers), grad="input")
    assert torch.equal(bits(dx_of(fused)[0]), bits(got)) and K.StandIn.calls == n   # the base forward did not run
    assert torch.equal(bits(dx_of(fused)[0]), bits(got))                             # two runs are equal
    # a batch element's dx does not depend on B or on its slot
    x3 = torch.cat([x[-1:], K.make_x(1, Cc, N, seed=99, device=dev), x[-1:]], dim=0).requires_grad_(True)
    d3 = torch.cat([dout[-1:], rnd(dev, 1, Cc, N, seed=98), dout[-1:]], dim=0)
    g3, _ = dx_of(lambda t: s(t, grad="input"), x3, d3)
    assert torch.equal(bits(g3[0]), bits(got[-1])) and torch.equal(bits(g3[2]), bits(got[-1]))
    # nothing requires a gradient: the plain untaped path
    with torch.no_grad():
        assert not fused(xr).requires_grad
    assert not fused(x).requires_grad and K.StandIn.calls == n


def test_a_trainable_parameter_takes_the_base_forward(dev, X):
    m = frozen(dev, 64, 2, 32, 1, seed=16)
    x = K.make_x(2, 64, 33, device=dev).requires_grad_(True)
    w = m.transformer_blocks[0].attn1.to_q.weight.requires_grad_(True)
    assert X.kernel_reason(m, x, grad="input") == "a parameter wants a gradient"
    n = K.StandIn.calls
    out = X.fuse_transformer1d(m, grad="input")(x)
    assert K.StandIn.calls == n + 1 and out.requires_grad
    out.square().sum().backward()
    assert bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0 and float(x.grad.abs().max()) > 0


def test_cached_transposes_follow_the_parameters(dev, X):
    m = frozen(dev, 64, 2, 32, 1, seed=11)
    x = K.make_x(1, 64, 33, device=dev).requires_grad_(True)
    dout = rnd(dev, 1, 64, 33, seed=4)
    a, = torch.autograd.grad(X.transformer1d(m, x, grad="input"), x, dout)
    with torch.no_grad():
        m.transformer_blocks[0].ff.net[2].weight.mul_(0.5)          # bumps the version counter
    b, = torch.autograd.grad(X.transformer1d(m, x, grad="input"), x, dout)
    c, = torch.autograd.grad(X.transformer1d(X.params_of(m), x, grad="input"), x, dout)
    assert not torch.equal(a, b) and torch.equal(bits(b), bits(c))


def test_graph_capture_of_forward_and_backward_replays_bitwise(dev, X):
    m = X.fuse_transformer1d(frozen(dev, 64, 2, 32, 2, seed=12), grad="input")
    x = K.make_x(2, 64, 129, seed=12, device=dev).requires_grad_(True)
    dout = rnd(dev, 2, 64, 129, seed=12)
    step = lambda: torch.autograd.grad(m(x), x, dout)[0]
    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dx = step()
    dx.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(dx), bits(eager))
    with torch.no_grad():
        x.copy_(K.make_x(2, 64, 129, seed=13, device=dev))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(dx), bits(step()))


# ---- return codes, empty inputs -----------------------------------------------------------------------------------------------------------
def test_return_codes(dev, X):
    from guassianhand_amd import _abi
    from guassianhand_amd._call import lib, stream, workspace
    L = lib()
    st = stream(dev)
    m = frozen(dev, 64, 2, 32, 1, seed=14)
    p = X._Packed(X.params_of(m))
    stem_t, layers_t = p.transposed()
    x = K.make_x(1, 64, 33, device=dev)
    dout = rnd(dev, 1, 64, 33, seed=14)
    y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    big = workspace(1 << 24, dev)
    tape_big = workspace(1 << 24, dev)
    tape_big.fill_(7)
    # M = 1024: the forward runs such a stack, the taped pair does not
    wide = _abi.GhXfDims(1, 64, 33, 32, 16, 64, 1, 1e-6, 1e-5)
    assert L.gh_xf_tape_bytes(C.byref(wide)) == 0 and L.gh_xf_backward_workspace_bytes(C.byref(wide)) == 0
    assert L.gh_xf_forward_tape(C.byref(wide), C.byref(p.stem), p.layers, x.data_ptr(), y.data_ptr(), tape_big.data_ptr(), 1 << 24, big.data_ptr(),
                                1 << 24, st) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_backward(C.byref(wide), C.byref(stem_t), layers_t, x.data_ptr(), tape_big.data_ptr(), dout.data_ptr(), dx.data_ptr(), big.data_ptr(),
                            1 << 24, st) == _abi.GH_ERR_UNSUPPORTED
    dims = _abi.GhXfDims(1, 64, 33, 32, 2, 32, 1, 1e-6, 1e-5)
    need, tneed, bneed = (int(f(C.byref(dims))) for f in (L.gh_xf_workspace_bytes, L.gh_xf_tape_bytes, L.gh_xf_backward_workspace_bytes))
    assert 0 < need <= 1 << 24 and 0 < tneed <= 1 << 24 and 0 < bneed <= 1 << 24
    fwd = lambda tb, wb: L.gh_xf_forward_tape(C.byref(dims), C.byref(p.stem), p.layers, x.data_ptr(), y.data_ptr(), tape_big.data_ptr(), tb,
                                              big.data_ptr(), wb, st)
    bwd = lambda wb, out: L.gh_xf_backward(C.byref(dims), C.byref(stem_t), layers_t, x.data_ptr(), tape_big.data_ptr(), dout.data_ptr(), out,
                                           big.data_ptr(), wb, st)
    assert fwd(tneed - 1, need) == _abi.GH_ERR_WORKSPACE_SMALL and fwd(tneed, need - 1) == _abi.GH_ERR_WORKSPACE_SMALL
    assert bwd(bneed - 1, dx.data_ptr()) == _abi.GH_ERR_WORKSPACE_SMALL
    assert bwd(bneed, dout.data_ptr()) == _abi.GH_ERR_INVALID_ARG and bwd(bneed, x.data_ptr()) == _abi.GH_ERR_INVALID_ARG
    buf = torch.full((40, 192), 7.0, device=dev)
    assert L.gh_xf_attention_backward(buf.data_ptr(), 192, buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), 64, 1, 33, 2, 48, dx.data_ptr(), 192,
                                      big.data_ptr(), 1 << 24, st) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_attention_backward(buf.data_ptr(), 192, buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), 64, 1, 33, 2, 32, dx.data_ptr(), 192,
                                      big.data_ptr(), 16, st) == _abi.GH_ERR_WORKSPACE_SMALL
    assert L.gh_xf_geglu_backward(buf.data_ptr(), 48, buf.data_ptr(), 48, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                  buf.data_ptr(), buf.data_ptr(), 4, 48, dx.data_ptr(), 384, st) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_group_norm_backward(x.data_ptr(), x.data_ptr(), buf.data_ptr(), buf.data_ptr(), dout.data_ptr(), dout.data_ptr(), 1, 64, 33, 32,
                                       1e-6, big.data_ptr(), 1 << 24, st) == _abi.GH_ERR_INVALID_ARG
    torch.cuda.synchronize()
    # every refusal came before any launch
    assert float((y - 7.0).abs().max()) == 0.0 and float((dx - 7.0).abs().max()) == 0.0 and int((tape_big != 7).sum()) == 0
    assert torch.equal(dout, rnd(dev, 1, 64, 33, seed=14))
    assert fwd(tneed, need) == _abi.GH_OK and bwd(bneed, dx.data_ptr()) == _abi.GH_OK
    xr = x.clone().requires_grad_(True)
    want, = torch.autograd.grad(X.transformer1d(m, xr, grad="input"), xr, dout)
    assert torch.equal(bits(dx), bits(want))
    with torch.no_grad():
        assert torch.equal(bits(y), bits(X.transformer1d(m, x)))


def test_empty_inputs(dev, X):
    from guassianhand_amd import _abi
    from guassianhand_amd._call import lib, stream
    m = frozen(dev, 64, 2, 32, 1, seed=15)
    for shape in ((0, 64, 33), (2, 64, 0)):
        x = torch.zeros(shape, device=dev, requires_grad=True)
        assert X.kernel_reason(m, x, grad="input") is None
        out = X.transformer1d(m, x, grad="input")
        assert tuple(out.shape) == shape and out.requires_grad
        g, = torch.autograd.grad(out, x, torch.zeros(shape, device=dev))
        assert tuple(g.shape) == shape and g.is_cuda and g.dtype == torch.float32
        dims = _abi.GhXfDims(shape[0], 64, shape[2], 32, 2, 32, 1, 1e-6, 1e-5)
        L = lib()
        assert L.gh_xf_forward_tape(C.byref(dims), None, None, None, None, None, 0, None, 0, stream(dev)) == _abi.GH_OK
        assert L.gh_xf_backward(C.byref(dims), None, None, None, None, None, None, None, 0, stream(dev)) == _abi.GH_OK
