"""The Transformer1D kernels (include/gh_xf.h) on the device. The criterion is tests/fit_cases.three_way: the kernel, the float32 torch
statements and the float64 ones run on the device on the same inputs, and per field
max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64|; the three errors are printed. Weights are scaled by 1 / sqrt(K).

Whole-stack error ratios (kernel error over the bound) are recorded under the names "xf_stack_*" by fit_cases.three_way."""
import ctypes as C

import pytest
import torch

from tests import transformer1d_cases as K
from tests.fit_cases import bits, three_way

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert (_abi.GH_XF_ROWS, _abi.GH_XF_COLS, _abi.GH_XF_ATTN_ROWS, _abi.GH_XF_ATTN_KEYS, _abi.GH_XF_GN_CHUNK) == \
        (K.ROW_TILE, K.COL_TILE, K.ATTN_ROWS, K.ATTN_KEYS, K.GN_CHUNK)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def X():
    from guassianhand_amd import transformer1d
    return transformer1d


# ---- gh_xf_linear ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", K.EPILOGUES)
@pytest.mark.parametrize("pro", K.PROLOGUES)
@pytest.mark.parametrize("T,Kin,n_out", K.LINEAR_SHAPES)
def test_linear_every_prologue_and_epilogue(dev, T, Kin, n_out, pro, epi):
    d = K.linear_inputs(T, Kin, n_out, pro, epi, seed=T + n_out, device=dev)
    got = K.linear_kernel(d, pro, epi)
    three_way({"y": got}, {"y": K.linear_ref(d, pro, epi, torch.float32)}, {"y": K.linear_ref(d, pro, epi, torch.float64)}, ("y",),
              tag=f"linear T={T} K={Kin} N_out={n_out} {pro} {epi}")


@pytest.mark.parametrize("pro", ["none", "ln"])
@pytest.mark.parametrize("T,Kin,n_out", [(65, 64, 65), (129, 512, 64)])
def test_linear_strided_misaligned_view_is_bitwise_its_copy(dev, T, Kin, n_out, pro):
    d = K.linear_inputs(T, Kin, n_out, pro, "bias_res", seed=7, device=dev)
    want = K.linear_kernel(d, pro, "bias_res")
    d2 = dict(d, res=K.strided_misaligned(d["res"]))
    got = K.linear_kernel(d2, pro, "bias_res", x=K.strided_misaligned(d["x"]))
    assert torch.equal(bits(got), bits(want))


def test_linear_row_does_not_depend_on_its_place(dev):
    """Rows 70 .. 72 alone (tile rows 0 .. 2) and among 257 (tile rows 6 .. 8 of the second tile), through LN and the GEGLU."""
    for pro, epi in (("ln", "geglu"), ("none", "bias_res"), ("ln", "plain")):
        d = K.linear_inputs(257, 64, 65, pro, epi, seed=8, device=dev)
        full = K.linear_kernel(d, pro, epi)
        part = K.linear_kernel(dict(d, x=d["x"][70:73], res=d["res"][70:73]), pro, epi)
        assert torch.equal(bits(part), bits(full[70:73])), (pro, epi)
        again = K.linear_kernel(d, pro, epi)
        assert torch.equal(bits(again), bits(full))


# ---- gh_xf_group_moments and the GroupNorm prologue ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 257, 2 * K.GN_CHUNK + 1])
@pytest.mark.parametrize("Cc", [32, 64])
def test_group_moments(dev, X, Cc, N):
    x = K.make_x(2, Cc, N, seed=N, device=dev) + 0.5
    got = X.group_moments(x, 32)

    def ref(t):
        g = t.reshape(2, 32, -1)
        mean = g.mean(dim=2)
        return {"mean": mean, "m2": (g - mean[..., None]).square().sum(dim=2)}

    three_way({"mean": got[..., 0], "m2": got[..., 1]}, ref(x), ref(x.double()), ("mean", "m2"), tag=f"group moments C={Cc} N={N}")
    assert torch.equal(bits(X.group_moments(x, 32)), bits(got))
    # a batch element's moments do not depend on its slot
    assert torch.equal(bits(X.group_moments(x[1:], 32)), bits(got[1:]))


def test_group_norm_of_one_value_is_exactly_its_bias(dev, X):
    """C = 32, G = 32, N = 1: every group is one value, its mean that value and its deviation 0, so the norm gives beta exactly; the
    identity weight passes it through the product unchanged."""
    d = K.linear_inputs(3, 32, 32, "gn", "plain", seed=9, device=dev)
    x = K.make_x(3, 32, 1, seed=9, device=dev) * 100
    mom = X.group_moments(x, 32)
    assert torch.equal(mom[..., 0], x[:, :, 0]) and float(mom[..., 1].abs().max()) == 0.0
    y = X.linear(x, torch.eye(32, device=dev), prologue="gn", gamma=d["gamma"], beta=d["beta"], eps=1e-6, groups=32, moments=mom)
    assert torch.equal(y, d["beta"].expand(3, 32))


# ---- gh_xf_attention -------------------------------------------------------------------------------------------------------------------
def make_qkv(dev, B, N, heads, D, seed=0):
    gen = torch.Generator().manual_seed(4000 + seed)
    return (torch.randn(B * N, 3 * heads * D, generator=gen) * torch.tensor([2.0, 1.0, 1.0]).repeat_interleave(heads * D)).to(dev)


@pytest.mark.parametrize("N", K.ATTN_N)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 2, 8])
@pytest.mark.parametrize("D", [32, 64])
def test_attention(dev, X, D, heads, B, N):
    qkv = make_qkv(dev, B, N, heads, D, seed=N)
    got = X.attention(qkv, B, N, heads, D)
    three_way({"out": got}, {"out": K.attention_ref(qkv, B, N, heads, D, torch.float32)}, {"out": K.attention_ref(qkv, B, N, heads, D, torch.float64)},
              ("out",), tag=f"attention D={D} heads={heads} B={B} N={N}")


@pytest.mark.parametrize("D", [32, 64])
def test_attention_bitwise_properties(dev, X, D):
    heads, N = 2, 257
    M = heads * D
    qkv = make_qkv(dev, 1, N, heads, D, seed=1)
    out = X.attention(qkv, 1, N, heads, D)
    assert torch.equal(bits(X.attention(qkv, 1, N, heads, D)), bits(out))
    # a query's result is a function of its q, K and V: every other query replaced
    other = qkv.clone()
    other[:, :M] = torch.randn(N, M, device=dev)
    for r in (0, 31, 32, 100, 256):
        other[r, :M] = qkv[r, :M]
    got = X.attention(other, 1, N, heads, D)
    for r in (0, 31, 32, 100, 256):
        assert torch.equal(bits(got[r]), bits(out[r])), r
    # a batch element's result does not depend on B or on its slot; a strided, misaligned buffer is read in place
    b3 = torch.cat([make_qkv(dev, 1, N, heads, D, seed=2), qkv, qkv], dim=0)
    o3 = X.attention(b3, 3, N, heads, D)
    assert torch.equal(bits(o3[N:2 * N]), bits(out)) and torch.equal(bits(o3[2 * N:]), bits(out))
    assert torch.equal(bits(X.attention(K.strided_misaligned(qkv), 1, N, heads, D)), bits(out))


# ---- the whole stack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.STACKS, ids=lambda c: "C%d_h%d_D%d_L%d_B%d_N%d_%s" % (*c[:6], "attn2" if c[6] else "noattn2"))
def test_whole_stack(dev, X, case):
    Cc, heads, D, layers, B, N, attn2 = case
    m, x, f64, t32 = K.stack_case(case, str(dev))
    name = "xf_stack_C%d_h%d_D%d_L%d_B%d_N%d" % case[:6] + ("" if attn2 else "_noattn2")
    with torch.no_grad():
        assert X.kernel_reason(m, x) is None
        got = X.transformer1d(X.params_of(m), x)
        three_way({"out": got}, {"out": t32}, {"out": f64}, ("out",), tag=name, name=name)
        s = X.Transformer1D(Cc, heads, D, layers, cross_attention_dim=heads * D if attn2 else None).to(dev)
        s.load_state_dict(m.state_dict())
        assert torch.equal(bits(s(x)), bits(got)) and torch.equal(bits(X.transformer1d(m, x)), bits(got))
        n = K.StandIn.calls
        fused = X.fuse_transformer1d(K.make_module(Cc, heads, D, layers, attn2=attn2, seed=layers, device=dev))
        assert torch.equal(bits(fused(x)), bits(got)) and K.StandIn.calls == n    # the base forward did not run
        assert torch.equal(bits(fused(x)), bits(got))                               # two runs are equal
        # a batch element does not depend on B or on its slot
        x3 = torch.cat([x[-1:], K.make_x(1, Cc, N, seed=99, device=dev), x[-1:]], dim=0)
        o3 = s(x3)
        assert torch.equal(bits(o3[0]), bits(got[-1])) and torch.equal(bits(o3[2]), bits(got[-1]))
    assert not got.requires_grad and X.kernel_reason(m, x) == "a gradient is wanted"   # grad mode on, trainable parameters


def test_fused_module_called_as_forward_calls_it(dev, X):
    """TGS._forward's call, `backbone(tokens, modulation_cond=<tensor>)`: the kernels run, the base class's forward does not, and the
    result is bitwise the kernel result without the argument."""
    m = X.fuse_transformer1d(K.make_module(64, 2, 32, 2, seed=17, device=dev))
    x, cond = K.make_x(2, 64, 129, seed=17, device=dev), torch.randn(2, 1, 32, device=dev)
    with torch.no_grad():
        want = X.transformer1d(X.params_of(m), x)
        n = K.StandIn.calls
        got = m(x, modulation_cond=cond)
        also = m(x, modulation_cond=cond.requires_grad_(True), timestep=None, class_labels=None)
        assert K.StandIn.calls == n and torch.equal(bits(got), bits(want)) and torch.equal(bits(also), bits(want))
        m(x, modulation_cond=cond, cross_attention_kwargs={"scale": 1.0})
        assert K.StandIn.calls == n + 1


def test_refresh_after_an_update_behind_autograd(dev, X):
    m = K.make_module(64, 2, 32, 1, seed=18, device=dev)
    x = K.make_x(1, 64, 33, device=dev)
    with torch.no_grad():
        X.transformer1d(m, x)
        m.transformer_blocks[0].attn1.to_q.weight.data.mul_(0.5)       # moves neither the version counter nor the storage
        X.refresh(m)
        assert torch.equal(bits(X.transformer1d(m, x)), bits(X.transformer1d(X.params_of(m), x)))


def test_cached_weights_follow_the_parameters(dev, X):
    m = K.make_module(64, 2, 32, 1, seed=11, device=dev)
    x = K.make_x(1, 64, 33, device=dev)
    with torch.no_grad():
        a = X.transformer1d(m, x)
        m.transformer_blocks[0].attn1.to_q.weight.mul_(0.5)           # bumps the version counter
        b = X.transformer1d(m, x)
        assert not torch.equal(a, b) and torch.equal(bits(b), bits(X.transformer1d(X.params_of(m), x)))


def test_graph_capture_replays_bitwise(dev, X):
    m = X.fuse_transformer1d(K.make_module(64, 2, 32, 2, seed=12, device=dev))
    x = K.make_x(2, 64, 129, seed=12, device=dev)
    with torch.no_grad():
        eager = m(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(x)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(eager))
        x.copy_(K.make_x(2, 64, 129, seed=13, device=dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(m(x)))


# ---- return codes, empty inputs, fallback ----------------------------------------------------------------------------------------------
def test_return_codes(dev, X):
    from guassianhand_amd import _abi
    from guassianhand_amd._call import lib, stream, workspace
    L = lib()
    buf = torch.zeros(64, 3 * 1056, device=dev)
    out = torch.zeros(64, 1056, device=dev)
    st = stream(dev)
    assert L.gh_xf_attention(buf.data_ptr(), 3 * 96, 1, 64, 2, 48, out.data_ptr(), 96, st) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_attention(buf.data_ptr(), 3 * 1056, 1, 64, 33, 32, out.data_ptr(), 1056, st) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_attention(buf.data_ptr(), 3 * 64, 1, 0, 2, 32, out.data_ptr(), 64, st) == _abi.GH_OK
    m = K.make_module(64, 2, 32, 1, seed=14, device=dev)
    p = X._Packed(X.params_of(m))
    x = K.make_x(1, 64, 33, device=dev)
    y = torch.full_like(x, 7.0)
    for heads, D in ((2, 48), (33, 32)):
        dims = _abi.GhXfDims(1, 64, 33, 32, heads, D, 1, 1e-6, 1e-5)
        assert L.gh_xf_workspace_bytes(C.byref(dims)) == 0
        assert L.gh_xf_forward(C.byref(dims), C.byref(p.stem), p.layers, x.data_ptr(), y.data_ptr(), None, 0, st) == _abi.GH_ERR_UNSUPPORTED
    dims = _abi.GhXfDims(1, 64, 33, 32, 2, 32, 1, 1e-6, 1e-5)
    need = L.gh_xf_workspace_bytes(C.byref(dims))
    ws = workspace(need, dev)
    assert L.gh_xf_forward(C.byref(dims), C.byref(p.stem), p.layers, x.data_ptr(), y.data_ptr(), ws.data_ptr(), need - 1, st) == _abi.GH_ERR_WORKSPACE_SMALL
    a = _abi.GhXfLinear(T=33, K=64, N_out=64, prologue=_abi.GH_XF_PRO_LN, epilogue=_abi.GH_XF_EPI_PLAIN, eps=1e-5, x=buf.data_ptr(), x_stride=64,
                        w=buf.data_ptr(), gamma=buf.data_ptr(), beta=buf.data_ptr(), y=out.data_ptr(), y_stride=64)
    assert L.gh_xf_linear(C.byref(a), ws.data_ptr(), L.gh_xf_linear_workspace_bytes(33, _abi.GH_XF_PRO_LN) - 1, st) == _abi.GH_ERR_WORKSPACE_SMALL
    a.K = 48
    assert L.gh_xf_linear(C.byref(a), ws.data_ptr(), need, st) == _abi.GH_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float((y - 7.0).abs().max()) == 0.0 and float(out.abs().max()) == 0.0     # refused before any launch
    assert L.gh_xf_forward(C.byref(dims), C.byref(p.stem), p.layers, x.data_ptr(), y.data_ptr(), ws.data_ptr(), need, st) == _abi.GH_OK
    with torch.no_grad():
        assert torch.equal(bits(y), bits(X.transformer1d(m, x)))


def test_empty_inputs(dev, X):
    m = K.make_module(64, 2, 32, 1, seed=15, device=dev)
    with torch.no_grad():
        for shape in ((0, 64, 33), (2, 64, 0)):
            x = torch.zeros(shape, device=dev)
            assert X.kernel_reason(m, x) is None
            out = X.transformer1d(m, x)
            assert tuple(out.shape) == shape and out.is_cuda and out.dtype == torch.float32


def test_trainable_parameter_falls_back_on_the_device(dev, X):
    m = K.make_module(64, 2, 32, 1, seed=16, device=dev)
    x = K.make_x(2, 64, 33, device=dev)
    for p in m.parameters():
        p.requires_grad_(False)
    w = m.transformer_blocks[0].attn1.to_q.weight.requires_grad_(True)
    assert X.kernel_reason(m, x) == "a gradient is wanted"
    n = K.StandIn.calls
    out = X.fuse_transformer1d(m)(x)
    assert K.StandIn.calls == n + 1 and out.requires_grad
    out.square().sum().backward()
    assert bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0
    with torch.no_grad():
        assert X.kernel_reason(m, x) is None
