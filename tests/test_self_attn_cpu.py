"""The interaction attention on the host (guassianhand_amd/attention.py): its plain-torch restatement and its SelfAttn module against
outputs and gradients CAPTURED from the reference's own SelfAttn(131) (tests/golden/make_self_attn_fixture.py ->
self_attn_fixture.npz), the module's state-dict keys, the C-ABI's symbols and host-side argument checks, the train-mode rule and the
opt-in renderer names. No GPU compute is launched here."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import _abi
from guassianhand_amd import attention as A
from tests.helpers import header_symbols
from tests.self_attn_cases import F_DIM, KEYS, MATRICES, ROWS, PlainSelfAttn, errors, load_fixture, projected, run_module, sampled


@pytest.fixture(scope="module")
def case(golden_dir):
    return load_fixture(golden_dir)


def _bound(e_ref):
    """Twice the reference's own float32 error against float64, per field; nothing is added."""
    return 2 * e_ref


def test_fixture_keeps_its_promises(case):
    fx = case[0]
    assert abs(float(fx["score_max"]) - 8.0) < 0.05                # scores spread over +-8: the softmax is far from uniform
    assert fx["x_q"].shape == (1, 48, F_DIM) and fx["out_r4"].shape == (1, 12, F_DIM)
    for k in KEYS:
        assert float(abs(case[3][k]).min()) > 0, k                 # no parameter is zero


def test_attention_ref_reproduces_the_reference_self_attn(case):
    """fc(attention_ref(w_qs z, w_ks z, w_vs z)) on the fixture's parameters against the reference's `self_attn(x)`: the output and
    the gradient of x within twice the reference's own float32 error against the same restatement with acc=torch.float64."""
    fx, x, cot, st = case

    def restated(dtype, acc):
        xx = x.to(dtype).clone().requires_grad_(True)
        w = {k: v.to(dtype) for k, v in st.items()}
        q, k, v = (F.linear(xx, w[f"{n}.weight"], w[f"{n}.bias"]).view(1, -1, 4, 32) for n in ("w_qs", "w_ks", "w_vs"))
        out = F.linear(A.attention_ref(q, k, v, 32 ** 0.5, acc=acc), w["fc.weight"], w["fc.bias"])
        (out * cot.to(dtype)).sum().backward()
        return out.detach(), xx.grad

    o32, g32 = restated(torch.float32, None)
    o64, g64 = restated(torch.float64, torch.float64)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    bad = []
    for name, got, want, ref in (("attn_out", o32, fx["attn_out_r4"], o64), ("attn_grad_x", g32, fx["attn_grad_x_r4"], g64)):
        errors(name, got[:, ::ROWS], ref[:, ::ROWS], torch.tensor(want), _bound, bad)
    assert not bad, bad


def test_module_reproduces_the_reference_module(case):
    """attention.SelfAttn with the fixture's state dict, eval(), on the CPU: output, gradient of x and of every parameter within twice
    the reference's own float32 error against the same module in float64."""
    fx, x, cot, st = case
    m = A.SelfAttn(F_DIM).eval()
    m.load_state_dict(st, strict=True)
    m64 = A.SelfAttn(F_DIM).double().eval()
    m64.load_state_dict({k: v.double() for k, v in st.items()}, strict=True)
    y, gx, gp = run_module(m, x, cot)
    y64, gx64, gp64 = run_module(m64, x.double(), cot.double())
    assert y.dtype == torch.float32 and y64.dtype == torch.float64
    bad = []
    errors("out", y[:, ::ROWS], y64[:, ::ROWS], torch.tensor(fx["out_r4"]), _bound, bad)
    errors("grad_x", gx[:, ::ROWS], gx64[:, ::ROWS], torch.tensor(fx["grad_x_r4"]), _bound, bad)
    assert sorted(gp) == sorted(KEYS)
    for k in KEYS:
        name, got = sampled(k, gp[k])
        errors(name, got, sampled(k, gp64[k])[1], torch.tensor(fx[name]), _bound, bad)
        if k in MATRICES:                                           # every row of the matrix's gradient, as one signed sum
            name, got = projected(k, gp[k])
            errors(name, got, projected(k, gp64[k], round32=False)[1], torch.tensor(fx[name]), _bound, bad)
    assert not bad, bad


def test_reference_state_dict_loads_under_the_recorded_keys_and_shapes(case):
    fx, _, _, st = case
    torch.manual_seed(3)
    m = A.SelfAttn(F_DIM)
    sd = m.state_dict()
    init = sorted(k[len("init."):] for k in fx.files if k.startswith("init."))
    assert sorted(sd.keys()) == init == sorted(KEYS)
    for k in init:
        assert tuple(sd[k].shape) == tuple(int(n) for n in fx[f"init.{k}"]), k
    assert (m.n_heads, m.d_q, m.d_v, m.f_dim) == (4, 32, 32, F_DIM) and m.norm == 32 ** 0.5
    assert m.layer_norm.eps == 1e-6 and m.ff.layer_norm.eps == 1e-6
    assert [d.p for d in (m.dropout1, m.dropout2, m.ff.dropout1, m.ff.dropout2)] == [0.1] * 4
    # default initialisation: nn.Linear's uniform within 1 / sqrt(fan_in) (weights and biases), LayerNorm's ones and zeros
    for name in ("w_qs", "w_ks", "w_vs", "fc", "ff.fc1", "ff.fc2"):
        w, b = sd[f"{name}.weight"], sd[f"{name}.bias"]
        lim = w.shape[1] ** -0.5
        assert 0.9 * lim < float(w.abs().max()) <= lim and 0 < float(b.abs().max()) <= lim, name
    assert torch.equal(sd["layer_norm.weight"], torch.ones(F_DIM)) and torch.equal(sd["ff.layer_norm.bias"], torch.zeros(F_DIM))
    m.load_state_dict(st, strict=True)


def test_attention_on_cpu_tensors_is_attention_ref_bitwise():
    g = torch.Generator().manual_seed(2)
    for D in (32, 16):
        q, k, v = (torch.randn(2, 37, 4, D, generator=g) for _ in range(3))
        assert torch.equal(A.attention(q, k, v), A.attention_ref(q, k, v))
        assert torch.equal(A.attention(q, k, v, norm=3.0, ops="torch"), A.attention_ref(q, k, v, 3.0))
    out, lse = A.attention(q, k, v, return_lse=True)
    assert tuple(out.shape) == (2, 37, 64) and tuple(lse.shape) == (2, 4, 37)
    a = q.clone().requires_grad_(True)
    A.attention(a, k, v).sum().backward()
    assert a.grad is not None
    assert tuple(A.attention(q[:, :0], k[:, :0], v[:, :0]).shape) == (2, 0, 64)
    with pytest.raises(ValueError, match="ops"):
        A.attention(q, k, v, ops="eager")
    with pytest.raises(ValueError, match="expected"):
        A.attention(q, k[:, :5], v)
    with pytest.raises(ValueError, match="BS, V, H, D"):
        A.attention(q[0], k[0], v[0])
    with pytest.raises(ValueError, match="norm"):
        A.attention(q, k, v, norm=0.0)
    q64, k64, v64 = (torch.randn(1, 9, 4, 32, generator=g, dtype=torch.float64) for _ in range(3))
    assert torch.equal(A.attention(q64, k64, v64), A.attention_ref(q64, k64, v64))     # any dtype but float32 is the torch path's


def test_grafted_class_in_train_mode_calls_the_base_method(case):
    """fuse_self_attn swaps the class only; train() with p = 0.1 calls the base class's self_attn (a spy counts), eval() and p = 0
    do not."""
    st = case[3]
    base = PlainSelfAttn()
    base.load_state_dict(st, strict=True)
    r = SimpleNamespace(self_attn_layer=base)
    ptrs = [p.data_ptr() for p in base.parameters()]
    assert A.fuse_self_attn(r) is r and r.self_attn_layer is base
    A.fuse_self_attn(r)                                            # idempotent
    assert isinstance(base, PlainSelfAttn) and type(base) is A.fused_self_attn_cls(PlainSelfAttn) and type(base).__name__ == "PlainSelfAttn"
    assert [p.data_ptr() for p in base.parameters()] == ptrs and sorted(base.state_dict()) == sorted(KEYS)
    assert type(base).forward is PlainSelfAttn.forward            # LayerNorm, residual and ff stay the base class's
    x = case[1]
    base.eval()
    want = A.self_attn_core(base, base.layer_norm(x))
    assert torch.equal(base.self_attn(base.layer_norm(x)), want) and base.calls == 0
    base(x)
    assert base.calls == 0                                         # eval: the grafted method, not the base's
    base.train()
    torch.manual_seed(0)
    a = base(x)
    assert base.calls == 1                                         # train with p = 0.1: the base method, dropout included
    plain = PlainSelfAttn()
    plain.load_state_dict(st, strict=True)
    plain.train()
    torch.manual_seed(0)
    assert torch.equal(plain(x), a)
    base.dropout1.p = base.dropout2.p = 0.0
    base(x)
    assert base.calls == 1                                         # train with p = 0: nothing to drop, the grafted method again
    own = SimpleNamespace(self_attn_layer=A.SelfAttn(F_DIM))
    A.fuse_self_attn(own)
    assert type(own.self_attn_layer) is A.SelfAttn                 # the package's own module needs no graft


def test_own_module_keeps_dropout_in_train_mode(case):
    _, x, _, st = case
    m = A.SelfAttn(F_DIM)
    m.load_state_dict(st)
    m.train()
    m.ff.dropout1.p = m.ff.dropout2.p = 0.0                        # only the attention's own dropouts are live
    torch.manual_seed(0)
    a = m(x)
    torch.manual_seed(1)
    assert not torch.equal(a, m(x))
    plain = PlainSelfAttn()
    plain.load_state_dict(st)
    plain.train()
    plain.ff.dropout1.p = plain.ff.dropout2.p = 0.0
    torch.manual_seed(0)
    assert torch.equal(plain(x), a)


def test_library_exports_the_attn_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.ATTN_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_attn(L)
    assert sorted(_abi.ATTN_SYMBOLS) == header_symbols("gh_attn.h")
    assert set(_abi.ATTN_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    hdr = open(gh_lib_path.replace("guassianhand_amd/libgh_raster.so", "include/gh_attn.h")).read()
    for name in ("GH_ATTN_D", "GH_ATTN_MAX_BH"):
        assert f"#define {name} {getattr(_abi, name)}" in hdr, name
    assert "#define GH_ATTN_MAX_V (1 << 30)" in hdr and _abi.GH_ATTN_MAX_V == 1 << 30
    ws = lambda *a: L.gh_attn_workspace_bytes(C.byref(_abi.GhAttnDims(*a)))
    assert ws(1, 12320, 4, 32, 32 ** 0.5) >= 4 * 4 * 12320 and ws(1, 12320, 4, 32, 32 ** 0.5) < 4 * 4 * 12320 + 256
    for dims in ((1, 0, 4, 32, 1.0), (0, 10, 4, 32, 1.0), (1, 10, 4, 16, 1.0), (1, 10, 0, 32, 1.0), (1, 10, 4, 32, 0.0), (16384, 10, 4, 32, 1.0)):
        assert ws(*dims) == 0, dims


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for unsupported shapes, null pointers and a short workspace (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_attn(L)
    one = C.c_void_p(1 << 20)
    t = _abi.GhAttnTensor(1 << 20, 10 * 128, 128, 32)
    hole = _abi.GhAttnTensor(None, 10 * 128, 128, 32)
    odd = _abi.GhAttnTensor((1 << 20) + 2, 10 * 128, 128, 32)
    bad, uns = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED

    def fwd(dims=(1, 10, 4, 32, 5.0), q=t, k=t, v=t, out=one, lse=one):
        return L.gh_attn_forward(C.byref(_abi.GhAttnDims(*dims)), C.byref(q) if q else None, C.byref(k), C.byref(v), out, lse, None)

    assert fwd((1, 10, 4, 16, 5.0)) == fwd((1, 10, 4, 64, 5.0)) == fwd((1, 10, 65536, 32, 5.0)) == fwd((16384, 10, 4, 32, 5.0)) == uns
    assert fwd((1, (1 << 30) + 1, 4, 32, 5.0)) == uns
    assert fwd((1, 10, 4, 32, 0.0)) == fwd((1, 10, 4, 32, float("nan"))) == fwd((1, -1, 4, 32, 5.0)) == fwd((1, 10, 0, 32, 5.0)) == bad
    assert fwd(q=None) == fwd(q=hole) == fwd(k=hole) == fwd(v=odd) == fwd(out=None) == fwd(lse=None) == bad
    assert L.gh_attn_forward(None, C.byref(t), C.byref(t), C.byref(t), one, one, None) == bad
    assert fwd((1, 0, 4, 32, 5.0)) == fwd((0, 10, 4, 32, 5.0)) == _abi.GH_OK                  # no rows: nothing to launch
    assert fwd((1, 0, 4, 16, 5.0)) == uns                                                    # the shape is judged first

    def bwd(dims=(1, 10, 4, 32, 5.0), q=t, g=t, out=one, dq=one, dk=one, dv=one, ws=one, nbytes=1 << 20):
        return L.gh_attn_backward(C.byref(_abi.GhAttnDims(*dims)), C.byref(q), C.byref(t), C.byref(t), out, one, C.byref(g), dq, dk, dv,
                                  ws, nbytes, None)

    assert bwd((1, 10, 4, 16, 5.0)) == uns
    assert bwd(q=hole) == bwd(g=hole) == bwd(out=None) == bwd(ws=None) == bwd(ws=C.c_void_p((1 << 20) + 4)) == bad
    assert bwd(nbytes=16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert bwd(dq=None, dk=None, dv=None, ws=None, nbytes=0) == _abi.GH_OK                   # nothing asked for
    assert bwd((1, 0, 4, 32, 5.0), ws=None, nbytes=0) == _abi.GH_OK


def test_opt_in_renderer_names_resolve_lazily():
    """tgs_renderer's four names with the attention core, and no other name, apply it last; the rows without it keep theirs."""
    import guassianhand_amd.tgs_renderer as T
    assert T._VARIANTS["FusedAttn"] == ("attn",) and T._VARIANTS["FusedAllFetchAttn"] == ("gate", "head", "fetch", "attn")
    assert [s for s, row in T._VARIANTS.items() if row[-1] == "attn"] == ["FusedAttn", "FusedAllFetchAttn"]
    assert all("attn" not in row for s, row in T._VARIANTS.items() if "Attn" not in s)
    assert T._GRAFTS["attn"][:2] == ("attention", "fuse_self_attn") and all(len(row) == 3 and isinstance(row[2], str) for row in T._GRAFTS.values())
    with pytest.raises(AttributeError):
        T.GS3DRendererFusedAttnNothing
    import importlib.util
    have_reference = importlib.util.find_spec("tgs") is not None
    for name in ("GS3DRendererFusedAttn", "GS3DRendererEditFusedAttn", "GS3DRendererFusedAllFetchAttn", "GS3DRendererEditFusedAllFetchAttn"):
        if not have_reference:                                     # the name is known: resolving it reaches for the reference's classes
            with pytest.raises(ImportError) as e:
                getattr(T, name)
            assert (e.value.name or "").split(".")[0] == "tgs"      # and for nothing else that is missing
            continue
        cls = getattr(T, name)
        assert isinstance(cls, type) and callable(cls.configure)
