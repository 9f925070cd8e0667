"""The Transformer1D backward to the input (transformer1d's grad="input") without a device: the fallback and its gradient, the
default's unchanged reasons, the second seam class, the ABI mirror of what include/gh_xf.h gained, and the gelu' formula."""
import ctypes as C
import os
import pickle
import re

import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import _abi
from guassianhand_amd import transformer1d as X
from tests import transformer1d_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frozen(seed=21):
    m = K.make_module(64, 2, 32, 1, seed=seed)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_grad_input_on_the_cpu_falls_back_with_the_restatements_gradient():
    m = _frozen()
    x = K.make_x(2, 64, 13).requires_grad_(True)
    assert X.kernel_reason(m, x, grad="input") == "x is not on a ROCm device"
    dout = torch.randn(2, 64, 13, generator=torch.Generator().manual_seed(5))
    want, = torch.autograd.grad(X.transformer1d_ref(X.params_of(m), x), x, dout)
    for how in ("function", "params", "module", "seam"):
        if how == "function":
            out = X.transformer1d(m, x, grad="input")
        elif how == "params":
            out = X.transformer1d(X.params_of(m), x, grad="input")
        elif how == "module":
            s = X.Transformer1D(64, 2, 32, 1, cross_attention_dim=64)
            s.load_state_dict(m.state_dict())
            s.requires_grad_(False)
            out = s(x, grad="input")
        else:
            n = K.StandIn.calls
            out = X.fuse_transformer1d(_frozen(), grad="input")(x)
            assert K.StandIn.calls == n + 1
        got, = torch.autograd.grad(out, x, dout)
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), how
    assert torch.equal(torch.autograd.grad(X.transformer1d(m, x, grad="input"), x, dout)[0], want)   # the same statements


def test_default_keeps_its_reasons():
    m = _frozen()
    x = K.make_x(2, 64, 13).requires_grad_(True)
    assert X.kernel_reason(m, x) == X.kernel_reason(m, x, grad="none") == "x is not on a ROCm device"
    # the order of the checks on a device is pinned through _params_reason with the device test taken out of the way
    class OnDevice(torch.Tensor):
        is_cuda = True

    p = X.params_of(m)
    xd = x.detach().as_subclass(OnDevice).requires_grad_(True)
    assert X._params_reason(p, xd) == "a gradient is wanted" and X._params_reason(p, xd, "none") == "a gradient is wanted"
    assert X._params_reason(p, xd, "input") is None
    w = m.transformer_blocks[0].attn1.to_q.weight.requires_grad_(True)
    assert X._params_reason(p, xd) == "a gradient is wanted" and X._params_reason(p, xd, "input") == "a parameter wants a gradient"
    assert X._params_reason(p, xd.detach().as_subclass(OnDevice), "input") == "a parameter wants a gradient"
    w.requires_grad_(False)
    with torch.no_grad():
        assert X._params_reason(p, xd, "input") is None and X._params_reason(p, xd) is None
    with pytest.raises(ValueError):
        X.kernel_reason(m, x, grad="all")
    with pytest.raises(ValueError):
        X.transformer1d(m, x, grad="weights")


def test_grad_input_refuses_a_backbone_wider_than_the_data_product():
    """M = 1024 runs the forward kernels but not the taped pair: 8 M would exceed GH_XF_MAX_K."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    m = K.make_module(64, 16, 64, 1, seed=3)
    m.requires_grad_(False)
    p = X.params_of(m)
    x = K.make_x(1, 64, 3).as_subclass(OnDevice).requires_grad_(True)
    assert X._params_reason(p, x, "input") == "sizes"
    with torch.no_grad():
        assert X._params_reason(p, x, "input") is None
    assert 8 * _abi.GH_XF_GRAD_MAX_M == _abi.GH_XF_MAX_K


def test_seam_classes():
    a, b = X.fused_transformer1d_cls(K.StandIn), X.fused_transformer1d_cls(K.StandIn, grad="input")
    assert a is not b and a is X.fused_transformer1d_cls(K.StandIn, grad="none") and b is X.fused_transformer1d_cls(K.StandIn, "input")
    assert issubclass(b, K.StandIn) and b._gh_grad == "input" and a._gh_grad == "none"
    m = X.fuse_transformer1d(_frozen(8), grad="input")
    assert type(m) is b and type(X.fuse_transformer1d(m, grad="input")) is b
    back = pickle.loads(pickle.dumps(m))
    assert type(back) is b
    for (k, v), (k2, v2) in zip(m.state_dict().items(), back.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    assert type(X.fuse_transformer1d(m)) is a                     # the other grad swaps the class, the base stays
    import importlib
    mod = importlib.import_module("guassianhand_amd.tgs_backbone")
    assert mod._GRAD == {"Transformer1D": "none", "Transformer1DGrad": "input"}
    with pytest.raises(AttributeError):
        mod.Transformer1DGradient


def test_abi_mirror_of_the_backward():
    txt = open(os.path.join(ROOT, "include", "gh_xf.h")).read()
    for name in ("GH_XF_PRO_CF", "GH_XF_ATTN_BWD_ROWS", "GH_XF_ATTN_BWD_STAGE", "GH_XF_GRAD_MAX_M"):
        value = re.search(r"^#define %s (\d+)" % name, txt, flags=re.M).group(1)
        assert getattr(_abi, name) == int(value), name
    assert X.PROLOGUES["cf"] == _abi.GH_XF_PRO_CF == 3 and _abi.GH_XF_MAX_K == 4096
    for cls, struct in ((_abi.GhXfStemT, "GhXfStemT"), (_abi.GhXfLayerT, "GhXfLayerT")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert [f for f, _ in cls._fields_] == re.findall(r"\*\s*(\w+)", body), struct
        assert C.sizeof(cls) == 8 * len(cls._fields_)
    assert C.sizeof(_abi.GhXfStemT) == 3 * 8 and C.sizeof(_abi.GhXfLayerT) == 12 * 8
    new = ("gh_xf_attention_lse", "gh_xf_attention_backward_workspace_bytes", "gh_xf_attention_backward", "gh_xf_geglu_backward",
           "gh_xf_layernorm_backward", "gh_xf_group_norm_backward_workspace_bytes", "gh_xf_group_norm_backward", "gh_xf_tape_bytes",
           "gh_xf_forward_tape", "gh_xf_backward_workspace_bytes", "gh_xf_backward")
    assert set(new) <= set(_abi.XF_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    for sym in new:
        assert re.search(r"^\s*(?:int|size_t)\s+%s\s*\(" % sym, txt, flags=re.M), sym


def test_host_sizes_of_the_backward(gh_lib_path):
    """Pure host arithmetic: the tape's and the workspace's sizes as the header lays them out, and the refusals."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    al = lambda n: (n + 255) & ~255
    B, N, heads, D, G, Cc, layers = 1, 2048, 8, 64, 32, 512, 10
    T, M = B * N, heads * D
    ok = _abi.GhXfDims(B, Cc, N, G, heads, D, layers, 1e-6, 1e-5)
    attn = al(T * M * 4) + al(T * 8) + al(T * 3 * M * 4) + al(T * M * 4) + al(T * heads * 4)
    ff = al(T * M * 4) + al(T * 8)
    assert L.gh_xf_tape_bytes(C.byref(ok)) == al(B * G * 8) + layers * (2 * attn + ff)
    chunks = (N + 255) // 256
    assert L.gh_xf_backward_workspace_bytes(C.byref(ok)) == 2 * al(T * M * 4) + al(T * 8 * M * 4) + al(T * heads * 4) + al(T * Cc * 4) + \
        al(B * G * chunks * 8) + al(B * G * 8)
    for bad in (_abi.GhXfDims(1, 512, 2048, 32, 16, 64, 10, 1e-6, 1e-5), _abi.GhXfDims(1, 512, 2048, 32, 8, 48, 10, 1e-6, 1e-5),
                _abi.GhXfDims(0, 512, 2048, 32, 8, 64, 10, 1e-6, 1e-5)):
        assert L.gh_xf_tape_bytes(C.byref(bad)) == 0 and L.gh_xf_backward_workspace_bytes(C.byref(bad)) == 0
    wide = _abi.GhXfDims(1, 512, 2048, 32, 16, 64, 10, 1e-6, 1e-5)            # M = 1024
    assert L.gh_xf_workspace_bytes(C.byref(wide)) > 0                        # the forward takes it
    assert L.gh_xf_forward_tape(C.byref(wide), None, None, None, None, None, 0, None, 0, None) == _abi.GH_ERR_UNSUPPORTED
    assert L.gh_xf_backward(C.byref(wide), None, None, None, None, None, None, None, 0, None) == _abi.GH_ERR_UNSUPPORTED


@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (-6.0, 6.0)])
def test_gelu_grad_formula_is_autograds(lo, hi):
    g = torch.linspace(lo, hi, 4001, dtype=torch.float64).requires_grad_(True)
    want, = torch.autograd.grad(F.gelu(g).sum(), g)
    got = X.gelu_grad(g.detach())
    # the formula's constants carry eight digits: 0.70710678 and 0.39894228 are within 5e-10 of 1 / sqrt 2 and 1 / sqrt(2 pi), and g exp(-g^2 / 2) <= 0.61
    assert float((got - want).abs().max()) <= 1e-9
