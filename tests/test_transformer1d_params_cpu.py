"""The Transformer1D backward to the parameters (transformer1d's grad="params") without a device: the accepted keyword, the reasons with
the device test out of the way, the fallback and its gradients, the third seam class, and the ABI mirror of what include/gh_xf.h gained."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import transformer1d as X
from tests import transformer1d_cases as K
from tests import transformer1d_params_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OnDevice(torch.Tensor):
    is_cuda = True


def _frozen(*a, **kw):
    return K.make_module(*a, **kw).requires_grad_(False)


def test_params_is_a_gradient_mode_and_the_others_still_raise():
    m = _frozen(64, 2, 32, 1, seed=21)
    x = K.make_x(2, 64, 13)
    assert X.GRADS == ("none", "input", "params")
    assert X.kernel_reason(m, x, grad="params") == "x is not on a ROCm device"
    assert tuple(X.transformer1d(m, x, grad="params").shape) == (2, 64, 13)
    for bad in ("all", "weights"):
        with pytest.raises(ValueError):
            X.kernel_reason(m, x, grad=bad)
        with pytest.raises(ValueError):
            X.transformer1d(m, x, grad=bad)
        with pytest.raises(ValueError):
            X.fused_transformer1d_cls(K.StandIn, bad)


def test_a_trainable_parameter_is_no_reason_under_params():
    m = _frozen(64, 2, 32, 1, seed=21)
    p = X.params_of(m)
    xd = K.make_x(2, 64, 13).as_subclass(OnDevice)
    w = m.transformer_blocks[0].attn1.to_q.weight.requires_grad_(True)
    assert X._params_reason(p, xd, "params") is None
    assert X._params_reason(p, xd.detach().as_subclass(OnDevice).requires_grad_(True), "params") is None
    # the other two modes answer as before
    assert X._params_reason(p, xd, "input") == "a parameter wants a gradient" and X._params_reason(p, xd, "none") == "a gradient is wanted"
    w.requires_grad_(False)
    m.norm.bias.requires_grad_(True)
    assert X._params_reason(p, xd, "params") is None and X._params_reason(p, xd, "input") == "a parameter wants a gradient"


def test_params_refuses_a_backbone_wider_than_the_data_product():
    m = K.make_module(64, 16, 64, 1, seed=3)                      # M = 1024, every parameter trainable
    p = X.params_of(m)
    x = K.make_x(1, 64, 3).as_subclass(OnDevice)
    assert X._params_reason(p, x, "params") == "sizes"
    with torch.no_grad():
        assert X._params_reason(p, x, "params") is None           # nothing to tape: the forward takes M = 1024
    m.requires_grad_(False)
    assert X._params_reason(p, x, "params") is None
    assert X._params_reason(p, x.detach().as_subclass(OnDevice).requires_grad_(True), "params") == "sizes"


def _break(kind):
    """(a module changed in one way, x on the pretended device, the reason every mode gives)."""
    m = K.make_module(64, 2, 32, 1, seed=5)
    x = K.make_x(1, 64, 5)
    if kind == "cpu":
        return m, x, "x is not on a ROCm device"
    x = x.as_subclass(OnDevice)
    if kind == "rank":
        return m, x[0], "x is not a (B, C, N) tensor"
    if kind == "dtype":
        return m, x.double().as_subclass(OnDevice), "not float32 on one device"
    if kind == "channels":
        return m, K.make_x(1, 32, 5).as_subclass(OnDevice), "sizes"
    if kind == "attention_bias":
        m.transformer_blocks[0].attn1.to_q.bias = torch.nn.Parameter(torch.zeros(64))
        return m, x, "attention_bias"
    if kind == "eps":
        m2 = K.make_module(64, 2, 32, 2, seed=5)
        m2.transformer_blocks[1].norm1.eps = 1e-3
        return m2, x, "blocks with different LayerNorm eps"
    if kind == "ff":
        m.transformer_blocks[0].ff.net[2] = torch.nn.Linear(128, 64)
        return m, x, "a feed-forward that is not M -> 8M -> M"
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["cpu", "rank", "dtype", "channels", "attention_bias", "eps", "ff"])
def test_every_other_reason_is_unchanged(kind):
    m, x, want = _break(kind)
    p = X.params_of(m)
    for trainable in (True, False):
        m.requires_grad_(trainable)
        with torch.no_grad():                                     # no gradient in play: the three modes see the same call
            assert X._params_reason(p, x, "none") == X._params_reason(p, x, "input") == X._params_reason(p, x, "params") == want, kind
    m.requires_grad_(True)
    assert X._params_reason(p, x, "params") == want               # and the trainable parameters do not get in front of it
    assert X.kernel_reason(m, x, grad="params", attention_mask=torch.ones(1, 5)) == "encoder_hidden_states or a mask"


def test_on_the_cpu_params_is_the_restatement_and_its_gradients_are_autograds():
    m, x = P.trainable((64, 2, 32, 2, 2, 13, True))
    x.requires_grad_(True)
    dout = torch.randn(2, 64, 13, generator=torch.Generator().manual_seed(5))
    want, wout = P.module_grads(lambda t: X.transformer1d_ref(X.params_of(m), t), m, x, dout)
    assert len(want) == 1 + len(list(m.parameters()))
    for f in (lambda t: X.transformer1d(m, t, grad="params"), lambda t: X.transformer1d(X.params_of(m), t, grad="params")):
        got, out = P.module_grads(f, m, x, dout)
        assert torch.equal(out, wout)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    s = X.Transformer1D(64, 2, 32, 2, cross_attention_dim=64)
    s.load_state_dict(m.state_dict())
    got, out = P.module_grads(lambda t: s(t, grad="params"), s, x, dout)
    assert torch.equal(out, wout) and all(torch.equal(got[k], want[k]) for k in want)
    n = K.StandIn.calls
    fused = X.fuse_transformer1d(P.trainable((64, 2, 32, 2, 2, 13, True))[0], grad="params")
    got, _ = P.module_grads(fused, fused, x, dout)
    assert K.StandIn.calls == n + 1                               # the seam's fallback is the base class's own forward
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-5 * max(float(want[k].abs().max()), 1.0), k


def test_the_third_seam_class_resolves_lazily():
    mod = importlib.import_module("guassianhand_amd.tgs_backbone")     # importing it needs no reference checkout
    assert mod._TRAIN == {"Transformer1DTrain": "params"} and "Transformer1DTrain" in mod.__doc__
    with pytest.raises(AttributeError):
        mod.Transformer1DTraining
    try:
        importlib.import_module("tgs.models.transformers")
    except ImportError:
        with pytest.raises(ImportError):                          # the name is known: resolving it is what needs the reference
            mod.Transformer1DTrain
    a, b, c = (X.fused_transformer1d_cls(K.StandIn, g) for g in X.GRADS)
    assert len({a, b, c}) == 3 and c._gh_grad == "params" and issubclass(c, K.StandIn) and "parameter" in c.__doc__
    m = X.fuse_transformer1d(K.make_module(64, 2, 32, 1, seed=8), grad="params")
    assert type(m) is c and type(X.fuse_transformer1d(m, grad="params")) is c and type(X.fuse_transformer1d(m)) is a


def test_grad_slots_follow_the_tensor_order():
    for attn2 in (True, False):
        m = K.make_module(64, 2, 32, 2, attn2=attn2, seed=1)
        p = X.params_of(m)
        ts, slots = X._tensors(p), X._grad_slots(p)
        assert len(ts) == len(slots) == len(list(m.parameters()))
        packed_fields = {None: dict(zip(_abi.XF_STEM, (*p["norm"], *p["proj_in"], *p["proj_out"])))}
        for i, b in enumerate(p["blocks"]):
            f = {"ln1_w": b["norm1"][0], "ln1_b": b["norm1"][1], "ln3_w": b["norm3"][0], "ln3_b": b["norm3"][1], "ff1_w": b["ff1"][0],
                 "ff1_b": b["ff1"][1], "ff2_w": b["ff2"][0], "ff2_b": b["ff2"][1], "qkv1": [b["attn1"][k] for k in "qkv"],
                 "o1_w": b["attn1"]["o_w"], "o1_b": b["attn1"]["o_b"]}
            if attn2:
                f.update(ln2_w=b["norm2"][0], ln2_b=b["norm2"][1], qkv2=[b["attn2"][k] for k in "qkv"], o2_w=b["attn2"]["o_w"], o2_b=b["attn2"]["o_b"])
            packed_fields[i] = f
        for t, (layer, field, block) in zip(ts, slots):
            want = packed_fields[layer][field]
            assert t is (want if block is None else want[block]), (layer, field, block)


def test_abi_mirror_of_the_parameter_gradients():
    txt = open(os.path.join(ROOT, "include", "gh_xf.h")).read()
    for name in ("GH_XF_WGRAD_ROWS", "GH_XF_WGRAD_CHUNK", "GH_XF_WGRAD_MAX_BLOCKS", "GH_XF_LNP_ROWS"):
        assert getattr(_abi, name) == int(re.search(r"^#define %s (\d+)" % name, txt, flags=re.M).group(1)), name
    assert (_abi.GH_XF_WGRAD_ROWS, _abi.GH_XF_WGRAD_CHUNK, _abi.GH_XF_LNP_ROWS) == (P.SLAB, P.WGRAD_CHUNK, P.LNP_ROWS)
    for cls, struct in ((_abi.GhXfStemG, "GhXfStemG"), (_abi.GhXfLayerG, "GhXfLayerG")):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1), flags=re.S)
        assert [f for f, _ in cls._fields_] == re.findall(r"\*\s*(\w+)", body), struct
        assert C.sizeof(cls) == 8 * len(cls._fields_)
    assert [f for f, _ in _abi.GhXfLayerG._fields_] == [f for f, _ in _abi.GhXfLayer._fields_]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct GhXfWgrad \{(.*?)\} GhXfWgrad;", txt, flags=re.S).group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s\*,](\w+)\s*(?=,|$)", decl.strip())]
    assert [f for f, _ in _abi.GhXfWgrad._fields_] == names and C.sizeof(_abi.GhXfWgrad) == 8 * 4 + 11 * 8
    new = ("gh_xf_linear_wgrad_chunk", "gh_xf_linear_wgrad_workspace_bytes", "gh_xf_linear_wgrad", "gh_xf_layernorm_param_grads_workspace_bytes",
           "gh_xf_layernorm_param_grads", "gh_xf_group_norm_param_grads_workspace_bytes", "gh_xf_group_norm_param_grads",
           "gh_xf_backward_params_workspace_bytes", "gh_xf_backward_params")
    assert set(new) <= set(_abi.XF_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert "falls back to torch" not in txt


def test_host_sizes_of_the_parameter_gradients(gh_lib_path):
    """Pure host arithmetic: the chunk is a function of the sizes alone, the workspaces follow it, and the refusals."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    al = lambda n: (n + 255) & ~255

    def chunk(T, K_, n_out):
        tiles, c = -(-n_out // 64) * -(-K_ // 64), 256
        while c < T and tiles * -(-T // c) > 1024:
            c *= 2
        return c

    for T, K_, n_out in [(1, 32, 1), (255, 64, 65), (256, 64, 65), (257, 64, 65), (513, 512, 130), (2048, 512, 512), (2048, 512, 4096),
                         (2048, 2048, 512), (2048, 512, 1536), (16384, 512, 512), (16384, 512, 4096), (1 << 30, 4096, 8192)]:
        c = chunk(T, K_, n_out)
        assert L.gh_xf_linear_wgrad_chunk(T, K_, n_out) == c and c % P.SLAB == 0, (T, K_, n_out)
        n = -(-T // c)
        assert L.gh_xf_linear_wgrad_workspace_bytes(T, K_, n_out) == (0 if n == 1 else al(n * n_out * K_ * 4) + al(n * n_out * 4))
    for s in P.WGRAD_SHAPES:
        assert L.gh_xf_linear_wgrad_chunk(2 * P.WGRAD_CHUNK + 1, *s) == P.WGRAD_CHUNK
    for bad in [(0, 64, 64), (64, 48, 64), (64, 64, 0), (64, 8192, 64), (64, 64, 8193)]:
        assert L.gh_xf_linear_wgrad_chunk(*bad) == 0 and L.gh_xf_linear_wgrad_workspace_bytes(*bad) == 0
    assert L.gh_xf_layernorm_param_grads_workspace_bytes(257, 512) == al(5 * 2 * 512 * 4) and L.gh_xf_layernorm_param_grads_workspace_bytes(0, 512) == 0
    assert L.gh_xf_group_norm_param_grads_workspace_bytes(2, 512, 257, 32) == al(2 * 512 * 2 * 2 * 4)
    ok = _abi.GhXfDims(1, 512, 2048, 32, 8, 64, 10, 1e-6, 1e-5)
    assert L.gh_xf_backward_params_workspace_bytes(C.byref(ok)) > L.gh_xf_backward_workspace_bytes(C.byref(ok)) > 0
    wide = _abi.GhXfDims(1, 512, 2048, 32, 16, 64, 10, 1e-6, 1e-5)            # M = 1024
    assert L.gh_xf_backward_params_workspace_bytes(C.byref(wide)) == 0
    assert L.gh_xf_backward_params(C.byref(wide), None, None, None, None, None, None, None, None, None, None, None, 0, None) == _abi.GH_ERR_UNSUPPORTED
    empty = _abi.GhXfDims(0, 512, 2048, 32, 8, 64, 10, 1e-6, 1e-5)
    assert L.gh_xf_backward_params(C.byref(empty), None, None, None, None, None, None, None, None, None, None, None, 0, None) == _abi.GH_OK
    # bad arguments are refused before any launch: no stream is ever touched here
    a = _abi.GhXfWgrad()
    a.T, a.K, a.N_out = 64, 48, 64
    assert L.gh_xf_linear_wgrad(C.byref(a), None, 0, None) == _abi.GH_ERR_UNSUPPORTED
    a.K, a.prologue = 64, 7
    assert L.gh_xf_linear_wgrad(C.byref(a), None, 0, None) == _abi.GH_ERR_INVALID_ARG
    a.prologue = 0
    assert L.gh_xf_linear_wgrad(C.byref(a), None, 0, None) == _abi.GH_OK                  # nothing wanted: nothing launched
    buf = (C.c_float * 4)()
    a.db = C.addressof(buf)
    assert L.gh_xf_linear_wgrad(C.byref(a), None, 0, None) == _abi.GH_ERR_INVALID_ARG     # no dy
    assert L.gh_xf_layernorm_param_grads(None, 64, None, 64, None, 4, 64, C.addressof(buf), None, None, 0, None) == _abi.GH_ERR_INVALID_ARG
    assert L.gh_xf_group_norm_param_grads(None, None, None, 1, 64, 4, 32, 1e-6, C.addressof(buf), None, None, 0, None) == _abi.GH_ERR_INVALID_ARG
