"""guassianhand_amd.transformer1d without a device: the restatement against a straightforward nn.Module composition, the standalone
module's state-dict keys, the class swap, every fallback condition with its gradients, and the ABI mirror of include/gh_xf.h."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from guassianhand_amd import _abi, _lib
from guassianhand_amd import transformer1d as X
from tests import transformer1d_cases as K
from tests.helpers import header_symbols
from tests.test_cond_cpu import within_twice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("attn2", [True, False])
def test_restatement_is_the_composition(attn2):
    """transformer1d_ref in float32 against StandIn (nn.GroupNorm, nn.LayerNorm, nn.Linear, F.softmax), float64 StandIn as the truth."""
    m = K.make_module(64, 2, 32, 2, attn2=attn2, seed=1)
    x = K.make_x(2, 64, 37, seed=1)
    with torch.no_grad():
        got = X.transformer1d_ref(X.params_of(m), x)
        want = m(x)
        ref = K.make_module(64, 2, 32, 2, attn2=attn2, seed=1, dtype=torch.float64)(x.double())
        ref_r = X.transformer1d_ref(X.params_of(m), x, acc=torch.float64)
    assert got.dtype == torch.float32 and ref_r.dtype == torch.float64
    within_twice("out", got, want, ref)
    within_twice("out f64", ref_r.float(), want, ref)


def test_restatement_with_context_and_masks():
    """encoder_hidden_states and both masks go through the restatement as the composition takes them."""
    m = K.make_module(64, 2, 32, 1, seed=2)
    x, ctx = K.make_x(2, 64, 19, seed=2), K.make_x(2, 11, 64, seed=3)
    mask, emask = (torch.rand(2, 19) > 0.3).float(), (torch.rand(2, 11) > 0.3).float()
    with torch.no_grad():
        got = X.transformer1d_ref(X.params_of(m), x, encoder_hidden_states=ctx, attention_mask=mask, encoder_attention_mask=emask)
        want = m(x, encoder_hidden_states=ctx, attention_mask=mask, encoder_attention_mask=emask)
        ref = m.double()(x.double(), encoder_hidden_states=ctx.double(), attention_mask=mask.double(), encoder_attention_mask=emask.double())
    within_twice("out", got, want, ref)


def test_state_dict_keys_are_the_hand_written_list(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "transformer1d_keys.json")))
    assert "NOT recorded" in doc["note"]
    m = X.Transformer1D(**doc["config"])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == doc["keys"]
    # attn2 follows cross_attention_dim, as in the reference
    cfg = dict(doc["config"], cross_attention_dim=None)
    keys = list(X.Transformer1D(**cfg).state_dict())
    assert not any("attn2" in k or "norm2" in k for k in keys) and len(keys) == len(doc["keys"]) - 7
    # the composition of the tests carries the same keys, so a state dict moves between the two
    s = K.make_module(64, 2, 32, 1, seed=3)
    assert list(s.state_dict()) == [k for k, _ in doc["keys"]]
    m.load_state_dict(s.state_dict())
    x = K.make_x(1, 64, 9)
    with torch.no_grad():
        assert torch.equal(m(x), X.transformer1d_ref(X.params_of(s), x))


def test_fuse_keeps_parameters_and_is_idempotent():
    m = K.make_module(64, 2, 32, 1, seed=4)
    before = {k: (id(v), v.data_ptr()) for k, v in m.named_parameters()}
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    mods = [id(t) for t in m.modules()]
    x = K.make_x(2, 64, 13)
    with torch.no_grad():
        want = m(x)
    f = X.fuse_transformer1d(m)
    cls = type(f)
    assert f is m and isinstance(m, K.StandIn) and cls is not K.StandIn and cls.__name__ == "StandIn" and cls is X.fused_transformer1d_cls(K.StandIn)
    assert X.fuse_transformer1d(m) is m and type(m) is cls
    assert {k: (id(v), v.data_ptr()) for k, v in m.named_parameters()} == before and [id(t) for t in m.modules()] == mods
    assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    n = K.StandIn.calls
    with torch.no_grad():
        got = m(x)                                              # a CPU tensor: the base class's own forward
    assert K.StandIn.calls == n + 1 and torch.equal(got, want)


def test_fused_forward_ignores_what_layer_norm_blocks_ignore(monkeypatch):
    """TGS._forward passes modulation_cond to both backbones on every call. With plain LayerNorm blocks the base class does not read
    it (nor timestep, nor class_labels), so it must not keep the call from the kernels: the decision is kernel_reason's alone, and a
    non-empty cross_attention_kwargs still goes to the base class."""
    m = X.fuse_transformer1d(K.make_module(64, 2, 32, 1, seed=7))
    x, cond = K.make_x(2, 64, 13), torch.randn(2, 8)
    asked, ran = [], []
    monkeypatch.setattr(X, "kernel_reason", lambda mod, t, **kw: asked.append(kw) or None)
    monkeypatch.setattr(X, "_run", lambda packed, t: ran.append(packed) or t)
    n = K.StandIn.calls
    with torch.no_grad():
        out = m(x, modulation_cond=cond)                         # as infer_one_shot.py:256-264 calls it
        m(x, timestep=torch.zeros(2, dtype=torch.long), class_labels=torch.zeros(2, dtype=torch.long), modulation_cond=cond)
    assert len(asked) == 2 and len(ran) == 2 and out is x and K.StandIn.calls == n
    assert all(v is None for kw in asked for v in kw.values())
    with torch.no_grad():
        m(x, modulation_cond=cond, cross_attention_kwargs={"scale": 0.5})
    assert len(asked) == 2 and len(ran) == 2 and K.StandIn.calls == n + 1


def test_fused_module_pickles_to_its_own_class():
    import pickle
    m = X.fuse_transformer1d(K.make_module(64, 2, 32, 1, seed=8))
    back = pickle.loads(pickle.dumps(m))
    assert type(back) is type(m) and isinstance(back, K.StandIn) and not isinstance(back, X.Transformer1D)
    assert list(back.state_dict()) == list(m.state_dict()) and all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), m.state_dict().values()))
    x = K.make_x(1, 64, 9)
    with torch.no_grad():
        assert torch.equal(back(x), m(x))


def _grads(out, tensors):
    out.square().sum().backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in tensors)


@pytest.mark.parametrize("how", ["cpu", "float64", "trainable", "mask", "ops_torch"])
def test_fallbacks_take_the_torch_path_and_keep_every_gradient(how):
    dtype = torch.float64 if how == "float64" else torch.float32
    m = K.make_module(64, 2, 32, 1, seed=5, dtype=dtype)
    x = K.make_x(2, 64, 13, dtype=dtype).requires_grad_(True)
    kw = {}
    if how == "mask":
        kw["attention_mask"] = (torch.rand(2, 13) > 0.2).to(dtype)
    if how == "ops_torch":
        kw["ops"] = "torch"
    assert how == "ops_torch" or X.kernel_reason(m, x, **kw) is not None
    if how == "trainable":
        assert X.kernel_reason(m, x.detach()) is not None        # x needs none, a parameter does
    out = X.transformer1d(m, x, **kw)
    assert out.dtype == dtype and out.requires_grad
    want = m(x, **{k: v for k, v in kw.items() if k != "ops"})
    assert float((out - want).detach().abs().max()) <= 1e-4 * float(want.detach().abs().max())
    _grads(out, [x, *m.parameters()])
    # the same through the params form, the standalone module and the swapped class
    p = X.params_of(m)
    assert torch.equal(X.transformer1d(p, x, **kw), out)
    s = X.Transformer1D(64, 2, 32, 1, cross_attention_dim=64).to(dtype)
    s.load_state_dict(m.state_dict())
    assert torch.equal(s(x, **kw), out)
    n = K.StandIn.calls
    f = X.fuse_transformer1d(m)
    o2 = f(x, **{k: v for k, v in kw.items() if k != "ops"})
    assert K.StandIn.calls == n + 1 and o2.requires_grad


def test_structure_conditions_are_named():
    """Each structural condition of the issue turns the kernel path off by itself (checked on CPU through the module's reason)."""
    mk = lambda: K.make_module(64, 2, 32, 1, seed=6)
    assert X._module_reason(mk()) is None
    m = mk(); m.transformer_blocks[0].only_cross_attention = True
    assert X._module_reason(m)
    m = mk(); m.transformer_blocks[0].fuser = torch.nn.Identity()
    assert X._module_reason(m)
    m = mk(); m.transformer_blocks[0]._chunk_size = 4
    assert X._module_reason(m)
    m = mk(); m.transformer_blocks[0].norm1 = torch.nn.LayerNorm(64, elementwise_affine=False)
    assert X._module_reason(m)
    m = mk(); m.transformer_blocks[0].ff.net[0] = torch.nn.Linear(64, 256)
    assert X._module_reason(m)
    m = mk(); m.transformer_blocks[0].ff.net[1] = torch.nn.Dropout(0.1); m.train()
    assert X._module_reason(m)
    m.eval()
    assert X._module_reason(m) is None
    m = mk(); m.transformer_blocks[0].attn1.to_q = torch.nn.Linear(64, 64, bias=True)
    p = X.params_of(m)
    assert p["blocks"][0]["attn1"]["q_b"] is not None             # attention_bias: refused by the parameter check
    assert not X.sizes_supported(64, 32, 2, 48) and not X.sizes_supported(64, 32, 33, 32) and not X.sizes_supported(48, 16, 2, 32)
    assert X.sizes_supported(512, 32, 8, 64) and X.sizes_supported(1024, 32, 16, 64) and not X.sizes_supported(1056, 32, 8, 64)


def test_bad_ops_is_a_value_error():
    m = K.make_module(64, 2, 32, 1)
    with pytest.raises(ValueError):
        X.transformer1d(m, K.make_x(1, 64, 5), ops="hip")


def test_config_seam_is_lazy():
    import importlib
    mod = importlib.import_module("guassianhand_amd.tgs_backbone")     # importing it needs no reference checkout
    with pytest.raises(AttributeError):
        mod.NoSuchClass


def test_abi_mirror_matches_the_header():
    assert sorted(_abi.XF_SYMBOLS) == header_symbols("gh_xf.h") and set(_abi.XF_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    assert any(s.endswith("gh_xf.hip") for s in _lib.SOURCES) and any(h.endswith("gh_xf.h") for h in _lib.HEADERS)
    txt = open(os.path.join(ROOT, "include", "gh_xf.h")).read()
    for name, value in re.findall(r"^#define (GH_XF_\w+) (\d+|\(1 << \d+\))", txt, flags=re.M):
        assert getattr(_abi, name) == eval(value), name
    for cls, struct in ((_abi.GhXfStem, "GhXfStem"), (_abi.GhXfLayer, "GhXfLayer")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert [f for f, _ in cls._fields_] == re.findall(r"\*\s*(\w+)", body), struct
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct GhXfLinear \{(.*?)\} GhXfLinear;", txt, flags=re.S).group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s\*,](\w+)\s*(?=,|$)", decl.strip())]
    assert [f for f, _ in _abi.GhXfLinear._fields_] == names
    assert C.sizeof(_abi.GhXfLinear) == 8 * 4 + 14 * 8 and C.sizeof(_abi.GhXfDims) == 9 * 4


def test_library_exports_the_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.XF_SYMBOLS:
        getattr(L, sym)
    # pure host arithmetic: sizes and refusals need no device
    L.gh_xf_workspace_bytes.restype = C.c_size_t
    L.gh_xf_workspace_bytes.argtypes = [C.POINTER(_abi.GhXfDims)]
    ok = _abi.GhXfDims(1, 512, 2048, 32, 8, 64, 10, 1e-6, 1e-5)
    T, M = 2048, 512
    al = lambda n: (n + 255) & ~255
    assert L.gh_xf_workspace_bytes(C.byref(ok)) == al(T * M * 4) * 2 + al(T * 3 * M * 4) + al(T * 4 * M * 4) + al(T * 8) + al(32 * 8) + al(32 * 8 * 8)
    for bad in (_abi.GhXfDims(1, 512, 2048, 32, 8, 48, 10, 1e-6, 1e-5), _abi.GhXfDims(1, 512, 2048, 32, 33, 32, 10, 1e-6, 1e-5),
                _abi.GhXfDims(0, 512, 2048, 32, 8, 64, 10, 1e-6, 1e-5)):
        assert L.gh_xf_workspace_bytes(C.byref(bad)) == 0
    L.gh_xf_forward.restype = C.c_int
    L.gh_xf_forward.argtypes = [C.POINTER(_abi.GhXfDims)] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    for bad in (_abi.GhXfDims(1, 512, 2048, 32, 8, 48, 10, 1e-6, 1e-5), _abi.GhXfDims(1, 512, 2048, 32, 33, 32, 10, 1e-6, 1e-5)):
        assert L.gh_xf_forward(C.byref(bad), None, None, None, None, None, 0, None) == _abi.GH_ERR_UNSUPPORTED
