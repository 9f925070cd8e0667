"""The texture scene code on the host (guassianhand_amd/scene_code.py): its plain-torch restatement and its standalone module against
outputs and gradients CAPTURED from the reference's own detokenize and TriplaneUpsampleNetwork (tests/golden/
make_scene_code_fixture.py -> scene_code_fixture.npz; exact grids, so every comparison is bit for bit), the fallbacks, the module's
state-dict keys, the C-ABI's symbols, limits and host-side argument checks, and the opt-in class name. No GPU compute is launched."""
import ctypes as C
import importlib
import sys
import types

import pytest
import torch

from guassianhand_amd import _abi, _lib
from guassianhand_amd import scene_code as SC
from tests.helpers import header_symbols
from tests.scene_code_cases import PlainUpsample, load_fixture, make_inputs, make_module, run, to_planes


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_fixture(golden_dir)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("mode", ["kernel", "torch32", "f64"])
def test_restatement_reproduces_the_reference_bit_for_bit(cases, tag, mode):
    """scene_code on CPU tensors ('kernel' here: the public call), scene_code_ref, and scene_code_ref in float64."""
    c = cases[0][tag]
    out, da, db, dpb = run(mode, c.module, c.a, c.b, c.pb, c.cot)
    assert out.dtype == (torch.float64 if mode == "f64" else torch.float32) and out.shape == c.out.shape
    assert torch.equal(out.float(), c.out)
    assert torch.equal(da.float(), c.d_tokens) and torch.equal(db.float(), c.d_tokens)
    assert dpb.shape == c.pb.shape and torch.equal(dpb.float(), c.d_plane_bias)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_standalone_module_reproduces_the_reference_bit_for_bit(cases, tag):
    """The module's forward on detokenize's view, with the three statements around it written out."""
    c = cases[0][tag]
    B, Ci, Co, Np, S = c.dims
    a, b, pb = (t.clone().requires_grad_(True) for t in (c.a, c.b, c.pb))
    planes = (a + b).view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4)
    up = c.module(planes)
    assert up.shape == (B, Np, Co, 2 * S, 2 * S)
    out = torch.cat([up[:, 0], up[:, 1]], dim=-1).unsqueeze(1)
    out = out + torch.cat([pb[..., :2 * S], pb[..., :2 * S]], dim=-1)
    (out * c.cot).sum().backward()
    assert torch.equal(out, c.out) and torch.equal(a.grad, c.d_tokens) and torch.equal(b.grad, c.d_tokens)
    assert torch.equal(pb.grad, c.d_plane_bias)
    assert torch.equal(to_planes(c.out - torch.cat([c.pb[..., :2 * S]] * Np, dim=-1), Np), up.detach())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_a_pair_of_tokens_equals_their_sum(cases, tag):
    c = cases[0][tag]
    pair = run("torch32", c.module, c.a, c.b, c.pb, c.cot)
    one = run("torch32", c.module, c.a + c.b, None, c.pb, c.cot)
    assert torch.equal(pair[0], one[0]) and torch.equal(pair[1], one[1]) and torch.equal(pair[3], one[3])
    single = SC.scene_code(c.module, [c.a + c.b], c.pb)                                     # a sequence of one is one tensor
    assert torch.equal(single, one[0])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_plane_bias_gradient_has_the_parameters_shape_and_zeros_beyond_2s(cases, tag):
    c = cases[0][tag]
    S = c.dims[4]
    dpb = run("kernel", c.module, c.a, c.b, c.pb, c.cot, need_tok=False)[3]
    assert dpb.shape == c.pb.shape == (c.dims[2], 2 * S, 4 * S)
    assert float(dpb[..., 2 * S:].abs().max()) == 0.0 and float(dpb[..., :2 * S].abs().max()) > 0.0
    assert float(c.d_plane_bias[..., 2 * S:].abs().max()) == 0.0


def test_standalone_module_carries_the_references_keys_and_shapes(cases):
    fx = cases[1]
    keys, shapes = [str(k) for k in fx["init_keys"]], [tuple(int(v) for v in row if v) for row in fx["init_shapes"]]
    assert keys == ["upsample.weight", "upsample.bias"]
    m = SC.TriplaneUpsampleNetwork(512, 80, 2)
    sd = m.state_dict()
    assert list(sd.keys()) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    assert (m.cfg.in_channels, m.cfg.out_channels, m.cfg.n_plane) == (512, 80, 2)
    other = SC.TriplaneUpsampleNetwork(512, 80, 2)
    other.load_state_dict({k: torch.full(s, 0.25) for k, s in zip(keys, shapes)})           # strict
    assert float(other.upsample.weight.detach().min()) == 0.25
    # nn.ConvTranspose2d's default initialisation: uniform within +-1/sqrt(fan_in), fan_in = Co * 2 * 2 for a transposed weight
    lim = 1.0 / (80 * 4) ** 0.5
    top = float(m.upsample.weight.detach().abs().max())
    assert 0.9 * lim < top <= lim
    d = SC.TriplaneUpsampleNetwork()
    assert (d.cfg.in_channels, d.cfg.out_channels, d.cfg.n_plane) == (1024, 80, 1)


def _grads(module, fn, a, b, pb, cot):
    for p in module.parameters():
        p.grad = None
    la, lb, lpb = (t.detach().clone().requires_grad_(True) for t in (a, b, pb))
    out = fn(module, (la, lb), lpb)
    (out * cot.to(out.dtype)).sum().backward()
    return [out.detach(), la.grad, lb.grad, lpb.grad] + [p.grad for p in module.parameters()]


def _same(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y)


def test_fallbacks_return_the_restatement_and_all_its_gradients():
    dims = (2, 6, 5, 2, 3)
    a, b, pb, cot = make_inputs(dims)
    ref = lambda m, tok, bias: SC.scene_code_ref(m, tok, bias)
    trainable = make_module(dims, frozen=False)
    want = _grads(trainable, ref, a, b, pb, cot)
    assert want[4] is not None and want[5] is not None and want[4].shape == (6, 5, 2, 2)    # weight and bias get gradients
    _same(_grads(trainable, lambda m, tok, bias: SC.scene_code(m, tok, bias), a, b, pb, cot), want)          # CPU tensors, trainable
    _same(_grads(trainable, lambda m, tok, bias: SC.scene_code(m, tok, bias, ops="torch"), a, b, pb, cot), want)
    frozen = make_module(dims)
    _same(_grads(frozen, lambda m, tok, bias: SC.scene_code(m, tok, bias), a, b, pb, cot), _grads(frozen, ref, a, b, pb, cot))
    # float64 throughout
    m64 = make_module(dims, frozen=False).double()
    a64, b64, pb64 = a.double(), b.double(), pb.double()
    got = _grads(m64, lambda m, tok, bias: SC.scene_code(m, tok, bias), a64, b64, pb64, cot)
    assert got[0].dtype == torch.float64
    _same(got, _grads(m64, ref, a64, b64, pb64, cot))
    # a 3 x 3 kernel: planes of 2S + 1, and a plane bias of that height
    B, Ci, Co, Np, S = dims
    torch.manual_seed(5)
    m3 = PlainUpsample(Ci, Co, Np, kernel_size=3, stride=2)
    w = 2 * S + 1
    pb3, cot3 = torch.randn(Co, w, w + 2), torch.randn(B, 1, Co, w, Np * w)
    got = _grads(m3, lambda m, tok, bias: SC.scene_code(m, tok, bias), a, b, pb3, cot3)
    assert got[0].shape == (B, 1, Co, w, Np * w) and float(got[3][..., w:].abs().max()) == 0.0
    _same(got, _grads(m3, ref, a, b, pb3, cot3))
    assert SC.upsample_forward(m3, torch.randn(B, Np, Ci, S, S)) is None
    with pytest.raises(ValueError):
        SC.scene_code(frozen, a, pb, ops="hip")
    with pytest.raises(ValueError):
        SC.scene_code(frozen, a[..., :-1], pb)                                              # 17 tokens are not two square planes


def test_grafted_class_on_cpu_calls_the_base_forward():
    cls = SC.fused_upsample_cls(PlainUpsample)
    assert cls is SC.fused_upsample_cls(PlainUpsample) and issubclass(cls, PlainUpsample) and cls.__name__ == "PlainUpsample"
    torch.manual_seed(3)
    m = cls(6, 5, 2)
    planes = torch.randn(2, 2, 6, 3, 3)
    got = m(planes)
    assert m.calls == 1 and torch.equal(got, PlainUpsample.forward(m, planes))
    assert torch.equal(got, SC.upsample_ref(m, planes))


# ---- C-ABI (include/gh_scene.h) -----------------------------------------------------------------------------------------------------
def test_library_exports_the_scene_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.SCENE_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_scene(L)
    assert sorted(_abi.SCENE_SYMBOLS) == header_symbols("gh_scene.h")
    assert set(_abi.SCENE_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    hdr = open(gh_lib_path.replace("guassianhand_amd/libgh_raster.so", "include/gh_scene.h")).read()
    for name in ("GH_SCENE_PER_PLANE", "GH_SCENE_MAX_CI", "GH_SCENE_MAX_CO", "GH_SCENE_MAX_TILES"):
        assert f"#define {name} {getattr(_abi, name)} " in hdr or f"#define {name} {getattr(_abi, name)}\n" in hdr, name
    assert (SC.MAX_CI, SC.MAX_CO) == (1024, 128)
    assert any(s.endswith("gh_scene.hip") for s in _lib.SOURCES) and any(h.endswith("gh_scene.h") for h in _lib.HEADERS)
    assert C.sizeof(_abi.GhSceneDims) == 24


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes in the order include/gh_scene.h states them (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_scene(L)
    one, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2)
    bad, uns, ok = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED, _abi.GH_OK
    PP = _abi.GH_SCENE_PER_PLANE

    def fwd(dims=(1, 512, 80, 2, 32, 0), a=one, b=one, w=one, cb=one, pb=one, out=one):
        d = _abi.GhSceneDims(*dims)
        return L.gh_scene_code_forward(C.byref(d), a, 2048 * 512, 2048, b, 2048 * 512, 2048, w, cb, pb, 64 * 128, 128, out, None)

    assert fwd((1, 1025, 80, 2, 32, 0)) == fwd((1, 512, 129, 2, 32, 0)) == uns
    assert fwd((1, 512, 80, 2, 0, 0)) == fwd((-1, 512, 80, 2, 32, 0)) == fwd((1, 0, 80, 2, 32, 0)) == fwd((1, 512, 0, 2, 32, 0)) == bad
    assert fwd((1, 512, 80, 0, 32, 0)) == fwd((1, 512, 80, 2, 32, 2)) == bad
    assert fwd((1, 512, 80, 1, 1 << 30, 0)) == fwd(((1 << 31) - 1, 512, 80, 2, 1 << 12, 0)) == uns           # more tiles than one launch holds
    assert fwd((-1, 1025, 80, 2, 32, 0)) == bad                                              # nonsense is judged before size
    assert fwd(a=None) == fwd(w=None) == fwd(out=None) == bad
    assert fwd(a=odd) == fwd(b=odd) == fwd(w=odd) == fwd(cb=odd) == fwd(pb=odd) == fwd(out=odd) == bad
    assert fwd((1, 512, 80, 2, 32, PP)) == bad                                               # a plane bias with the per-plane form
    assert L.gh_scene_code_forward(None, one, 1, 1, one, 1, 1, one, one, one, 1, 1, one, None) == bad
    assert fwd((0, 512, 80, 2, 32, 0)) == fwd((0, 512, 80, 2, 32, PP), pb=None) == fwd((0, 1, 1, 1, 1, 0), b=None, cb=None, pb=None) == ok
    assert fwd((0, 1025, 80, 2, 32, 0)) == uns and fwd((0, 512, 80, 2, 32, 0), out=None) == bad   # judged before the empty batch

    def bwd(dims=(1, 512, 80, 2, 32, 0), w=one, g=one, d_tok=one, d_pb=one):
        d = _abi.GhSceneDims(*dims)
        return L.gh_scene_code_backward(C.byref(d), w, g, d_tok, d_pb, 64 * 128, 128, None)

    assert bwd((1, 1025, 80, 2, 32, 0)) == bwd((1, 512, 129, 2, 32, 0)) == uns
    assert bwd((1, 512, 80, 2, 0, 0)) == bwd((-1, 512, 80, 2, 32, 0)) == bad
    assert bwd(w=None) == bwd(g=None) == bwd(w=odd) == bwd(g=odd) == bwd(d_tok=odd) == bwd(d_pb=odd) == bad
    assert bwd((1, 512, 80, 2, 32, PP)) == bad
    assert bwd(d_tok=None, d_pb=None) == bwd((1, 512, 80, 2, 32, PP), d_tok=None, d_pb=None) == ok   # nothing asked for
    assert bwd((0, 512, 80, 2, 32, 0)) == ok
    assert L.gh_scene_code_backward(None, one, one, one, one, 1, 1, None) == bad


# ---- the opt-in class name ------------------------------------------------------------------------------------------------------------
def test_tgs_scene_resolves_its_one_name_lazily(monkeypatch):
    for n in [n for n in sys.modules if n.split(".")[0] in ("tgs", "diffusers")]:
        monkeypatch.delitem(sys.modules, n)
    import guassianhand_amd.tgs_scene as T
    T = importlib.reload(T)
    assert "tgs" not in sys.modules and "diffusers" not in sys.modules                       # importing it reaches for neither
    with pytest.raises(AttributeError):
        T.TriplaneUpsampleNetworkFused
    with pytest.raises(AttributeError):
        T.LocalPoolPointnet
    names = ("tgs", "tgs.models", "tgs.models.networks_texture")
    for n in names:
        monkeypatch.setitem(sys.modules, n, types.ModuleType(n))
    sys.modules[names[-1]].TriplaneUpsampleNetwork = PlainUpsample
    monkeypatch.setattr(T, "_cache", {})
    cls = T.TriplaneUpsampleNetwork
    assert cls is T.TriplaneUpsampleNetwork is SC.fused_upsample_cls(PlainUpsample) and issubclass(cls, PlainUpsample)
    assert "diffusers" not in sys.modules
