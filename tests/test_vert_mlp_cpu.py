"""The vertex MLP block on the host (guassianhand_amd/vert_mlp.py): its plain-torch restatement against outputs and gradients CAPTURED
from the reference's own vert_valid and vert_pos_refinement (tests/golden/make_vert_mlp_fixture.py -> vert_mlp_fixture.npz), the
modules' state-dict keys and initialisation, the C-ABI's symbols and host-side argument checks, the train-mode fallback and the
opt-in renderer names. No GPU compute is launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import vert_mlp as V
from tests.helpers import header_symbols

KEYS = {"ln_weight": "ff.layer_norm.weight", "ln_bias": "ff.layer_norm.bias", "fc1_weight": "ff.fc1.weight", "fc1_bias": "ff.fc1.bias",
        "fc2_weight": "ff.fc2.weight", "fc2_bias": "ff.fc2.bias", "fc_weight": "fc.weight", "fc_bias": "fc.bias"}
ACT = {"v": "sigmoid", "r": "tanh_offset"}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vert_mlp_fixture.npz"), allow_pickle=False)


def fixture_case(fx, tag):
    """(x, pts, params in V.PARAMS order, cotangent) of module `tag` ('v' gate, 'r' refinement)."""
    xs, ws, cs = (float(v) for v in fx["scales"])
    x, pts = torch.tensor(fx["x_q"]).float() * xs, torch.tensor(fx["pts"])
    params = [torch.tensor(fx[f"{tag}_{k}_q"]).float() * ws if f"{tag}_{k}_q" in fx.files else torch.tensor(fx[f"{tag}_{k}"]) for k in V.PARAMS]
    return x, pts, params, torch.tensor(fx[f"{tag}_cot_q"]).float() * cs


def test_params_order_is_the_abi_structs():
    assert V.PARAMS == tuple(KEYS) == tuple(n for n, _ in _abi.GhVertParams._fields_) == tuple(n for n, _ in _abi.GhVertGrads._fields_)


@pytest.mark.parametrize("tag", ["v", "r"])
def test_restatement_reproduces_the_reference_modules(fx, tag):
    """vert_block on CPU tensors (F.layer_norm and F.linear over torch.cat) against the reference's modules in eval(): every output
    and every gradient of the recorded cotangent within twice the reference's own float32 error against the float64 restatement,
    plus 2^-22 of the largest float64 value."""
    x, pts, params, cot = fixture_case(fx, tag)
    kw = dict(act=ACT[tag], radius=float(fx["radius"]))
    leaves = [v.clone().requires_grad_(True) for v in [x, pts] + params]
    out = V.vert_block(leaves[0], leaves[1], leaves[2:], **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == fx[f"{tag}_out"].shape
    (out * cot).sum().backward()
    l64 = [v.detach().clone().requires_grad_(True) for v in [x, pts] + params]
    out64 = V._vert_block_ref(l64[0], l64[1], l64[2:], **kw, acc=torch.float64)
    assert out64.dtype == torch.float64
    (out64 * cot.double()).sum().backward()
    rows = [("out", out.detach(), fx[f"{tag}_out"], out64.detach()),
            ("grad_x", leaves[0].grad[::8], fx[f"{tag}_grad_x8"], l64[0].grad[::8]),
            ("grad_pts", leaves[1].grad, fx[f"{tag}_grad_pts"], l64[1].grad)]
    rows += [(f"grad_{k}", leaves[2 + i].grad, fx[f"{tag}_grad_{k}"], l64[2 + i].grad) for i, k in enumerate(V.PARAMS)]
    bad = []
    for name, got, want, ref in rows:
        want = torch.tensor(want)
        assert got.shape == want.shape == ref.shape, name
        e_ref = float((want.double() - ref).abs().max())              # the reference's own float32 error
        e_got = float((got.double() - ref).abs().max())
        floor = 2.0 ** -22 * float(ref.abs().max())
        print(f"{tag} {name:16s} got-f64 {e_got:.3e}  reference-f64 {e_ref:.3e}  max|f64| {float(ref.abs().max()):.3e}")
        if not e_got <= 2 * e_ref + floor:
            bad.append((name, e_got, e_ref, floor))
    assert not bad, bad


def test_selected_rows_equal_the_fixtures(fx):
    """The rows above 0.1 and above 0.9 of the restatement's scores are the reference's, and the fixture keeps its promises: at least 8
    rows in each band and none within 1e-3 of a threshold."""
    x, pts, params, _ = fixture_case(fx, "v")
    got = V.vert_block(x, pts, params)[:, 0].numpy()
    want = fx["v_out"][:, 0]
    for t in (0.1, 0.9):
        assert np.array_equal(np.nonzero(got > t)[0], np.nonzero(want > t)[0]), t
    assert min((want < 0.1).sum(), ((want > 0.1) & (want < 0.9)).sum(), (want > 0.9).sum()) >= 8
    assert float(np.minimum(np.abs(want - 0.1), np.abs(want - 0.9)).min()) >= 1e-3


@pytest.mark.parametrize("tag,cls,K", [("v", V.VertValid, 1), ("r", V.VertPosRefinement, 3)])
def test_modules_carry_the_reference_state_dict_and_initialisation(fx, tag, cls, K):
    keys = sorted(k[len(f"init_{tag}."):] for k in fx.files if k.startswith(f"init_{tag}."))
    torch.manual_seed(3)
    m = cls(131)
    sd = m.state_dict()
    assert sorted(sd.keys()) == keys == sorted(KEYS.values())
    for k in keys:
        assert tuple(sd[k].shape) == tuple(int(n) for n in fx[f"init_{tag}.{k}"]), k
    assert tuple(sd["fc.weight"].shape) == (K, 33) and tuple(sd["ff.fc1.weight"].shape) == (33, 134)
    for name in ("ff.fc1", "ff.fc2", "fc"):                        # Xavier-uniform weights, zero biases
        w = sd[f"{name}.weight"]
        bound = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound, name
        assert float(sd[f"{name}.bias"].abs().max()) == 0.0, name
    assert torch.equal(sd["ff.layer_norm.weight"], torch.ones(134)) and torch.equal(sd["ff.layer_norm.bias"], torch.zeros(134))
    assert m.ff.layer_norm.eps == 1e-6 and m.ff.dropout1.p == 0.1 and m.ff.dropout2.p == 0.1
    # the fixture's parameters load under the reference's keys, and the eval-mode forward is vert_block over them
    x, pts, params, _ = fixture_case(fx, tag)
    m.load_state_dict({KEYS[k]: p for k, p in zip(V.PARAMS, params)}, strict=True)
    m.eval()
    want = V.vert_block(x, pts, params, act=ACT[tag], radius=0.001)
    assert torch.equal(m(x, pts), want)
    assert torch.equal(m(x.reshape(4, 16, 131), pts.reshape(4, 16, 3)), want.reshape(4, 16, K))   # leading dimensions pass through
    # if_detach: no gradient reaches the inputs
    d = cls(131, if_detach=True).eval()
    xg, pg = x.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    d(xg, pg).sum().backward()
    assert xg.grad is None and pg.grad is None and d.fc.weight.grad is not None


def test_refinement_position_term_carries_no_gradient(fx):
    x, pts, params, _ = fixture_case(fx, "r")
    p = pts.clone().requires_grad_(True)
    out = V.vert_block(x, p, params, act="tanh_offset", radius=0.001)
    out.sum().backward()
    # |tanh| <= 1, and the sum and the difference round at positions below 0.25 (half an ulp there is 1.5e-8 each)
    assert float((out.detach() - pts).abs().max()) <= 0.001 + 1e-7
    assert float(p.grad.abs().max()) < 0.1                         # (an identity term would add 1)


def test_library_exports_the_vert_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.VERT_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_vert(L)
    assert sorted(_abi.VERT_SYMBOLS) == header_symbols("gh_vert.h")
    per_tile = 2 * 134 + 33 * 134 + 33 + 33 * 33 + 33 + 3 * 33 + 3
    assert L.gh_vert_workspace_bytes(98562, 134, 33, 3) >= 4 * -(-98562 // _abi.GH_VERT_ROWS) * per_tile
    assert L.gh_vert_workspace_bytes(1, 4, 1, 1) > 0 and L.gh_vert_workspace_bytes(1, 259, 64, 3) > 0
    for P, D, Hd, K in ((0, 134, 33, 1), (-1, 134, 33, 1), (10, 3, 0, 1), (10, 260, 65, 1), (10, 134, 34, 1), (10, 134, 33, 2), (10, 134, 33, 0)):
        assert L.gh_vert_workspace_bytes(P, D, Hd, K) == 0, (P, D, Hd, K)


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for bad sizes, descriptors, null pointers and a short workspace (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_vert(L)
    one = C.c_void_p(1 << 20)
    params = _abi.GhVertParams(*[1 << 20] * 8)
    gate, refine = _abi.GhVertDesc(1, _abi.GH_VERT_ACT_SIGMOID, 0.0, 1e-6), _abi.GhVertDesc(3, _abi.GH_VERT_ACT_TANH_OFFSET, 0.001, 1e-6)
    bad = _abi.GH_ERR_INVALID_ARG

    def fwd(d=gate, P=10, Cf=131, stride=131, x=one, pts=one, p=params, out=one):
        return L.gh_vert_forward(x, stride, pts, P, Cf, C.byref(p) if p else None, C.byref(d) if d else None, out, None)

    assert fwd(Cf=0) == fwd(Cf=257) == fwd(Cf=-1) == bad
    assert fwd(_abi.GhVertDesc(2, 0, 0.0, 1e-6)) == fwd(_abi.GhVertDesc(0, 0, 0.0, 1e-6)) == bad                  # K
    assert fwd(_abi.GhVertDesc(1, 2, 0.0, 1e-6)) == fwd(_abi.GhVertDesc(1, _abi.GH_VERT_ACT_TANH_OFFSET, 0.001, 1e-6)) == bad
    assert fwd(_abi.GhVertDesc(1, 0, 0.0, -1.0)) == fwd(_abi.GhVertDesc(1, 0, 0.0, float("nan"))) == bad          # eps
    assert fwd(None) == fwd(p=None) == fwd(x=None) == fwd(pts=None) == fwd(out=None) == fwd(stride=130) == fwd(P=-1) == bad
    for i in range(8):
        holes = [1 << 20] * 8
        holes[i] = None
        assert fwd(p=_abi.GhVertParams(*holes)) == bad, i
    assert fwd(P=0) == fwd(refine, P=0) == _abi.GH_OK                                        # no rows: nothing to launch

    def bwd(d=refine, P=10, Cf=131, x=one, gx=one, gxs=131, grads=None, ws=None, nbytes=0):
        return L.gh_vert_backward(x, 131, one, P, Cf, C.byref(params), C.byref(d), one, gx, gxs, one, C.byref(grads) if grads else None,
                                  ws, nbytes, None)

    full = _abi.GhVertGrads(*[1 << 20] * 8)
    assert bwd(Cf=0) == bwd(Cf=257) == bwd(x=None) == bwd(gx=None) == bwd(gxs=130) == bad
    assert bwd(_abi.GhVertDesc(2, 0, 0.0, 1e-6)) == bad
    assert bwd(grads=_abi.GhVertGrads(*([1 << 20] * 7 + [None])), ws=one, nbytes=1 << 30) == bad
    assert bwd(grads=full, ws=None, nbytes=1 << 30) == bwd(grads=full, ws=C.c_void_p((1 << 20) + 4), nbytes=1 << 30) == bad
    assert bwd(grads=full, ws=one, nbytes=16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert bwd(P=0) == bwd(P=0, grads=full) == _abi.GH_OK


def test_python_refuses_bad_arguments_on_the_host():
    x, pts = torch.zeros(6, 5), torch.zeros(6, 3)
    params = [torch.zeros(s) for s in V.param_shapes(5, 1)]
    V.vert_block(x, pts, params)
    with pytest.raises(TypeError, match="float32"):
        V.vert_block(x.double(), pts, params)
    with pytest.raises(ValueError, match="1 to 256"):
        V.vert_block(torch.zeros(6, 257), pts, [torch.zeros(s) for s in V.param_shapes(257, 1)])
    with pytest.raises(ValueError, match="1 to 256"):
        V.vert_block(torch.zeros(6, 0), pts, params)
    with pytest.raises(ValueError, match="K must be 1 or 3"):
        V.vert_block(x, pts, [torch.zeros(s) for s in V.param_shapes(5, 2)])
    with pytest.raises(ValueError, match="K must be 3"):
        V.vert_block(x, pts, params, act="tanh_offset")
    with pytest.raises(ValueError, match="ln_weight: expected"):
        V.vert_block(x, pts, [torch.zeros(s) for s in V.param_shapes(9, 1)])
    with pytest.raises(ValueError, match="pts"):
        V.vert_block(x, pts[:5], params)
    with pytest.raises(ValueError, match="params"):
        V.vert_block(x, pts, params[:7])
    with pytest.raises(ValueError, match="act"):
        V.vert_block(x, pts, params, act="relu")
    with pytest.raises(ValueError, match="ops"):
        V.vert_block(x, pts, params, ops="eager")
    assert tuple(V.vert_block(x[:0], pts[:0], params).shape) == (0, 1)


class _Theirs(torch.nn.Module):
    """Someone else's vert_valid-shaped module whose forward counts its calls."""

    def __init__(self, K):
        super().__init__()
        self.verts_f_dim, self.detach, self.radius, self.calls = 5, False, 0.001, 0
        self.ff = V._MLPBlock(8, 2)
        self.fc = torch.nn.Linear(2, K)

    def forward(self, verts_f, verts_position):
        self.calls += 1
        return torch.full((verts_f.shape[0], self.fc.out_features), 7.0)


def test_fuse_vert_mlps_swaps_the_classes_only_and_train_mode_calls_the_base_forward():
    from types import SimpleNamespace
    r = SimpleNamespace(gs_valid=_Theirs(1), vert_pos_refinement=_Theirs(3))
    mods = (r.gs_valid, r.vert_pos_refinement)
    ptrs = [[p.data_ptr() for p in m.parameters()] for m in mods]
    assert V.fuse_vert_mlps(r) is r and (r.gs_valid, r.vert_pos_refinement) == mods
    V.fuse_vert_mlps(r)                                            # idempotent
    g = torch.Generator().manual_seed(4)
    x, pts = torch.randn(4, 5, generator=g), torch.randn(4, 3, generator=g)
    for m, p, act in zip(mods, ptrs, ("sigmoid", "tanh_offset")):
        assert isinstance(m, _Theirs) and type(m) is V.fused_vert_cls(_Theirs) and [q.data_ptr() for q in m.parameters()] == p
        m.eval()
        want = V.vert_block(x, pts, V._module_params(m), act=act, radius=0.001)
        assert torch.equal(m(x, pts), want) and m.calls == 0                    # eval: the fused forward, not the base's
        m.train()
        assert float(m(x, pts)[0, 0]) == 7.0 and m.calls == 1                   # train with p = 0.1: the base forward, unchanged
        m.ff.dropout1.p = m.ff.dropout2.p = 0.0
        assert torch.equal(m(x, pts), want) and m.calls == 1                    # train with p = 0: nothing to drop, fused again


def test_own_modules_keep_dropout_in_train_mode(fx):
    x, pts, params, _ = fixture_case(fx, "v")
    m = V.VertValid(131)
    m.load_state_dict({KEYS[k]: p for k, p in zip(V.PARAMS, params)})
    m.train()
    torch.manual_seed(0)
    a = m(x, pts)
    torch.manual_seed(1)
    b = m(x, pts)
    assert not torch.equal(a, b)                                   # dropout is live
    m.eval()
    assert torch.equal(m(x, pts), V.vert_block(x, pts, params))


def test_opt_in_renderer_names_resolve_lazily():
    """tgs_renderer's four new names exist beside the old ones and, like them, import nothing of the reference until asked for."""
    import guassianhand_amd.tgs_renderer as T
    with pytest.raises(AttributeError):
        T.GS3DRendererFusedNothing
    src = open(T.__file__).read()
    for name in ("GS3DRendererFusedGate", "GS3DRendererEditFusedGate", "GS3DRendererFusedAll", "GS3DRendererEditFusedAll"):
        assert name in src
        try:                                                       # the name is known: resolving it reaches for the reference's classes
            cls = getattr(T, name)
        except ImportError:
            continue
        assert isinstance(cls, type) and callable(cls.configure)
