"""The Gaussian trunk on the host (guassianhand_amd/gs_trunk.py): its plain-torch restatement against outputs and gradients CAPTURED
from the reference's own forward_gs statements (tests/golden/make_trunk_fixture.py -> trunk_fixture.npz), the module's state-dict
keys, the seam's choice of path, the C-ABI's symbols and host-side argument checks. No GPU compute is launched here."""
import ctypes as C
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi, _lib
from guassianhand_amd import gs_trunk as T
from guassianhand_amd.gs_head import GSLayer, _activations_keep
from tests.helpers import header_symbols
from tests.res_block_cases import three_way

FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
GUARD = 2.0 ** -16


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "trunk_fixture.npz"), allow_pickle=False)


def _case(fx, t):
    cin, H, cout, width, use_rgb, restrict, relu, clip = fx[f"{t}_cfg"]
    cin, H, cout, width = int(cin), int(H), int(cout), int(width)
    xs, ws, cs = (float(v) for v in fx["scales"])
    f = lambda k: torch.tensor(fx[k]).float() * ws
    x = torch.tensor(fx["x_q"][:, :cin]).float() * xs
    trunk = (f("W1_q")[:H, :cin].contiguous(), torch.tensor(fx[f"{t}_b1"]), f("W2_q")[:H, :H].contiguous(), torch.tensor(fx[f"{t}_b2"]),
             f("W3_q")[:cout, :H].contiguous(), torch.tensor(fx[f"{t}_b3"]))
    kw = dict(shs_width=width, use_rgb=bool(use_rgb), xyz_offset=True, restrict_offset=bool(restrict),
              clip_scaling=None if clip < 0 else float(clip), activation="relu" if relu else "silu")
    cot = {k: torch.tensor(fx[f"{t}_cot_{k}_q"]).float() * cs for k in FIELDS}
    return x, torch.tensor(fx["pts"]), trunk, f("Wh_q")[:11 + width, :cout].contiguous(), torch.tensor(fx[f"{t}_bh"]), kw, cot


def _run(x, pts, trunk, Wh, bh, kw, cot, acc=None):
    dt = acc or torch.float32
    xl, pl = x.clone().requires_grad_(True), pts.clone().requires_grad_(True)
    gm = T._gs_trunk_ref(xl, pl, trunk, Wh, bh, acc=acc, **kw) if acc else T.gs_trunk(xl, pl, trunk, Wh, bh, **kw)
    sum((getattr(gm, k) * cot[k].to(dt)).sum() for k in FIELDS).backward()
    out = {k: getattr(gm, k).detach() for k in FIELDS}
    out["grad_pts"], out["grad_x16"] = pl.grad, xl.grad[::16]
    return out


@pytest.mark.parametrize("t", ["a", "b", "c", "d"])
def test_restatement_reproduces_the_reference_forward_gs(fx, t):
    """gs_trunk on CPU tensors against what the reference's `mlp_net(x)` and `gs_net(x, p)` gave: per field
    max|restatement - f64| <= 4 max|recorded reference - f64| + 2^-20 max|f64|, f64 being the restatement in float64. The ReLU and
    clip cases sit off their kinks by the fixture's margin, asserted here on the float64 values before anything is compared."""
    x, pts, trunk, Wh, bh, kw, cot = _case(fx, t)
    if kw["activation"] == "relu":
        v1 = torch.nn.functional.linear(x.double(), trunk[0].double(), trunk[1].double())
        v2 = torch.nn.functional.linear(torch.relu(v1), trunk[2].double(), trunk[3].double())
        for v in (v1, v2):
            assert float(v.abs().min()) > GUARD * float(v.abs().max()) and bool((v > 0).any()) and bool((v < 0).any())
    f64 = _run(x, pts, trunk, Wh, bh, kw, cot, acc=torch.float64)
    assert f64["xyz"].dtype == torch.float64
    if kw["clip_scaling"] is not None:
        s = T._gs_trunk_ref(x, pts, trunk, Wh, bh, acc=torch.float64, **{**kw, "clip_scaling": None}).scaling
        clip = kw["clip_scaling"]
        assert float((s - clip).abs().min()) > GUARD * float(s.abs().max()) and bool((s > clip).any()) and bool((s < clip).any())
    got = _run(x, pts, trunk, Wh, bh, kw, cot)
    recorded = {k: torch.tensor(fx[f"{t}_{k}"]) for k in FIELDS + ("grad_pts", "grad_x16")}
    for k in recorded:
        assert got[k].shape == recorded[k].shape and got[k].dtype == torch.float32, (t, k)
    three_way(got, recorded, f64, fields=FIELDS + ("grad_pts", "grad_x16"), tag=f"case {t}")


def test_trunk_mlp_carries_the_reference_state_dict(fx):
    keys, shapes = [str(k) for k in fx["init_keys"]], [tuple(int(n) for n in s if n) for s in fx["init_shapes"]]
    m = T.TrunkMLP(131, 128, 128, 2, "silu")
    sd = m.state_dict()
    assert list(sd) == keys == [f"layers.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    assert [tuple(v.shape) for v in sd.values()] == shapes
    m.load_state_dict({k: torch.full(s, 0.5) for k, s in zip(keys, shapes)}, strict=True)
    assert all(float(v.min()) == 0.5 for v in m.state_dict().values())
    assert isinstance(m.layers[1], torch.nn.SiLU) and isinstance(T.TrunkMLP(3, 32, 32, 2, "relu").layers[3], torch.nn.ReLU)
    assert len(T.TrunkMLP(3, 32, 32, 3, "relu").layers) == 7
    w = T.TrunkMLP(131, 128, 128, 2, "silu").layers[0].weight                      # nn.Linear's own initialisation: U(-1/sqrt(fan_in), ..)
    assert 0.5 / 131 ** 0.5 < float(w.detach().abs().max()) <= 1 / 131 ** 0.5
    with pytest.raises(NotImplementedError):
        T.TrunkMLP(3, 32, 32, 2, "tanh")


class _Head(GSLayer):
    """GSLayer's five nn.Linear and its activations in plain torch, in the dtype of its input (the reference's own statements)."""

    def forward(self, x, pts):
        raw = {k: layer(x) for k, layer in zip(self.cfg.feature_channels, self.out_layers)}
        c = self.cfg
        return _activations_keep(raw, pts, c.use_rgb, c.xyz_offset, c.restrict_offset, c.clip_scaling)


class _Renderer(torch.nn.Module):
    """forward_gs and what it reads of the reference's renderer, statement for statement."""

    def __init__(self, mlp=None, use_rgb=True, conf="default", dim_in=9, H=32, act="silu", head=GSLayer):
        super().__init__()
        conf = dict(n_neurons=H, n_hidden_layers=2, activation=act) if conf == "default" else conf
        self.cfg = SimpleNamespace(mlp_network_config=conf)
        if conf is not None:
            self.mlp_net = mlp if mlp is not None else T.TrunkMLP(dim_in, 32, H, conf["n_hidden_layers"], conf["activation"])
        self.gs_net = head(dict(in_channels=32 if conf is not None else dim_in, use_rgb=use_rgb, restrict_offset=True))
        with torch.no_grad():
            for layer in self.gs_net.out_layers:                           # (the reference starts most heads at zero weights)
                layer.weight.normal_(0, 0.1, generator=torch.Generator().manual_seed(layer.out_features))

    def forward_gs(self, x, p):
        if self.cfg.mlp_network_config is not None:
            x = self.mlp_net(x)
        return self.gs_net(x, p)


def _xp(n=7, c=9, dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return torch.randn(n, c, generator=g).to(dtype), 0.1 * torch.randn(n, 3, generator=g).to(dtype)


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in FIELDS)


def test_forward_gs_fused_on_cpu_tensors_is_the_unfused_statements_bit_for_bit():
    r = _Renderer().requires_grad_(False)
    x, p = _xp()
    want = r.forward_gs(x, p)
    assert T.kernel_args(r, x, p) is None                                  # CPU tensors
    assert _same(T.forward_gs_fused(r, x, p), want)
    T.fuse_forward_gs(r)
    assert _same(r.forward_gs(x, p), want)
    r0 = T.fuse_forward_gs(_Renderer(conf=None).requires_grad_(False))      # mlp_network_config: null -> the head alone
    assert T.kernel_args(r0, x, p) is None and tuple(r0.forward_gs(x, p).xyz.shape) == (7, 3)


def _mixed():
    m = T.TrunkMLP(9, 32, 32, 2, "silu")
    m.layers[3] = torch.nn.ReLU()
    return m


def _no_bias():
    m = T.TrunkMLP(9, 32, 32, 2, "silu")
    m.layers[2] = torch.nn.Linear(32, 32, bias=False)
    return m


class _OnDevice(torch.Tensor):                                            # a CPU tensor that says it lives on the device
    is_cuda = True


def _fake(t):
    return t.as_subclass(_OnDevice)


# name -> (the renderer's builder, taking the head's class; what is trainable: "trunk", "head", or None for a case of structure or dtype)
INELIGIBLE = {
    "trainable trunk": (lambda head: _Renderer(head=head), "trunk"),
    "trainable head": (lambda head: _Renderer(head=head), "head"),
    "one hidden layer": (lambda head: _Renderer(conf=dict(n_neurons=32, n_hidden_layers=1, activation="silu"), head=head), None),
    "three hidden layers": (lambda head: _Renderer(conf=dict(n_neurons=32, n_hidden_layers=3, activation="silu"), head=head), None),
    "mixed activations": (lambda head: _Renderer(mlp=_mixed(), head=head), None),
    "a bias-free layer": (lambda head: _Renderer(mlp=_no_bias(), head=head), None),
    "float64": (lambda head: _Renderer(head=head).double(), None),
}


def test_the_stand_in_renderer_is_eligible_when_frozen_and_on_the_device():
    """The premise of the cases below: nothing but the case's own property stands between the stand-in and the kernels."""
    x, p = _xp()
    r = _Renderer().requires_grad_(False)
    assert T.kernel_args(r, x, p) is None                                  # CPU tensors
    args = T.kernel_args(r, _fake(x), _fake(p))
    assert args is not None and args[3]["activation"] == "silu" and tuple(args[1].shape) == (14, 32)
    assert T.kernel_args(_Renderer(act="relu").requires_grad_(False), _fake(x), _fake(p))[3]["activation"] == "relu"
    assert T.kernel_args(r, _fake(x.double()), _fake(p)) is None and T.kernel_args(r, _fake(x), _fake(p.double())) is None
    assert T.kernel_args(r, _fake(x)[:, :8], _fake(p)) is None and T.kernel_args(r, _fake(x), _fake(p)[:6]) is None
    assert T.kernel_args(_Renderer(head=_Head).requires_grad_(False), _fake(x), _fake(p)) is None      # a head with a forward of its own


@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_ineligible_cases_keep_the_unfused_statements_and_every_gradient(name):
    """Each case alone makes kernel_args refuse, the tensors passed off as ROCm ones. A case of structure or dtype is refused on a
    fully frozen renderer, with and without torch.no_grad(), so that the refusal is the property's and not the gradient request's;
    a trainable trunk or head is refused where autograd records, and only there. forward_gs is then the unfused statements, with a
    gradient for every parameter that asks for one."""
    build, trainable = INELIGIBLE[name]
    x, p = _xp(dtype=torch.float64 if name == "float64" else torch.float32)
    frozen = build(GSLayer).requires_grad_(False)
    if trainable is None:
        assert T.kernel_args(frozen, _fake(x), _fake(p)) is None
        with torch.no_grad():
            assert T.kernel_args(frozen, _fake(x), _fake(p)) is None
    else:
        assert T.kernel_args(frozen, _fake(x), _fake(p)) is not None
        (frozen.mlp_net if trainable == "trunk" else frozen.gs_net).requires_grad_(True)
        assert T.kernel_args(frozen, _fake(x), _fake(p)) is None
        with torch.no_grad():
            assert T.kernel_args(frozen, _fake(x), _fake(p)) is not None   # torch.no_grad() qualifies
    # the run itself: a module in training keeps every gradient (float64 needs the plain-torch head: gs_head's own takes float32)
    r = build(_Head if name == "float64" else GSLayer).requires_grad_(False)
    for mod in {"trunk": (r.mlp_net,), "head": (r.gs_net,), None: (r.mlp_net, r.gs_net)}[trainable]:
        mod.requires_grad_(True)
    want = r.forward_gs(x, p)
    T.fuse_forward_gs(r)
    got = r.forward_gs(x, p)
    assert _same(got, want)
    sum(getattr(got, k).sum() for k in FIELDS).backward()
    asked = [n for n, q in r.named_parameters() if q.requires_grad]
    assert asked and all(dict(r.named_parameters())[n].grad is not None for n in asked)


def test_fuse_forward_gs_is_idempotent_and_leaves_the_state_dict_alone():
    r = _Renderer()
    before = {k: v.clone() for k, v in r.state_dict().items()}
    ptrs, mods = [q.data_ptr() for q in r.parameters()], (r.mlp_net, r.gs_net)
    assert T.fuse_forward_gs(r) is r
    cls = type(r)
    assert cls is T.fused_forward_gs_cls(_Renderer) and isinstance(r, _Renderer) and cls.forward_gs is T.forward_gs_fused
    assert T.fuse_forward_gs(r) is r and type(r) is cls
    after = r.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [q.data_ptr() for q in r.parameters()] == ptrs and (r.mlp_net, r.gs_net) == mods
    assert type(T.fuse_forward_gs(_Renderer(use_rgb=False))) is cls        # one cached subclass per base class


def test_library_exports_the_trunk_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.TRUNK_SYMBOLS:
        assert hasattr(L, sym), sym
    assert sorted(_abi.TRUNK_SYMBOLS) == header_symbols("gh_trunk.h") and set(_abi.TRUNK_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert any(s.endswith("gh_trunk.hip") for s in _lib.SOURCES) and any(h.endswith("gh_trunk.h") for h in _lib.HEADERS)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gh_trunk.h")).read()
    for name in ("GH_TRUNK_SILU", "GH_TRUNK_RELU", "GH_TRUNK_ROWS", "GH_TRUNK_MAX_CIN"):
        assert f"#define {name} {getattr(_abi, name)}" in h, name


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for null pointers, sizes outside the kernels' and bad descriptors (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    one = C.c_void_p(1 << 20)
    ok = _abi.GhHeadDesc(3, _abi.GH_HEAD_USE_RGB | _abi.GH_HEAD_XYZ_OFFSET, 0.0)

    def fwd(d=ok, P=10, Cin=131, H=128, Cout=128, stride=131, x=one, W2=one, xyz=one, act=_abi.GH_TRUNK_SILU):
        return L.gh_trunk_forward(x, stride, P, Cin, H, Cout, one, one, one, W2, one, one, one, one, one, C.byref(d) if d else None, act,
                                  xyz, one, one, one, one, one, None)

    def bwd(d=ok, P=10, Cin=131, H=128, Cout=128, stride=131, raw=one, gx=one, gstride=131, act=_abi.GH_TRUNK_SILU):
        return L.gh_trunk_backward(raw, one, stride, P, Cin, H, Cout, one, one, one, one, one, one, C.byref(d) if d else None, act,
                                   one, None, None, None, None, gx, gstride, None, None)

    for call in (fwd, bwd):
        assert call(d=None) == _abi.GH_ERR_INVALID_ARG
        assert call(H=48) == call(Cout=48) == call(H=160) == _abi.GH_ERR_UNSUPPORTED
        assert call(Cin=193, stride=193) == _abi.GH_ERR_UNSUPPORTED
        assert call(d=_abi.GhHeadDesc(4, _abi.GH_HEAD_XYZ_OFFSET, 0.0)) == _abi.GH_ERR_UNSUPPORTED               # O = 15
        assert call(d=_abi.GhHeadDesc(48, _abi.GH_HEAD_USE_RGB, 0.0)) == _abi.GH_ERR_UNSUPPORTED
        assert call(d=_abi.GhHeadDesc(3, 64, 0.0)) == _abi.GH_ERR_INVALID_ARG                                    # unknown flag
        assert call(Cin=0) == call(P=-1) == call(stride=130) == call(act=2) == _abi.GH_ERR_INVALID_ARG
        assert call(P=0) == _abi.GH_OK                                                                           # nothing to do, no launch
    assert fwd(x=None) == fwd(W2=None) == fwd(xyz=None) == _abi.GH_ERR_INVALID_ARG
    assert bwd(raw=None) == bwd(gx=None) == bwd(gstride=130) == _abi.GH_ERR_INVALID_ARG
    assert fwd(x=C.c_void_p((1 << 20) + 2)) == _abi.GH_ERR_INVALID_ARG                                           # 4-byte alignment


def test_python_refuses_bad_arguments_on_the_host():
    x, p = _xp()
    r = _Renderer()
    l1, _, l2, _, l3 = r.mlp_net.layers
    trunk = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    Wh, bh = torch.zeros(14, 32), torch.zeros(14)
    kw = dict(shs_width=3, use_rgb=True)
    T.gs_trunk(x, p, trunk, Wh, bh, **kw)
    with pytest.raises(ValueError, match="activation"):
        T.gs_trunk(x, p, trunk, Wh, bh, activation="tanh", **kw)
    with pytest.raises(ValueError, match="six|6|trunk must"):
        T.gs_trunk(x, p, trunk[:4], Wh, bh, **kw)
    with pytest.raises(ValueError, match="chain"):
        T.gs_trunk(x, p, trunk[:2] + [torch.zeros(32, 31)] + trunk[3:], Wh, bh, **kw)
    with pytest.raises(ValueError, match="11 \\+ shs_width"):
        T.gs_trunk(x, p, trunk, torch.zeros(59, 32), torch.zeros(59), **kw)
    with pytest.raises(TypeError, match="float32"):
        T.gs_trunk(x.double(), p, trunk, Wh, bh, **kw)
    with pytest.raises(ValueError, match="ops"):
        T.gs_trunk(x, p, trunk, Wh, bh, ops="eager", **kw)


@pytest.fixture
def no_livehand():
    """The two Uvd names register the livehand shim where livehand is absent: take it out again."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "livehand" or k.startswith("livehand.")}
    yield
    for k in [k for k in sys.modules if k == "livehand" or k.startswith("livehand.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    importlib.invalidate_caches()


def test_opt_in_renderer_names_resolve_lazily(no_livehand):
    """The six new names go through tgs_renderer's own construction: where the reference is importable they resolve to classes whose
    configure() is the graft; elsewhere resolving them reaches for the reference's classes and for nothing else."""
    import importlib.util
    import guassianhand_amd.tgs_renderer as R
    for suffix, inner in (("FusedTrunk", ""), ("FusedAllFetchAttnBlockTrunk", "FusedAllFetchAttnBlock"),
                          ("FusedAllFetchAttnBlockUvdTrunk", "FusedAllFetchAttnBlockUvd")):
        assert R._VARIANTS[suffix] == R._VARIANTS.get(inner, ()) + ("head", "trunk")          # the fused head, then the trunk over it
    assert [s for s, row in R._VARIANTS.items() if "trunk" in row] == ["FusedTrunk", "FusedAllFetchAttnBlockTrunk", "FusedAllFetchAttnBlockUvdTrunk"]
    with pytest.raises(AttributeError):
        R.GS3DRendererFusedGateTrunk
    have_reference = importlib.util.find_spec("tgs") is not None
    for name in ("GS3DRendererFusedTrunk", "GS3DRendererEditFusedTrunk", "GS3DRendererFusedAllFetchAttnBlockTrunk",
                 "GS3DRendererEditFusedAllFetchAttnBlockTrunk", "GS3DRendererFusedAllFetchAttnBlockUvdTrunk",
                 "GS3DRendererEditFusedAllFetchAttnBlockUvdTrunk"):
        if not have_reference:                                     # the name is known: resolving it reaches for the reference's classes
            with pytest.raises(ImportError) as e:
                getattr(R, name)
            assert (e.value.name or "").split(".")[0] == "tgs"      # and for nothing else that is missing
            continue
        cls = getattr(R, name)
        assert isinstance(cls, type) and callable(cls.configure)


def test_trunk_configure_applies_both_grafts(monkeypatch):
    """The class a ...Trunk name builds, over a stand-in base in place of the reference's: configure() is the base's, then
    fuse_gs_head and fuse_forward_gs on the same object."""
    import guassianhand_amd.tgs_renderer as R

    class Base(_Renderer):
        """stand-in"""
        configured = 0

        def configure(self):
            self.configured += 1

    monkeypatch.setitem(R._cache, "GS3DRenderer", Base)
    monkeypatch.delitem(R._cache, "GS3DRendererFusedTrunk", raising=False)
    cls = R.GS3DRendererFusedTrunk
    monkeypatch.delitem(R._cache, "GS3DRendererFusedTrunk", raising=False)          # (nothing built on the stand-in stays cached)
    assert issubclass(cls, Base) and cls is not Base
    r = cls(head=_Head)
    net = r.gs_net
    r.configure()
    assert r.configured == 1 and type(r) is T.fused_forward_gs_cls(cls) and type(r).forward_gs is T.forward_gs_fused
    assert r.gs_net is net and isinstance(net, GSLayer)
