"""The Gaussian head on the host (guassianhand_amd/gs_head.py): its plain-torch restatement against outputs and gradients CAPTURED from
the reference's own GSLayer (tests/golden/make_gs_head_fixture.py -> gs_head_fixture.npz), the module's state-dict keys and
initialisation, the C-ABI's symbols and host-side argument checks. No GPU compute is launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import gs_head as H
from tests.helpers import header_symbols

FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "gs_head_fixture.npz"), allow_pickle=False)


def _case(fx, t):
    cin, width, use_rgb, restrict, xyz_offset, clip = fx[f"{t}_cfg"]
    cin, width = int(cin), int(width)
    xs, ws, cs = (float(v) for v in fx["scales"])
    x = torch.tensor(fx["x_q"][:, :cin]).float() * xs
    W = torch.tensor(fx["W_q"][:11 + width, :cin]).float() * ws
    kw = dict(shs_width=width, use_rgb=bool(use_rgb), xyz_offset=bool(xyz_offset), restrict_offset=bool(restrict),
              clip_scaling=None if clip < 0 else float(clip))
    cot = {k: torch.tensor(fx[f"{t}_cot_{k}_q"]).float() * cs for k in FIELDS}
    return x, torch.tensor(fx["pts"]), W, torch.tensor(fx[f"{t}_bias"]), kw, cot


@pytest.mark.parametrize("t", ["a", "b", "c", "d"])
def test_restatement_reproduces_the_reference_gslayer(fx, t):
    """gs_head on CPU tensors (gs_activations over ONE F.linear of the concatenated heads) against the reference's five nn.Linear calls
    and its activations: the recorded outputs bit for bit (the fixture's dot products are exact in float32), and the gradients of the
    recorded cotangents to float32 rounding of their O- and P-term sums, which one GEMM and five split differently."""
    x, pts, W, b, kw, cot = _case(fx, t)
    leaves = [v.clone().requires_grad_(True) for v in (x, pts, W, b)]
    gm = H.gs_head(*leaves, **kw)
    assert isinstance(gm, H.GaussianModel)
    for k in FIELDS:
        got, want = getattr(gm, k).detach().numpy(), fx[f"{t}_{k}"]
        assert got.shape == want.shape, (t, k)
        assert np.array_equal(got, want), (t, k, float(np.abs(got - want).max()))
    sum((getattr(gm, k) * cot[k]).sum() for k in FIELDS).backward()
    gx, gp, gW, gb = (v.grad for v in leaves)
    assert np.array_equal(gp.numpy(), fx[f"{t}_grad_pts"])
    # yardstick for the sums: the same gradients in float64
    l64 = [v.detach().clone().requires_grad_(True) for v in (x, pts, W, b)]
    gm64 = H._gs_head_ref(*l64, **kw, acc=torch.float64)
    assert gm64.xyz.dtype == torch.float64 and gm64.scaling.dtype == torch.float64
    sum((getattr(gm64, k) * cot[k].double()).sum() for k in FIELDS).backward()
    for name, got, want, ref in (("grad_x", gx[::16], fx[f"{t}_grad_x16"], l64[0].grad[::16]), ("grad_bias", gb, fx[f"{t}_grad_bias"], l64[3].grad)) + \
            ((("grad_weight", gW, fx[f"{t}_grad_weight"], l64[2].grad),) if f"{t}_grad_weight" in fx.files else ()):
        want = torch.tensor(want)
        e_ref = float((want.double() - ref).abs().max())              # the reference's own float32 error
        e_got = float((got.double() - ref).abs().max())
        floor = 2.0 ** -22 * float(ref.abs().max())
        assert e_got <= 2 * e_ref + floor, (t, name, e_got, e_ref)


def test_restatement_options(fx):
    """ops="torch" is the same function on any device; without xyz_offset the positions pass through and the xyz head gets no gradient."""
    x, pts, W, b, kw, cot = _case(fx, "a")
    a, c = H.gs_head(x, pts, W, b, **kw), H.gs_head(x, pts, W, b, ops="torch", **kw)
    assert all(torch.equal(getattr(a, k), getattr(c, k)) for k in FIELDS)
    Wl = W.clone().requires_grad_(True)
    gm = H.gs_head(x, pts, Wl, b, **{**kw, "xyz_offset": False})
    assert torch.equal(gm.xyz, pts)
    (gm.xyz.sum() + gm.opacity.sum()).backward()
    assert float(Wl.grad[:3].abs().max()) == 0.0 and float(Wl.grad[10].abs().max()) > 0
    empty = H.gs_head(x[:0], pts[:0], W, b, **kw)
    assert [tuple(getattr(empty, k).shape) for k in FIELDS] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, 1, 3)]


@pytest.mark.parametrize("tag,use_rgb", [("rgb", True), ("sh", False)])
def test_module_carries_the_reference_state_dict_and_initialisation(fx, tag, use_rgb):
    """A state dict with the reference's keys (recorded from its configure()) loads into gs_head.GSLayer unchanged, and a fresh module
    reproduces the reference's initial values: zero weights except the RGB head, scaling bias -5, rotation bias (1,0,0,0), opacity
    bias logit(0.1)."""
    keys = sorted(k[len(f"init_{tag}."):] for k in fx.files if k.startswith(f"init_{tag}."))
    m = H.GSLayer(dict(in_channels=128, use_rgb=use_rgb))
    assert sorted(m.state_dict().keys()) == keys == sorted(f"out_layers.{i}.{p}" for i in range(5) for p in ("weight", "bias"))
    sd = {}
    for k in keys:
        v = fx[f"init_{tag}.{k}"]
        want_shape = tuple(m.state_dict()[k].shape)
        if v.dtype.kind == "i":                                    # an all-zero tensor, stored as its shape
            assert tuple(int(n) for n in v) == want_shape, k
            sd[k] = torch.zeros(want_shape)
        else:
            assert v.shape == want_shape, k
            sd[k] = torch.tensor(v)
    fresh = m.state_dict()
    for k in keys:
        if not (use_rgb and k.startswith("out_layers.4.")):       # (the RGB head keeps nn.Linear's random initialisation)
            assert torch.equal(fresh[k], sd[k]), k
    assert float(fresh["out_layers.4.weight"].abs().max()) > 0 if use_rgb else True
    assert torch.equal(fresh["out_layers.1.bias"], torch.full((3,), -5.0))
    assert torch.equal(fresh["out_layers.2.bias"], torch.tensor([1.0, 0.0, 0.0, 0.0]))
    assert abs(float(fresh["out_layers.3.bias"]) - math.log(0.1 / 0.9)) < 1e-6
    assert tuple(fresh["out_layers.4.weight"].shape) == ((3, 128) if use_rgb else (48, 128))
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in keys)
    # the module's forward is gs_head over the concatenated parameters, whatever order feature_channels lists the heads in
    g = torch.Generator().manual_seed(1)
    x, pts = torch.randn(5, 128, generator=g), torch.randn(5, 3, generator=g)
    out = m(x, pts)
    W = torch.cat([m.out_layers[i].weight for i in range(5)])
    b = torch.cat([m.out_layers[i].bias for i in range(5)])
    want = H.gs_head(x, pts, W, b, shs_width=3 if use_rgb else 48, use_rgb=use_rgb)
    assert all(torch.equal(getattr(out, k), getattr(want, k)) for k in FIELDS)
    m2 = H.GSLayer(in_channels=128, use_rgb=use_rgb, feature_channels=dict(shs=48, opacity=1, xyz=3, rotation=4, scaling=3))
    for key, layer in zip(m2.cfg.feature_channels, m2.out_layers):
        src = m.out_layers[list(m.cfg.feature_channels).index(key)]
        layer.load_state_dict(src.state_dict())
    out2 = m2(x, pts)
    assert all(torch.equal(getattr(out2, k), getattr(want, k)) for k in FIELDS)


def test_fuse_gs_head_swaps_the_class_only():
    """fuse_gs_head on an object whose gs_net is someone else's GSLayer-shaped module: the class changes to a subclass, the module
    object and its parameters do not, and the forward becomes gs_head's."""
    from types import SimpleNamespace

    class Theirs(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = SimpleNamespace(feature_channels=dict(xyz=3, scaling=3, rotation=4, opacity=1, shs=48), use_rgb=True,
                                       xyz_offset=True, restrict_offset=True, clip_scaling=0.01)
            self.out_layers = torch.nn.ModuleList(torch.nn.Linear(7, n) for n in (3, 3, 4, 1, 3))

        def forward(self, x, pts):
            raise AssertionError("the base forward must not run")

    r = SimpleNamespace(gs_net=Theirs())
    net, params = r.gs_net, [p.data_ptr() for p in r.gs_net.parameters()]
    assert H.fuse_gs_head(r) is r and r.gs_net is net
    assert isinstance(net, Theirs) and type(net) is not Theirs and type(net) is H.fused_gs_layer_cls(Theirs)
    assert [p.data_ptr() for p in net.parameters()] == params
    H.fuse_gs_head(r)                                              # idempotent
    assert type(net) is H.fused_gs_layer_cls(Theirs)
    g = torch.Generator().manual_seed(2)
    x, pts = torch.randn(4, 7, generator=g), torch.randn(4, 3, generator=g)
    out = net(x, pts)
    W, b = torch.cat([l.weight for l in net.out_layers]), torch.cat([l.bias for l in net.out_layers])
    want = H.gs_head(x, pts, W, b, shs_width=3, use_rgb=True, restrict_offset=True, clip_scaling=0.01)
    assert all(torch.equal(getattr(out, k), getattr(want, k)) for k in FIELDS)


def test_library_exports_the_head_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.HEAD_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_head(L)
    assert sorted(_abi.HEAD_SYMBOLS) == header_symbols("gh_head.h")
    nb = -(-98562 // _abi.GH_HEAD_ROWS)
    assert L.gh_head_workspace_bytes(98562, 128, 14) >= 4 * nb * 14 * (128 + 1)
    assert L.gh_head_workspace_bytes(1, 3, 59) > 0
    for P, Cin, O in ((0, 128, 14), (-1, 128, 14), (10, 0, 14), (10, 128, 13), (10, 128, 15), (10, 128, 60), (10, 128, 11), (10, 128, 0)):
        assert L.gh_head_workspace_bytes(P, Cin, O) == 0, (P, Cin, O)


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for bad descriptors, sizes, null pointers and a short workspace (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_head(L)
    one = C.c_void_p(1 << 20)
    ok = _abi.GhHeadDesc(3, _abi.GH_HEAD_USE_RGB | _abi.GH_HEAD_XYZ_OFFSET, 0.0)
    fwd = lambda d, P=10, Cin=128, stride=128, x=one, raw=one: L.gh_head_forward(x, stride, P, Cin, one, one, one, C.byref(d) if d else None,
                                                                                  one, one, one, one, one, raw, None)
    assert fwd(None) == _abi.GH_ERR_INVALID_ARG
    assert fwd(_abi.GhHeadDesc(5, 0, 0.0)) == _abi.GH_ERR_UNSUPPORTED                              # shs width
    assert fwd(_abi.GhHeadDesc(48, _abi.GH_HEAD_USE_RGB, 0.0)) == _abi.GH_ERR_UNSUPPORTED          # use_rgb with 48 channels
    assert fwd(_abi.GhHeadDesc(3, 64, 0.0)) == _abi.GH_ERR_INVALID_ARG                             # unknown flag
    assert fwd(_abi.GhHeadDesc(3, _abi.GH_HEAD_CLIP_SCALING, -1.0)) == _abi.GH_ERR_INVALID_ARG
    assert fwd(_abi.GhHeadDesc(3, _abi.GH_HEAD_CLIP_SCALING, float("nan"))) == _abi.GH_ERR_INVALID_ARG
    assert fwd(ok, P=0) == fwd(ok, Cin=0) == fwd(ok, stride=127) == fwd(ok, x=None) == _abi.GH_ERR_INVALID_ARG
    bwd = lambda gW, gb, ws, nbytes, x=one: L.gh_head_backward(one, x, 128, 10, 128, one, C.byref(ok), one, None, None, None, None, one, 128,
                                                               None, gW, gb, ws, nbytes, None)
    assert bwd(one, None, one, 1 << 30) == bwd(None, one, one, 1 << 30) == _abi.GH_ERR_INVALID_ARG   # grad_W and grad_b: both or neither
    assert bwd(one, one, one, 16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert bwd(one, one, None, 1 << 30) == bwd(one, one, one, 1 << 30, x=None) == _abi.GH_ERR_INVALID_ARG
    assert L.gh_head_backward(None, one, 128, 10, 128, one, C.byref(ok), *[None] * 5, one, 128, None, None, None, None, 0, None) == _abi.GH_ERR_INVALID_ARG
    assert L.gh_head_backward(one, one, 128, 10, 128, one, C.byref(ok), *[None] * 5, one, 127, None, None, None, None, 0, None) == _abi.GH_ERR_INVALID_ARG


def test_python_refuses_bad_arguments_on_the_host():
    """Wrong dtype, wrong O for the flags and a P mismatch between x and pts raise before any device work (CPU tensors here: the
    checks run ahead of the choice of path)."""
    x, pts, W, b = torch.zeros(6, 16), torch.zeros(6, 3), torch.zeros(14, 16), torch.zeros(14)
    kw = dict(shs_width=3, use_rgb=True)
    H.gs_head(x, pts, W, b, **kw)
    with pytest.raises(TypeError, match="float32"):
        H.gs_head(x.double(), pts, W, b, **kw)
    with pytest.raises(TypeError, match="float32"):
        H.gs_head(x, pts, W.half(), b, **kw)
    with pytest.raises(ValueError, match="11 \\+ shs_width"):
        H.gs_head(x, pts, torch.zeros(59, 16), torch.zeros(59), **kw)                   # the SH head's rows under the RGB flags
    with pytest.raises(ValueError, match="11 \\+ shs_width"):
        H.gs_head(x, pts, W, b, shs_width=48)
    with pytest.raises(ValueError, match="use_rgb needs"):
        H.gs_head(x, pts, torch.zeros(59, 16), torch.zeros(59), shs_width=48, use_rgb=True)
    with pytest.raises(ValueError, match="shs_width must be"):
        H.gs_head(x, pts, torch.zeros(16, 16), torch.zeros(16), shs_width=5)
    with pytest.raises(ValueError, match="pts"):
        H.gs_head(x, pts[:5], W, b, **kw)
    with pytest.raises(ValueError, match="columns"):
        H.gs_head(x[:, :8], pts, W, b, **kw)
    with pytest.raises(ValueError, match="clip_scaling"):
        H.gs_head(x, pts, W, b, clip_scaling=-0.1, **kw)
    with pytest.raises(ValueError, match="ops"):
        H.gs_head(x, pts, W, b, ops="eager", **kw)


def test_opt_in_renderer_names_resolve_lazily():
    """tgs_renderer's two new names exist beside the old ones and, like them, import nothing of the reference until asked for."""
    import guassianhand_amd.tgs_renderer as T
    with pytest.raises(AttributeError):
        T.NoSuchRenderer
    src = open(T.__file__).read()
    assert "GS3DRendererFusedHead" in src and "GS3DRendererEditFusedHead" in src
