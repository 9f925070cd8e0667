"""The point conditioning on the host (guassianhand_amd/cond.py): PointRows.dense() and the plain-torch restatement of
additional_features_fc against values CAPTURED from the reference's own SpatialEncoder and additional_features_fc
(tests/golden/make_cond_fixture.py -> cond_fixture.npz), the split linear form, the module's state-dict keys and initialisation, the
C-ABI's symbols and host-side argument checks, and the fallbacks. No GPU compute is launched here."""
import ctypes as C
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import _abi
from guassianhand_amd import cond
from tests.helpers import header_symbols

KEYS = {"ln_weight": "ff1.layer_norm.weight", "ln_bias": "ff1.layer_norm.bias", "fc1_weight": "ff1.fc1.weight", "fc1_bias": "ff1.fc1.bias",
        "fc2_weight": "ff1.fc2.weight", "fc2_bias": "ff1.fc2.bias"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "cond_fixture.npz"), allow_pickle=False)


def fixture_case(fx):
    """(dict of the inputs of TGS._forward's two statements, params in cond.PARAMS order, cotangent)"""
    s_code, s_pose, s_ln, s_fc1, s_fc2, s_cot = (float(v) for v in fx["scales"])
    t = lambda k: torch.tensor(fx[k])
    inp = {"uv": t("uv"), "xyz": t("xyz"), "flag": t("flag"), "code": t("code_q").float() * s_code, "pose": t("pose_q").float() * s_pose}
    params = [1.0 + t("ln_weight_q").float() * s_ln, t("ln_bias_q").float() * s_ln, t("fc1_weight_q").float() * s_fc1, t("fc1_bias"),
              t("fc2_weight_q").float() * s_fc2, t("fc2_bias")]
    return inp, params, t("cot_q").float() * s_cot


def full_rows(inp, code=None):
    return cond.PointRows(uv=inp["uv"], xyz=inp["xyz"], flag=inp["flag"], code=inp["code"] if code is None else code, broadcast=(inp["pose"],))


def within_twice(name, got, want, ref):
    """The rule of tests/test_vert_mlp_cpu.py: got within twice the reference's own float32 error against float64, plus 2^-22 max|f64|."""
    want = torch.as_tensor(want)
    assert got.shape == want.shape == ref.shape, name
    e_ref, e_got = float((want.double() - ref).abs().max()), float((got.double() - ref).abs().max())
    floor = 2.0 ** -22 * float(ref.abs().max())
    print(f"{name:12s} got-f64 {e_got:.3e}  reference-f64 {e_ref:.3e}  max|f64| {float(ref.abs().max()):.3e}")
    assert e_got <= 2 * e_ref + floor, (name, e_got, e_ref, floor)


def test_dense_is_the_reference_concatenation_bit_for_bit(fx):
    inp, _, _ = fixture_case(fx)
    rows = full_rows(inp)
    d = rows.dense()
    assert (rows.B, rows.N, rows.Dv, rows.De, rows.Cc) == (2, 32, 84, 768, 33) and tuple(d.shape) == (2, 32, 852) and d.dtype == torch.float32
    assert torch.equal(d[..., 0:2], inp["uv"]) and torch.equal(d[..., 2:20], torch.tensor(fx["uv_sp"]))
    assert torch.equal(d[..., 20:23], inp["xyz"]) and torch.equal(d[..., 23:50], torch.tensor(fx["xyz_sp"]))
    assert torch.equal(d[..., 50:51], inp["flag"].float()) and torch.equal(d[..., 51:84], inp["code"])
    assert torch.equal(d[..., 84:], inp["pose"].repeat(1, 32, 1))
    assert torch.equal(cond.spatial_encode(inp["uv"], 4), torch.tensor(fx["uv_sp"]))
    assert torch.equal(rows.varying(), d[..., :84]) and torch.equal(rows.uv_columns(), inp["uv"])
    # the sp output repeats x: u, v, u, v, then per level sin(u), sin(v), cos(u), cos(v)
    y = (inp["uv"] * np.float32(np.pi * 2)).float()
    assert torch.equal(d[..., 2:4], inp["uv"]) and torch.equal(d[..., 8:10], torch.sin(y)) and torch.equal(d[..., 10:12], torch.cos(y))
    # the widths of the three layouts of _forward
    shade = cond.PointRows(uv=inp["uv"], xyz=inp["xyz"], flag=inp["flag"], broadcast=(inp["pose"], inp["pose"]))
    texture = cond.PointRows(uv=inp["uv"], code=inp["code"])
    assert (shade.Dv, shade.De, texture.Dv, texture.De) == (51, 1536, 53, 0)
    assert tuple(shade.dense().shape) == (2, 32, 1587) and tuple(texture.dense().shape) == (2, 32, 53)


def test_restatement_reproduces_the_reference_module(fx):
    """cond_mlp and additional_features on CPU tensors against the reference's module in eval(): the output and the gradient of
    identity_code_vert within twice the reference's own float32 error against the float64 restatement."""
    inp, params, cot = fixture_case(fx)
    code = inp["code"].clone().requires_grad_(True)
    out = cond.cond_mlp(full_rows(inp, code), params)
    assert out.dtype == torch.float32
    (out * cot).sum().backward()
    c64 = inp["code"].clone().requires_grad_(True)
    out64 = cond._cond_mlp_ref(full_rows(inp, c64), params, acc=torch.float64)
    assert out64.dtype == torch.float64
    (out64 * cot.double()).sum().backward()
    within_twice("out", out.detach(), fx["out"], out64.detach())
    within_twice("grad_code", code.grad, fx["grad_code"], c64.grad)
    m = cond.AdditionalFeaturesFC(852, 51).eval()
    m.load_state_dict({KEYS[k]: p for k, p in zip(cond.PARAMS, params)}, strict=True)
    seam = cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], inp["code"], inp["pose"])
    assert torch.equal(seam, out.detach()) and torch.equal(m(full_rows(inp)), seam) and torch.equal(m(full_rows(inp).dense()), seam)


def test_module_carries_the_reference_state_dict_and_initialisation(fx):
    keys = sorted(k[len("init."):] for k in fx.files if k.startswith("init."))
    torch.manual_seed(3)
    m = cond.AdditionalFeaturesFC(852, 51)
    sd = m.state_dict()
    assert sorted(sd.keys()) == keys == sorted(KEYS.values())
    for k in keys:
        assert tuple(sd[k].shape) == tuple(int(n) for n in fx[f"init.{k}"]), k
    for name in ("ff1.fc1", "ff1.fc2"):                            # Xavier-uniform weights, zero biases
        w = sd[f"{name}.weight"]
        bound = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
        assert 0.5 * bound < float(w.abs().max()) <= bound, name
        assert float(sd[f"{name}.bias"].abs().max()) == 0.0, name
    assert torch.equal(sd["ff1.layer_norm.weight"], torch.ones(852)) and torch.equal(sd["ff1.layer_norm.bias"], torch.zeros(852))
    assert m.ff1.layer_norm.eps == 1e-6 and m.ff1.dropout1.p == 0.1 and m.ff1.dropout2.p == 0.1


def test_train_mode_runs_the_reference_statements_dropout_included(fx):
    inp, params, _ = fixture_case(fx)
    m = cond.AdditionalFeaturesFC(852, 51)
    m.load_state_dict({KEYS[k]: p for k, p in zip(cond.PARAMS, params)})
    m.train()
    torch.manual_seed(0)
    a = cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], inp["code"], inp["pose"])
    torch.manual_seed(0)
    feats = torch.cat([inp["uv"], cond.spatial_encode(inp["uv"], 4), inp["xyz"], cond.spatial_encode(inp["xyz"], 4), inp["flag"], inp["code"],
                       inp["pose"].repeat(1, 32, 1)], dim=-1)
    b = m.ff1(feats)
    torch.manual_seed(1)
    c = cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], inp["code"], inp["pose"])
    assert torch.equal(a, b) and not torch.equal(a, c)             # dropout is live, and drawn as the reference's statements draw it
    m.ff1.dropout1.p = m.ff1.dropout2.p = 0.0
    assert torch.equal(cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], inp["code"], inp["pose"]), cond.cond_mlp(full_rows(inp), params))


@pytest.mark.parametrize("layout", ["shade", "texture"])
def test_linear_is_the_linear_layer_over_the_concatenation(fx, layout):
    """PointRows.linear(fc) against F.linear(dense()) for the two encoder inputs of _forward: within twice F.linear's own float32
    error against float64, output and the gradients of code, weight, bias and the broadcast vectors."""
    inp, _, _ = fixture_case(fx)
    g = torch.Generator().manual_seed(21)
    cam = torch.randn(2, 1, 768, generator=g)
    width = 1587 if layout == "shade" else 53
    fc = torch.nn.Linear(width, 256)
    with torch.no_grad():
        fc.weight.copy_(torch.randn(256, width, generator=g) / width ** 0.5)
        fc.bias.copy_(0.2 * torch.randn(256, generator=g))
    cot = torch.randn(2, 32, 256, generator=g)

    def run(mode):
        dt = torch.float64 if mode == "f64" else torch.float32
        leaves = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in (("code", inp["code"]), ("pose", inp["pose"]), ("cam", cam),
                                                                                 ("weight", fc.weight), ("bias", fc.bias))}
        if layout == "shade":
            rows = cond.PointRows(uv=inp["uv"].to(dt), xyz=inp["xyz"].to(dt), flag=inp["flag"], broadcast=(leaves["pose"], leaves["cam"]))
        else:
            rows = cond.PointRows(uv=inp["uv"].to(dt), code=leaves["code"])
        layer = SimpleNamespace(weight=leaves["weight"], bias=leaves["bias"])      # (linear() reads .weight and .bias)
        out = rows.linear(layer) if mode == "split" else F.linear(rows.dense(), leaves["weight"], leaves["bias"])
        names = ("weight", "bias") + (("pose", "cam") if layout == "shade" else ("code",))
        grads = torch.autograd.grad((out * cot.to(dt)).sum(), [leaves[k] for k in names])
        res = {"out": out.detach(), **{f"grad_{k}": v for k, v in zip(names, grads)}}
        return res

    f64, t32, split = run("f64"), run("t32"), run("split")
    assert sorted(split) == sorted(t32) and split["out"].dtype == torch.float32
    for k in sorted(split):
        within_twice(f"{layout} {k}", split[k], t32[k], f64[k])


def test_pointnet_forward_takes_point_rows(fx):
    """pool.pointnet_forward over a PointRows equals the same encoder over dense() up to the first layer's rounding (CPU, plain torch)."""
    from guassianhand_amd import pool
    inp, _, _ = fixture_case(fx)
    torch.manual_seed(2)
    enc = pool.LocalPoolPointnet(input_channels=53, c_dim=8, hidden_dim=16, plane_size=4, n_blocks=3).eval()
    for blk in enc.blocks:
        torch.nn.init.normal_(blk.fc_1.weight, std=0.1)
    rows = cond.PointRows(uv=inp["uv"] * 2 - 1, code=inp["code"])
    a, b = enc(rows), enc(rows.dense())
    assert tuple(a.shape) == tuple(b.shape) == (2, 8, 4, 4)
    assert float((a - b).detach().abs().max()) <= 1e-5 * float(b.detach().abs().max()) and float(b.detach().abs().max()) > 0
    with pytest.raises(ValueError, match="expected"):
        enc(rows.dense()[0])


def test_fallbacks_never_raise_where_the_statements_work(fx):
    """levels outside 1..8, Cc > 64, Hd > 64, float64: the plain-torch restatement, on any input the reference's statements accept."""
    inp, _, _ = fixture_case(fx)
    g = torch.Generator().manual_seed(6)

    def params(D, Hd, dt=torch.float32):
        return [torch.randn(s, generator=g).to(dt) for s in ((D,), (D,), (Hd, D), (Hd,), (Hd, Hd), (Hd,))]

    for levels, Cc, Hd, dt in ((0, 33, 51, torch.float32), (9, 33, 51, torch.float32), (4, 65, 51, torch.float32), (4, 33, 65, torch.float32),
                               (4, 33, 51, torch.float64)):
        code = torch.randn(2, 32, Cc, generator=g).to(dt)
        rows = cond.PointRows(uv=inp["uv"].to(dt), xyz=inp["xyz"].to(dt), flag=inp["flag"], code=code, broadcast=(inp["pose"].to(dt),), levels=levels)
        D = (2 + 3) * (2 + 2 * levels) + 1 + Cc + 768
        assert rows.Dv + rows.De == D == rows.dense().shape[-1]
        out = cond.cond_mlp(rows, params(D, Hd, dt))
        assert tuple(out.shape) == (2, 32, Hd) and out.dtype == dt
    with pytest.raises(ValueError, match="ops"):
        cond.cond_mlp(full_rows(inp), params(852, 51), ops="eager")
    with pytest.raises(ValueError, match="ln_weight: expected"):
        cond.cond_mlp(full_rows(inp), params(851, 51))
    with pytest.raises(ValueError, match="at least one"):
        cond.PointRows(broadcast=(inp["pose"],))
    with pytest.raises(ValueError, match="xyz: expected"):
        cond.PointRows(uv=inp["uv"], xyz=inp["xyz"][:, :31])
    empty = cond.PointRows(uv=inp["uv"][:, :0], code=inp["code"][:, :0], broadcast=(inp["pose"],))
    assert tuple(cond.cond_mlp(empty, params(53 + 768, 7)).shape) == (2, 0, 7)


def test_symbols_and_the_untouched_rasteriser_sources(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.COND_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_cond(L)
    assert sorted(_abi.COND_SYMBOLS) == header_symbols("gh_cond.h")
    assert set(_abi.COND_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    assert cond.PARAMS == tuple(KEYS) == tuple(n for n, _ in _abi.GhCondParams._fields_)
    from guassianhand_amd import _lib
    assert any(s.endswith("gh_cond.hip") for s in _lib.SOURCES) and any(h.endswith("gh_cond.h") for h in _lib.HEADERS)
    import bench
    assert bench.source_hash() == json.load(open(os.path.join(ROOT, "profiles", "r6_pmc_traffic.json")))["source_hash"]
    _abi.declare_raster(L)
    assert int(L.gh_version()) == (0 << 16) | 8 and (_abi.GH_VERSION_MAJOR, _abi.GH_VERSION_MINOR) == (0, 8)


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Widths, fold sizes and status codes (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_cond(L)
    a, one, bad = 1 << 20, C.c_void_p(1 << 20), _abi.GH_ERR_INVALID_ARG
    rows = lambda uv=a, xyz=a, flag=a, code=a, stride=33, Cc=33, L_=4: _abi.GhCondRows(uv, xyz, flag, code, stride, Cc, L_)
    width = lambda r: L.gh_cond_width(C.byref(r))
    assert width(rows()) == 84 and width(rows(code=None, stride=0, Cc=0)) == 51 and width(rows(xyz=None, flag=None)) == 53
    assert width(rows(L_=1)) == 4 + 4 + 6 + 6 + 1 + 33 and width(rows(L_=8, stride=64, Cc=64)) == 36 + 54 + 1 + 64
    assert width(rows(uv=None, xyz=None, code=None, stride=0, Cc=0)) == 1
    for r in (rows(L_=0), rows(L_=9), rows(Cc=65, stride=65), rows(Cc=-1), rows(stride=32), rows(code=None), rows(Cc=0, stride=0),
              rows(uv=None, xyz=None, flag=None, code=None, stride=0, Cc=0)):
        assert width(r) == bad
    assert L.gh_cond_width(None) == bad
    assert L.gh_cond_fold_bytes(2, 84, 51) == 4 * (51 + 51 * 84 + 2 * (2 + 102))
    for B, Dv, Hd in ((0, 84, 51), (2, 0, 51), (2, 84, 0), (2, 84, 65)):
        assert L.gh_cond_fold_bytes(B, Dv, Hd) == 0
    params = _abi.GhCondParams(*[a] * 6)
    r = rows()
    assert L.gh_cond_rows(C.byref(r), 10, one, 83, None) == L.gh_cond_rows(C.byref(r), 10, None, 84, None) == L.gh_cond_rows(C.byref(r), -1, one, 84, None) == bad
    assert L.gh_cond_rows(C.byref(r), 0, one, 84, None) == _abi.GH_OK

    def fold(e=one, B=2, De=768, Dv=84, Hd=51, p=params, f=one, n=1 << 20):
        return L.gh_cond_fold(e, B, De, Dv, Hd, C.byref(p) if p else None, f, n, None)

    assert fold(e=None) == fold(B=-1) == fold(De=-1) == fold(Dv=0) == fold(Hd=0) == fold(Hd=65) == fold(p=None) == fold(f=None) == bad
    assert fold(p=_abi.GhCondParams(*([a] * 5 + [None]))) == bad and fold(n=16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert fold(B=0) == _abi.GH_OK

    def fwd(r=r, P=64, N=32, De=768, Hd=51, p=params, f=one, eps=1e-6, out=one):
        return L.gh_cond_mlp_forward(C.byref(r), P, N, De, Hd, C.byref(p) if p else None, f, eps, out, None)

    assert fwd(P=-32) == fwd(N=0) == fwd(P=65) == fwd(De=-1) == fwd(Hd=0) == fwd(Hd=65) == fwd(p=None) == fwd(f=None) == fwd(out=None) == bad
    assert fwd(eps=-1.0) == fwd(eps=float("nan")) == fwd(r=rows(L_=9)) == bad
    assert fwd(P=0) == _abi.GH_OK

    def bwd(r=r, P=64, N=32, g=one, dcode=one, stride=33):
        return L.gh_cond_mlp_backward(C.byref(r), P, N, 768, 51, C.byref(params), one, 1e-6, g, dcode, stride, None)

    assert bwd(r=rows(code=None, stride=0, Cc=0)) == bwd(dcode=None) == bwd(stride=32) == bwd(P=65) == bad
    assert bwd(P=0) == bwd(P=0, g=None) == _abi.GH_OK
