"""The fused vertex MLP block on the device (include/gh_vert.h through guassianhand_amd/vert_mlp.py) against its plain-torch restatement.

The tolerance is a measurement, not a constant. For the output and every gradient three things are computed on the same inputs on the
device: the float64 restatement, the float32 torch path (F.layer_norm and F.linear over torch.cat, with autograd) and the kernel. The
kernel passes when, per field,

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

The factor 4 is the Gaussian head's and covers a different split of the 134-term sums; the floor covers a 1-2 ulp difference between
expf / tanhf implementations where torch's own error happens to be near zero. The three errors are printed per field."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.vert_cases import ACT, make_inputs, names, run

pytestmark = pytest.mark.gpu

ROWS = 64                      # _abi.GH_VERT_ROWS: rows per workgroup


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert _abi.GH_VERT_ROWS == ROWS
    return torch.device("cuda:0")


def check(res, fields, tag=""):
    bad = []
    for k in fields:
        ref, t32, ker = res["f64"][k], res["torch32"][k], res["kernel"][k]
        assert ker.dtype == torch.float32 and ker.shape == ref.shape, (k, ker.shape, ref.shape)
        e_k = float((ker.double() - ref).abs().max()) if ref.numel() else 0.0
        e_t = float((t32.double() - ref).abs().max()) if ref.numel() else 0.0
        m = float(ref.abs().max()) if ref.numel() else 0.0
        print(f"{tag} {k:16s} kernel-f64 {e_k:.3e}  torch32-f64 {e_t:.3e}  max|f64| {m:.3e}  ratio {e_k / e_t if e_t else float('inf'):.2f}")
        if not e_k <= 4 * e_t + 2.0 ** -20 * m:
            bad.append((k, e_k, e_t, m))
    assert not bad, bad


def three_way(inputs, cot, K, tag=""):
    res = {m: run(m, inputs, cot, K) for m in ("f64", "torch32", "kernel")}
    check(res, ("out",) + names(), tag)
    return res


# P: wave and tile tails; Cf: 131 (the reference's), 128 (16-byte loads), 5 (Hd = 2), 1 (Hd = 1), 164 / 165 (the last width whose backward
# holds 64 rows per workgroup and the first that holds 32) and 256 (the widest)
SHAPES = [(P, 131) for P in (1, 63, 64, 65, 257)] + [(257, Cf) for Cf in (128, 5, 1)] + [(65, Cf) for Cf in (164, 165, 256)]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("P,Cf", SHAPES)
def test_shapes_and_modes(dev, P, Cf, K):
    inputs, cot = make_inputs(dev, P, Cf, K)
    three_way(inputs, cot, K, tag=f"P={P} Cf={Cf} K={K}")


@pytest.mark.parametrize("K", [1, 3])
def test_no_points(dev, K):
    """P = 0: shapes, devices and zero parameter gradients, without a launch."""
    from guassianhand_amd import vert_mlp as V
    inputs, _ = make_inputs(dev, 4, 131, K)
    x0, p0 = inputs[0][:0].clone().requires_grad_(True), inputs[1][:0].clone().requires_grad_(True)
    params = [t.clone().requires_grad_(True) for t in inputs[2:]]
    out = V.vert_block(x0, p0, params, act=ACT[K])
    assert tuple(out.shape) == (0, K) and out.is_cuda
    out.sum().backward()
    assert tuple(x0.grad.shape) == (0, 131) and tuple(p0.grad.shape) == (0, 3)
    assert all(float(p.grad.abs().max()) == 0.0 for p in params)


@pytest.mark.parametrize("K", [1, 3])
def test_constant_row(dev, K):
    """Every feature and coordinate of row 70 is 0.5: mean and variance are exact (0.5 and 0), rstd = 1 / sqrt(eps), the normalised row
    is zero and the output is what the LayerNorm's bias alone gives."""
    from guassianhand_amd import vert_mlp as V
    inputs, cot = make_inputs(dev, 130, 131, K, seed=1)
    inputs[0][70] = 0.5
    inputs[1][70] = 0.5
    res = three_way(inputs, cot, K, tag=f"constant row K={K}")
    beta = inputs[3].double()
    o = torch.nn.functional.linear(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(beta, inputs[4].double(), inputs[5].double())),
                                                              inputs[6].double(), inputs[7].double()), inputs[8].double(), inputs[9].double())
    want = torch.sigmoid(o) if K == 1 else 0.5 + torch.tanh(o) * 0.001
    got = res["kernel"]["out"][70]
    assert bool(torch.isfinite(got).all())
    assert float((got.double() - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max()) + 4 * float((res["torch32"]["out"][70].double() - want).abs().max())
    for k in ("grad_x", "grad_pts"):                              # the row's own gradient, against float64, under the same bound
        ref, t32, ker = (res[m][k][70] for m in ("f64", "torch32", "kernel"))
        assert bool(torch.isfinite(ker).all())
        e_k, e_t = float((ker.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
        print(f"constant row K={K} {k} kernel-f64 {e_k:.3e} torch32-f64 {e_t:.3e} max|f64| {float(ref.abs().max()):.3e}")
        assert e_k <= 4 * e_t + 2.0 ** -20 * float(res["f64"][k].abs().max())


def test_nan_in_one_feature_stays_in_its_row(dev):
    from guassianhand_amd import vert_mlp as V
    inputs, cot = make_inputs(dev, 257, 131, 1, seed=2)
    clean = run("kernel", inputs, cot, 1)
    dirty_in = [t.clone() for t in inputs]
    dirty_in[0][130, 17] = float("nan")
    dirty = run("kernel", dirty_in, cot, 1, frozen=True)
    s = dirty["out"][:, 0]
    assert bool(torch.isnan(s[130]))
    keep = torch.arange(257, device=dev) != 130
    assert torch.equal(s[keep], clean["out"][keep, 0])
    assert torch.equal(dirty["grad_x"][keep], clean["grad_x"][keep]) and torch.equal(dirty["grad_pts"][keep], clean["grad_pts"][keep])
    assert not bool((s > 0.1)[130]) and not bool((s > 0.9)[130])                     # selected at neither threshold
    from guassianhand_amd.renderer import select_gaussians
    pv, fv, pc, fc = select_gaussians(s, dirty_in[1], dirty_in[0], 0.1, 0.9)
    assert pv.shape[0] == int((clean["out"][keep, 0] > 0.1).sum()) and pc.shape[0] == int((clean["out"][keep, 0] > 0.9).sum())
    assert bool(torch.isfinite(fv).all()) and bool(torch.isfinite(fc).all())


@pytest.fixture(scope="module")
def p257(dev):
    inputs, cot = make_inputs(dev, 257, 131, 3, seed=3)
    return inputs, cot, run("kernel", inputs, cot, 3)


@pytest.mark.parametrize("K", [1, 3])
def test_row_130_alone_is_bitwise_the_same(dev, K):
    inputs, cot = make_inputs(dev, 257, 131, K, seed=4)
    full = run("kernel", inputs, cot, K)
    one = run("kernel", [inputs[0][130:131], inputs[1][130:131]] + inputs[2:], cot[130:131], K)
    for k in ("out", "grad_x", "grad_pts"):
        assert torch.equal(one[k], full[k][130:131]), k


@pytest.mark.parametrize("Cf", [131, 128])
def test_column_window_is_read_in_place_and_matches_the_copy_bitwise(dev, Cf):
    """x = big[:, 5:5+Cf]: row stride > Cf, rows not 16-byte aligned."""
    inputs, cot = make_inputs(dev, 257, Cf, 3, seed=5)
    big = torch.randn(257, Cf + 9, device=dev)
    big[:, 5:5 + Cf] = inputs[0]
    view = big[:, 5:5 + Cf]
    assert view.stride(0) == Cf + 9 and view.data_ptr() % 16 != 0 and not view.is_contiguous()
    a = run("kernel", [view] + inputs[1:], cot, 3)
    c = run("kernel", [view.contiguous()] + inputs[1:], cot, 3)
    for k in ("out",) + names():
        assert torch.equal(a[k], c[k]), k


def test_parameter_gradients_are_bitwise_reproducible(dev, p257):
    inputs, cot, full = p257
    again = run("kernel", inputs, cot, 3)
    for k in names():
        assert torch.equal(again[k], full[k]), k
    assert all(float(full[k].abs().max()) > 0 for k in names())


def test_frozen_backward_is_the_same_grad_x_and_no_parameter_gradients(dev, p257):
    from guassianhand_amd import vert_mlp as V
    inputs, cot, full = p257
    frozen = run("kernel", inputs, cot, 3, frozen=True)
    assert sorted(frozen) == ["grad_pts", "grad_x", "out"]
    assert torch.equal(frozen["grad_x"], full["grad_x"]) and torch.equal(frozen["grad_pts"], full["grad_pts"])
    x = inputs[0].clone().requires_grad_(True)
    (V.vert_block(x, inputs[1], inputs[2:], act="tanh_offset") * cot).sum().backward()
    assert torch.equal(x.grad, full["grad_x"]) and all(t.grad is None for t in inputs[1:])


def test_null_cotangent_writes_zeros(dev, p257):
    """gh_vert_backward with g_out = NULL: every gradient is written, as zero, frozen and trainable."""
    from guassianhand_amd import _abi, _call
    inputs, _, _ = p257
    x, pts, params = inputs[0], inputs[1], inputs[2:]
    L = _call.lib()
    desc = _abi.GhVertDesc(3, _abi.GH_VERT_ACT_TANH_OFFSET, 0.001, 1e-6)
    ps = _call.struct(_abi.GhVertParams, params)
    ptr, stream = _call.ptr, _call.stream(dev)
    for trainable in (False, True):
        gx, gp = torch.full_like(x, 7.0), torch.full_like(pts, 7.0)
        grads = [torch.full_like(p, 7.0) for p in params]
        gs = _call.struct(_abi.GhVertGrads, grads)
        n = int(L.gh_vert_workspace_bytes(257, 134, 33, 3))
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = L.gh_vert_backward(ptr(x), 131, ptr(pts), 257, 131, C.byref(ps), C.byref(desc), None, ptr(gx), 131, ptr(gp),
                                C.byref(gs) if trainable else None, ptr(ws) if trainable else None, n if trainable else 0, stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert float(gx.abs().max()) == 0.0 and float(gp.abs().max()) == 0.0
        assert all(float(g.abs().max()) == (0.0 if trainable else 7.0) for g in grads)


def test_forward_and_backward_are_graph_capturable(dev, p257):
    """Forward and backward captured in one graph on a single stream, replayed once, equal to the eager result."""
    from guassianhand_amd import vert_mlp as V
    inputs, cot, full = p257
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]

    def step():
        out = V.vert_block(leaves[0], leaves[1], leaves[2:], act="tanh_offset")
        return [out] + list(torch.autograd.grad((out * cot).sum(), leaves))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, o in zip(("out",) + names(), outs):
        assert torch.equal(o, full[k]), k


# ---- through forward_single_batch --------------------------------------------------------------------------------------------------
class _RefShaped(torch.nn.Module):
    """A module shaped like the reference's vert_valid / vert_pos_refinement (ff.layer_norm, ff.fc1, ff.fc2, ff.dropout1/2, fc) whose forward
    is plain torch in `dtype`, returned as float32; `nudge` is added to the refinement's output (a position perturbation)."""

    def __init__(self, Cf, K, params, dtype=torch.float32, nudge=None):
        super().__init__()
        from guassianhand_amd import vert_mlp as V
        self.verts_f_dim, self.detach, self.radius, self.dtype, self.nudge = Cf, False, 0.001, dtype, nudge
        self.ff = V._MLPBlock(Cf + 3, (Cf + 3) // 4)
        self.fc = torch.nn.Linear((Cf + 3) // 4, K)
        with torch.no_grad():
            for dst, src in zip(V._module_params(self), params):
                dst.copy_(src)

    def forward(self, f, p):
        from guassianhand_amd import vert_mlp as V
        out = V._vert_block_ref(f, p, V._module_params(self), act=ACT[self.fc.out_features], radius=self.radius,
                                acc=None if self.dtype == torch.float32 else self.dtype).float()
        return out if self.nudge is None else out + self.nudge[:out.shape[0]]


def test_fuse_vert_mlps_end_to_end_through_forward_single_batch(dev, golden_dir):
    """The fixture's 64 rows and parameters, 2 views of 32 x 32, forward_single_batch before and after fuse_vert_mlps. The same rows are
    selected. The images are held to the block's own bound carried through the unfused run: with I64 the image of the run whose two
    modules compute in float64 (rounded once to float32), I32 that of the float32 torch modules, and Id that of the float64 run with
    every refined coordinate moved by 2^-20 * max|position| (random signs) — the floor of the bound, as a position error —

        max|I_fused - I64|  <=  4 * max|I32 - I64|  +  max|Id - I64|  +  2^-20 * max|I64|"""
    from types import SimpleNamespace
    from guassianhand_amd import vert_mlp as V
    from guassianhand_amd.renderer import forward_single_batch
    from helpers import BatchStandIns, batch_inputs
    from test_vert_mlp_cpu import fixture_case

    fx = np.load(os.path.join(golden_dir, "vert_mlp_fixture.npz"), allow_pickle=False)
    x, pts, pv, _ = (t for t in fixture_case(fx, "v"))
    _, _, pr, _ = fixture_case(fx, "r")
    x, pts, pv, pr = x.to(dev), pts.to(dev), [t.to(dev) for t in pv], [t.to(dev) for t in pr]
    st, inp = BatchStandIns(dev, use_rgb=True), batch_inputs(N=64, n_views=2, H=32, W=32)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}

    def renderer(dtype=torch.float32, nudge=None):
        ns = st.namespace(dev)
        ns.gs_valid = _RefShaped(131, 1, pv, dtype).to(dev).eval()
        ns.vert_pos_refinement = _RefShaped(131, 3, pr, dtype, nudge).to(dev).eval()
        ns.forward_gs = lambda f, p: st.forward_gs(0.2 * f[:, :st.C] + 0.5, p)
        return ns

    def call(ns):
        with torch.no_grad():
            return forward_single_batch(ns, x, pts, d["w2cs"], d["Ks"], 32, 32, 0.71, 1.42, d["bg"], color_w=d["color_w"], xyz_b=d["xyz_b"],
                                        color_b=None, opacity_b=None, vert3d_uv=[None], face_uv=None, face_uv_xy=None)

    ns32 = renderer()
    with torch.no_grad():
        s32 = ns32.gs_valid(x, pts)[:, 0]
    margin = float(torch.minimum((s32 - 0.1).abs(), (s32 - 0.9).abs()).min())
    print(f"torch32 scores on the device: closest to a threshold {margin:.3e}")
    assert margin >= 1e-3, margin                                   # the fixture's condition, on this device's float32 scores
    i32 = call(ns32)
    i64 = call(renderer(torch.float64))
    g = torch.Generator().manual_seed(9)
    delta = 2.0 ** -20 * float(pts.abs().max())
    nudge = (delta * (2.0 * torch.randint(0, 2, (64, 3), generator=g).float() - 1.0)).to(dev)
    idel = call(renderer(torch.float64, nudge))

    fused = renderer()
    mods = (fused.gs_valid, fused.vert_pos_refinement)
    assert V.fuse_vert_mlps(fused) is fused and (fused.gs_valid, fused.vert_pos_refinement) == mods
    assert all(type(m) is V.fused_vert_cls(_RefShaped) for m in mods)
    with torch.no_grad():
        sk = fused.gs_valid(x, pts)[:, 0]
    for t in (0.1, 0.9):
        assert torch.equal(sk > t, s32 > t), t                      # identical selected rows
    assert 8 <= int((sk > 0.9).sum()) < int((sk > 0.1).sum()) <= 56
    ik = call(fused)
    assert ik["3dgs"].xyz.shape == i32["3dgs"].xyz.shape == (int((sk > 0.1).sum()) + int((sk > 0.9).sum()), 3)
    for k in ("comp_rgb", "comp_mask"):
        ref = i64[k].double()
        e_k, e_t, e_d = (float((i[k].double() - ref).abs().max()) for i in (ik, i32, idel))
        print(f"{k}: fused-I64 {e_k:.3e}  I32-I64 {e_t:.3e}  Id-I64 {e_d:.3e}  max|I64| {float(ref.abs().max()):.3e}")
        assert e_k <= 4 * e_t + e_d + 2.0 ** -20 * float(ref.abs().max()), (k, e_k, e_t, e_d)
    assert float(ik["comp_mask"].max()) > 0.1 and float(ik["comp_rgb"].std()) > 0.001       # (something was rendered)
