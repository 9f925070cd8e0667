"""The fused Gaussian head on the device (include/gh_head.h through guassianhand_amd/gs_head.py) against its plain-torch restatement.

The tolerance is a measurement, not a constant. For every output field and every gradient three things are computed on the same
inputs on the device: the float64 restatement, the float32 torch path (gs_activations over F.linear with autograd) and the kernel.
The kernel passes when, per field,

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

The factor 4 covers a sequential float32 sum of <= 131 terms against rocBLAS's blocked one; the floor covers a 1-2 ulp difference
between expf implementations where torch's own error happens to be near zero. The three errors are printed per field."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
GRADS = ("grad_x", "grad_pts", "grad_weight", "grad_bias")
ROWS = 64                      # _abi.GH_HEAD_ROWS: rows per workgroup


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert _abi.GH_HEAD_ROWS == ROWS
    return torch.device("cuda:0")


def make_inputs(dev, P, Cin=128, width=3, seed=0):
    """Random non-zero W, b = N(0, 0.5^2) with the scaling bias shifted by -5; one cotangent per output field."""
    g = torch.Generator().manual_seed(1000 * seed + P + 7 * Cin + width)
    O = 11 + width
    x = torch.randn(P, Cin, generator=g)
    pts = 0.1 * torch.randn(P, 3, generator=g)
    W = torch.randn(O, Cin, generator=g) / math.sqrt(Cin)
    b = 0.5 * torch.randn(O, generator=g)
    b[3:6] -= 5.0
    cot = {k: torch.randn(P, n, generator=g) for k, n in zip(FIELDS, (3, 3, 4, 1, width))}
    cot["shs"] = cot["shs"].reshape(P, width // 3, 3)
    return [t.to(dev) for t in (x, pts, W, b)], {k: v.to(dev) for k, v in cot.items()}


def run(mode, inputs, cot, kw, used=FIELDS, frozen=False):
    """One forward + backward -> {field: tensor, grad_*: tensor}. mode: 'f64' | 'torch32' | 'kernel'."""
    from guassianhand_amd import gs_head as H
    leaves = [t.detach().clone().requires_grad_(not (frozen and i >= 2)) for i, t in enumerate(inputs)]
    if mode == "f64":
        gm = H._gs_head_ref(*leaves, **kw, acc=torch.float64)
    else:
        gm = H.gs_head(*leaves, **kw, ops="torch" if mode == "torch32" else "fused")
    out = {k: getattr(gm, k).detach() for k in FIELDS}
    loss = sum((getattr(gm, k) * cot[k].to(getattr(gm, k).dtype)).sum() for k in used)
    loss.backward()
    for name, leaf in zip(GRADS, leaves):
        if leaf.requires_grad:
            out[name] = leaf.grad
    return out


def three_way(inputs, cot, kw, used=FIELDS, fields=FIELDS + GRADS, tag=""):
    res = {m: run(m, inputs, cot, kw, used) for m in ("f64", "torch32", "kernel")}
    bad = []
    for k in fields:
        ref, t32, ker = res["f64"][k], res["torch32"][k], res["kernel"][k]
        assert ker.dtype == torch.float32 and ker.shape == ref.shape, (k, ker.shape, ref.shape)
        e_k = float((ker.double() - ref).abs().max()) if ref.numel() else 0.0
        e_t = float((t32.double() - ref).abs().max()) if ref.numel() else 0.0
        m = float(ref.abs().max()) if ref.numel() else 0.0
        print(f"{tag} {k:12s} kernel-f64 {e_k:.3e}  torch32-f64 {e_t:.3e}  max|f64| {m:.3e}")
        if not e_k <= 4 * e_t + 2.0 ** -20 * m:
            bad.append((k, e_k, e_t, m))
    assert not bad, bad
    return res


RGB = dict(shs_width=3, use_rgb=True, xyz_offset=True, restrict_offset=True, clip_scaling=None)
SH3 = dict(shs_width=48, use_rgb=False, xyz_offset=True, restrict_offset=False, clip_scaling=None)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 3 * ROWS + 1, 1000])
def test_wave_and_tile_tails(dev, P):
    inputs, cot = make_inputs(dev, P)
    three_way(inputs, cot, RGB, tag=f"P={P}")


@pytest.mark.parametrize("Cin", [131, 3])
@pytest.mark.parametrize("name,kw", [("rgb", RGB), ("sh3", SH3)])
def test_unaligned_and_tiny_cin(dev, Cin, name, kw):
    inputs, cot = make_inputs(dev, 3 * ROWS + 1, Cin=Cin, width=kw["shs_width"])
    three_way(inputs, cot, kw, tag=f"Cin={Cin} {name}")


@pytest.mark.parametrize("name,kw", [("sh3", SH3), ("no_xyz_offset", {**RGB, "xyz_offset": False}), ("free_offset", {**RGB, "restrict_offset": False})])
def test_head_variants(dev, name, kw):
    inputs, cot = make_inputs(dev, 3 * ROWS + 1, width=kw["shs_width"], seed=1)
    res = three_way(inputs, cot, kw, tag=name)
    if not kw["xyz_offset"]:
        assert torch.equal(res["kernel"]["xyz"], inputs[1]) and float(res["kernel"]["grad_weight"][:3].abs().max()) == 0.0
        assert torch.equal(res["kernel"]["grad_pts"], cot["xyz"])


@pytest.mark.parametrize("Cin,kw", [(128, RGB), (131, RGB), (131, SH3)])
def test_column_window_is_read_in_place_and_matches_the_copy_bitwise(dev, Cin, kw):
    """x = big[:, 5:5+Cin]: row stride > Cin, rows not 16-byte aligned."""
    inputs, cot = make_inputs(dev, 300, Cin=Cin, width=kw["shs_width"], seed=2)
    big = torch.randn(300, Cin + 9, device=dev)
    big[:, 5:5 + Cin] = inputs[0]
    view = big[:, 5:5 + Cin]
    assert view.stride(0) == Cin + 9 and view.data_ptr() % 16 != 0 and not view.is_contiguous()
    a = run("kernel", [view] + inputs[1:], cot, kw)
    c = run("kernel", [view.contiguous()] + inputs[1:], cot, kw)
    for k in FIELDS + GRADS:
        assert torch.equal(a[k], c[k]), k
    three_way([view] + inputs[1:], cot, kw, tag=f"window Cin={Cin}")


def test_clip_scaling_clamps_and_gates_the_gradient(dev):
    kw = {**RGB, "clip_scaling": 0.005}
    inputs, cot = make_inputs(dev, 1000, seed=3)
    inputs[3][3:6] = math.log(0.005)                      # raw scalings on both sides of log(clip)
    res = three_way(inputs, cot, kw, tag="clip")
    raw_s = torch.nn.functional.linear(inputs[0].double(), inputs[2][3:6].double(), inputs[3][3:6].double())
    below, above = raw_s < math.log(0.005) - 1e-4, raw_s > math.log(0.005) + 1e-4
    assert int(below.sum()) > 100 and int(above.sum()) > 100
    s = res["kernel"]["scaling"]
    assert float(s.max()) == float(torch.tensor(0.005, dtype=torch.float32)) and bool((s[above] == s.max()).all()) and bool((s[below] < s.max()).all())
    # the gate: a row above the clamp sends nothing to the scaling head; shut every other path and look at grad_x
    only = {k: (v if k == "scaling" else torch.zeros_like(v)) for k, v in cot.items()}
    gx = run("kernel", inputs, only, kw)["grad_x"]
    rows_all_above, rows_some_below = above.all(dim=1), below.any(dim=1)
    assert float(gx[rows_all_above].abs().max()) == 0.0 and bool((gx[rows_some_below].abs().amax(dim=1) > 0).all())


def test_backward_of_a_large_raw_scaling_uses_exp_15(dev):
    inputs, cot = make_inputs(dev, 200, seed=4)
    inputs[2][3:6] = 0.0
    inputs[3][3:6] = 20.0                                  # raw scaling exactly 20 on every row
    res = three_way(inputs, cot, RGB, tag="raw=20")
    assert bool((res["kernel"]["scaling"] == res["kernel"]["scaling"][0, 0]).all())
    assert abs(float(res["kernel"]["scaling"][0, 0]) / math.exp(20.0) - 1) < 1e-6
    want, scale = cot["scaling"].double().sum(0) * math.exp(15.0), cot["scaling"].double().abs().sum(0) * math.exp(15.0)
    assert float(((res["kernel"]["grad_bias"][3:6].double() - want).abs() / scale).max()) < 1e-4      # exp(15), not exp(20) = 148 x


def test_all_zero_rotation_row_gives_zero_and_no_nan(dev):
    inputs, cot = make_inputs(dev, 130, seed=5)
    inputs[0][77] = 0.0                                    # a zero feature row and a zero rotation bias: raw rotation (0,0,0,0)
    inputs[3][6:10] = 0.0
    cot["rotation"][77] = 0.0                              # (below the floor the gradient is g / 1e-12: keep it out of the sums compared)
    res = three_way(inputs, cot, RGB, tag="zero rotation row")
    assert float(res["kernel"]["rotation"][77].abs().max()) == 0.0
    for k in FIELDS + GRADS:
        assert bool(torch.isfinite(res["kernel"][k]).all()), k
    cot["rotation"][77] = 1.0                              # and with a gradient arriving there: finite, g / 1e-12 on the rotation head
    out = run("kernel", inputs, cot, RGB)
    assert all(bool(torch.isfinite(out[k]).all()) for k in GRADS)
    assert float(out["grad_bias"][6:10].abs().min()) > 1e11


@pytest.fixture(scope="module")
def p1000(dev):
    inputs, cot = make_inputs(dev, 1000, seed=6)
    return inputs, cot, run("kernel", inputs, cot, RGB)


def test_rows_do_not_depend_on_their_neighbours(dev, p1000):
    inputs, cot, full = p1000
    for r in (0, 64, 999):
        one = run("kernel", [inputs[0][r:r + 1], inputs[1][r:r + 1], inputs[2], inputs[3]], {k: v[r:r + 1] for k, v in cot.items()}, RGB)
        for k in FIELDS + ("grad_x", "grad_pts"):
            assert torch.equal(one[k], full[k][r:r + 1]), (r, k)


def test_weight_gradients_are_bitwise_reproducible(dev, p1000):
    inputs, cot, full = p1000
    again = run("kernel", inputs, cot, RGB)
    assert torch.equal(again["grad_weight"], full["grad_weight"]) and torch.equal(again["grad_bias"], full["grad_bias"])
    assert float(full["grad_weight"].abs().min()) > 0


def test_frozen_head_skips_the_reduction_and_changes_nothing_else(dev, p1000):
    inputs, cot, full = p1000
    frozen = run("kernel", inputs, cot, RGB, frozen=True)
    assert "grad_weight" not in frozen and "grad_bias" not in frozen
    assert torch.equal(frozen["grad_x"], full["grad_x"]) and torch.equal(frozen["grad_pts"], full["grad_pts"])
    from guassianhand_amd import gs_head as H
    x, pts, W, b = (t.detach().clone() for t in inputs)
    x.requires_grad_(True)
    gm = H.gs_head(x, pts, W, b, **RGB)
    sum((getattr(gm, k) * cot[k]).sum() for k in FIELDS).backward()
    assert W.grad is None and b.grad is None and pts.grad is None and torch.equal(x.grad, full["grad_x"])


def test_unused_outputs_send_null_cotangents(dev):
    inputs, cot = make_inputs(dev, 257, seed=7)
    res = three_way(inputs, cot, RGB, used=("opacity", "xyz"), tag="opacity+xyz only")
    gw = res["kernel"]["grad_weight"]
    assert float(gw[3:10].abs().max()) == 0.0 and float(gw[11:].abs().max()) == 0.0 and float(gw[10].abs().min()) > 0


def test_no_points(dev):
    from guassianhand_amd import gs_head as H
    inputs, _ = make_inputs(dev, 4)
    x, pts, W, b = inputs
    x0, W0 = x[:0].clone().requires_grad_(True), W.clone().requires_grad_(True)
    gm = H.gs_head(x0, pts[:0], W0, b, **{**SH3, "shs_width": 3})
    assert [tuple(getattr(gm, k).shape) for k in FIELDS] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, 1, 3)]
    assert all(getattr(gm, k).is_cuda for k in FIELDS)
    sum(getattr(gm, k).sum() for k in FIELDS).backward()
    assert tuple(x0.grad.shape) == (0, 128) and float(W0.grad.abs().max()) == 0.0


def test_forward_and_backward_are_graph_capturable(dev, p1000):
    from guassianhand_amd import gs_head as H
    inputs, cot, full = p1000
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]

    def step():
        gm = H.gs_head(*leaves, **RGB)
        loss = sum((getattr(gm, k) * cot[k]).sum() for k in FIELDS)
        return [getattr(gm, k) for k in FIELDS] + list(torch.autograd.grad(loss, leaves))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, o in zip(FIELDS + GRADS, outs):
            assert torch.equal(o, full[k]), k


@pytest.mark.parametrize("use_rgb", [True, False])
def test_fuse_gs_head_end_to_end_through_forward_single_batch(dev, use_rgb):
    """A stand-in renderer whose gs_net is a GSLayer-shaped torch module: forward_single_batch before and after fuse_gs_head —
    the same Gaussians are selected, and the images agree within test_gpu_single_batch.py's image tolerance (1e-4)."""
    from types import SimpleNamespace
    from guassianhand_amd import gs_head as H
    from guassianhand_amd.renderer import forward_single_batch, gs_activations
    from helpers import BatchStandIns, batch_inputs

    st, inp = BatchStandIns(dev, use_rgb=use_rgb), batch_inputs()
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = SimpleNamespace(feature_channels=dict(xyz=3, scaling=3, rotation=4, opacity=1, shs=48), use_rgb=use_rgb,
                                       xyz_offset=True, restrict_offset=True, clip_scaling=None)
            self.out_layers = torch.nn.ModuleList()
            for k in FIELDS:
                lin = torch.nn.Linear(st.C, st.W[k].shape[1])
                with torch.no_grad():
                    lin.weight.copy_(st.W[k].t())
                    lin.bias.fill_(-5.0 if k == "scaling" else 0.0)
                self.out_layers.append(lin)

        def forward(self, x, pts):
            raw = {k: lin(x) for k, lin in zip(FIELDS, self.out_layers)}
            return gs_activations(raw, pts, use_rgb=use_rgb)

    ns = st.namespace(dev)
    ns.gs_net = Net().to(dev)
    ns.forward_gs = lambda x, p: ns.gs_net(x, p)
    call = lambda: forward_single_batch(ns, d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"],
                                        color_w=d["color_w"], xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"],
                                        vert3d_uv=[None], face_uv=None, face_uv_xy=None)
    with torch.no_grad():
        before = call()
        assert H.fuse_gs_head(ns) is ns and type(ns.gs_net) is H.fused_gs_layer_cls(Net)
        after = call()
    assert after["3dgs"].xyz.shape == before["3dgs"].xyz.shape and after["3dgs"].shs.shape == before["3dgs"].shs.shape
    for k in ("comp_rgb", "comp_mask"):
        err = float((after[k] - before[k]).abs().max())
        print(f"{k}: fused vs unfused L_inf {err:.3e}")
        assert err <= 1e-4, (k, err)
    assert float(after["comp_mask"].max()) > 0.5 and float(after["comp_rgb"].std()) > 0.01
    # and with gradients: the fused head passes them on to the features
    feat = d["feat"].clone().requires_grad_(True)
    out = forward_single_batch(ns, feat, d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"], color_w=d["color_w"],
                               xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"], vert3d_uv=[None])
    out["comp_rgb"].square().mean().backward()
    assert bool(torch.isfinite(feat.grad).all()) and float(feat.grad.abs().max()) > 0
