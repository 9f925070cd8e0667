"""The fused Gaussian trunk on the device (include/gh_trunk.h through guassianhand_amd/gs_trunk.py) against its plain-torch restatement.

The tolerance is a measurement, not a constant (tests/res_block_cases.three_way). For every output field and every gradient three
things are computed on the same inputs on the device: the float64 restatement, the float32 torch path (three F.linear, the
activations and gs_activations with autograd) and the kernels. The kernels pass when, per field,

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

The three errors are printed per field. Shapes: tests/gs_trunk_cases.py."""
from types import SimpleNamespace

import pytest
import torch

from tests import gs_trunk_cases as G
from tests.res_block_cases import three_way

pytestmark = pytest.mark.gpu

R = G.R
FIELDS, OUT = G.FIELDS, G.OUT
BIG = (2 * R + 1, 131, 128, 128, 3, "silu", True, None, 0)              # the flagship sizes over three tiles, one row in the last


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert _abi.GH_TRUNK_ROWS == R
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def big(dev):
    c = G.make(BIG, dev)
    return c, G.run(c, "kernel")


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_three_way(dev, case):
    c = G.make(case, dev)
    G.assert_margins(c, G.case_id(case))
    res = {m: G.run(c, m) for m in ("kernel", "torch32", "f64")}
    for k in OUT:
        assert res["kernel"][k].dtype == torch.float32 and res["kernel"][k].shape == res["f64"][k].shape, k
    three_way(res["kernel"], res["torch32"], res["f64"], fields=OUT, tag=G.case_id(case))
    if case[7] is not None:                                               # the clamp acts, and it gates the gradient
        s = res["kernel"]["scaling"]
        assert float(s.max()) == pytest.approx(case[7]) and float(s.min()) < case[7]


@pytest.mark.parametrize("off", [5, 4])
def test_column_window_is_read_in_place_and_matches_the_copy_bitwise(dev, off):
    """x = wide[:, off:off + 131]: row stride > Cin; at the odd offset no row is 16-byte aligned."""
    c = G.make(BIG, dev)
    wide = torch.randn(c.x.shape[0], 131 + 9, device=dev)
    wide[:, off:off + 131] = c.x
    view = wide[:, off:off + 131]
    assert view.stride(0) == 140 and not view.is_contiguous() and (view.data_ptr() % 16 != 0) == (off == 5)
    a, b = G.run(c, "kernel", x=view), G.run(c, "kernel", x=view.contiguous())
    for k in OUT:
        assert torch.equal(a[k], b[k]), k


def _forward_raw(c, x, pts):
    """The kernels called directly (the five outputs, raw, grad_x) for rows the caller picks."""
    from guassianhand_amd.gs_trunk import _GsTrunkFn
    xl = x.detach().requires_grad_(True)
    cfg = (c.kw["shs_width"], c.kw["use_rgb"], True, c.kw["restrict_offset"], c.kw["clip_scaling"])
    outs = _GsTrunkFn.apply(xl, pts, cfg, c.kw["activation"], *c.trunk, c.Wh, c.bh)
    raw = outs[0].grad_fn.saved_tensors[1]
    return outs, raw, xl


def test_rows_do_not_depend_on_their_neighbours(dev, big):
    """Row 70 of the (2R + 1)-row call, the same row alone at another stride, and as the last row of a 33-row call: outputs, raw and
    grad_x bit for bit."""
    c, _ = big
    cot = [c.cot[k].reshape(c.cot[k].shape[0], -1) for k in FIELDS]

    def rows(sel, x):
        outs, raw, xl = _forward_raw(c, x, c.pts[sel].contiguous())
        torch.autograd.backward(outs, [g[sel].contiguous() for g in cot])
        return [o.detach() for o in outs] + [raw, xl.grad]

    full = rows(slice(None), c.x)
    pad = torch.zeros(1, 200, device=dev)
    pad[:, 7:138] = c.x[70]
    alone = rows(slice(70, 71), pad[:, 7:138])
    last = rows(slice(38, 71), c.x[38:71])
    for name, f, a, l in zip(FIELDS + ("raw", "grad_x"), full, alone, last):
        assert torch.equal(f[70:71], a), name
        assert torch.equal(f[70:71], l[32:33]), name


def test_two_runs_are_bitwise_identical(dev, big):
    c, first = big
    again = G.run(c, "kernel")
    for k in OUT:
        assert torch.equal(first[k], again[k]), k


def test_identity_trunk_agrees_with_gs_head(dev):
    """W1 = [I | 0], W2 = W3 = I, zero biases, ReLU and positive inputs: the trunk hands x[:, :128] to its head unchanged, and its
    outputs, grad_x and grad_pts are held to the float64 head under the three-way rule with gs_head's kernels in the float32 slot."""
    from guassianhand_amd import gs_head as H
    c = G.make((2 * R + 1, 131, 128, 128, 3, "relu", True, None, 0), dev)
    eye, zero = torch.eye(128, device=dev), torch.zeros(128, device=dev)
    c.trunk = [torch.cat([eye, torch.zeros(128, 3, device=dev)], dim=1).contiguous(), zero, eye, zero, eye, zero]
    c.x = c.x.abs() + 0.01
    kw = {k: v for k, v in c.kw.items() if k != "activation"}

    def head(mode):
        xl, pl = c.x[:, :128].detach().requires_grad_(True), c.pts.detach().clone().requires_grad_(True)
        gm = H._gs_head_ref(xl, pl, c.Wh, c.bh, acc=torch.float64, **kw) if mode == "f64" else H.gs_head(xl, pl, c.Wh, c.bh, **kw)
        out = {k: getattr(gm, k).detach() for k in FIELDS}
        sum((getattr(gm, k) * c.cot[k].to(getattr(gm, k).dtype)).sum() for k in FIELDS).backward()
        out["grad_x"], out["grad_pts"] = xl.grad, pl.grad
        return out

    trunk = G.run(c, "kernel")
    assert float(trunk["grad_x"][:, 128:].abs().max()) == 0.0
    trunk["grad_x"] = trunk["grad_x"][:, :128]
    three_way(trunk, head("kernel"), head("f64"), fields=OUT, tag="identity trunk vs gs_head")


@pytest.mark.parametrize("only", FIELDS)
def test_one_cotangent_alone_the_others_null(dev, only):
    c = G.make((R + 1, 131, 128, 128, 3, "silu", True, None, 0), dev)
    res = {m: G.run(c, m, used=(only,)) for m in ("kernel", "torch32", "f64")}
    three_way(res["kernel"], res["torch32"], res["f64"], fields=("grad_x", "grad_pts"), tag=f"only {only}")
    assert (float(res["kernel"]["grad_pts"].abs().max()) > 0) == (only == "xyz")
    assert float(res["kernel"]["grad_x"].abs().max()) > 0


def test_zero_cotangents_give_zero_gradients(dev):
    c = G.make((R + 1, 131, 128, 128, 48, "silu", False, None, 0), dev)
    c.cot = {k: torch.zeros_like(v) for k, v in c.cot.items()}
    out = G.run(c, "kernel")
    assert float(out["grad_x"].abs().max()) == 0.0 and float(out["grad_pts"].abs().max()) == 0.0


def test_no_points(dev):
    from guassianhand_amd import gs_trunk as T
    c = G.make((4, 131, 128, 128, 3, "silu", True, None, 0), dev)
    x0 = c.x[:0].clone().requires_grad_(True)
    gm = T.gs_trunk(x0, c.pts[:0], c.trunk, c.Wh, c.bh, **c.kw)
    assert [tuple(getattr(gm, k).shape) for k in FIELDS] == [(0, 3), (0, 3), (0, 4), (0, 1), (0, 1, 3)]
    assert all(getattr(gm, k).is_cuda for k in FIELDS)
    sum(getattr(gm, k).sum() for k in FIELDS).backward()
    assert tuple(x0.grad.shape) == (0, 131)


def test_backward_of_a_large_raw_scaling_uses_exp_15(dev):
    """Raw scalings around 20: the forward is exp(v), the backward multiplies by exp(min(v, 15)) — as the float64 restatement does."""
    c = G.make((R + 1, 131, 128, 128, 3, "silu", True, None, 0), dev)
    c.bh[3:6] = 20.0
    c.Wh[3:6] *= 0.1
    res = {m: G.run(c, m, used=("scaling",)) for m in ("kernel", "torch32", "f64")}
    raw = torch.log(res["f64"]["scaling"])
    assert float(raw.min()) > 15.5
    three_way(res["kernel"], res["torch32"], res["f64"], fields=("scaling", "grad_x"), tag="raw scaling 20")
    ratio = res["kernel"]["grad_x"].double().abs().max() / res["f64"]["grad_x"].abs().max()
    assert 0.99 < float(ratio) < 1.01                                      # (exp(20) in the backward would be 148 times too much)


def test_all_zero_rotation_row_gives_zero_and_no_nan(dev):
    c = G.make((R + 1, 131, 128, 128, 3, "silu", True, None, 0), dev)
    c.Wh[6:10] = 0.0
    c.bh[6:10] = 0.0
    out = G.run(c, "kernel")
    assert float(out["rotation"].abs().max()) == 0.0
    assert all(bool(torch.isfinite(out[k]).all()) for k in OUT)
    ref = G.run(c, "f64")
    three_way(out, G.run(c, "torch32"), ref, fields=OUT, tag="zero rotation")


def test_forward_and_backward_are_graph_capturable(dev, big):
    from guassianhand_amd import gs_trunk as T
    c, eager = big
    xl, pl = c.x.detach().clone().requires_grad_(True), c.pts.detach().clone().requires_grad_(True)

    def step():
        gm = T.gs_trunk(xl, pl, c.trunk, c.Wh, c.bh, **c.kw)
        loss = sum((getattr(gm, k) * c.cot[k]).sum() for k in FIELDS)
        return [getattr(gm, k) for k in FIELDS] + list(torch.autograd.grad(loss, [xl, pl]))

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
        for k, o in zip(OUT, outs):
            assert torch.equal(o, eager[k]), k


def test_kernel_path_refuses_a_trainable_weight(dev):
    from guassianhand_amd import gs_trunk as T
    c = G.make((4, 131, 128, 128, 3, "silu", True, None, 0), dev)
    c.trunk[2] = c.trunk[2].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no gradient of a weight"):
        T.gs_trunk(c.x, c.pts, c.trunk, c.Wh, c.bh, **c.kw)
    with torch.no_grad():
        T.gs_trunk(c.x, c.pts, c.trunk, c.Wh, c.bh, **c.kw)
    with pytest.raises(ValueError, match="kernels take"):
        T.gs_trunk(torch.zeros(4, 193, device=dev), c.pts, [torch.zeros(128, 193, device=dev)] + c.trunk[1:], c.Wh, c.bh, **c.kw)


# ---- through forward_single_batch --------------------------------------------------------------------------------------------------
class _StandIn(SimpleNamespace):
    """What forward_single_batch reads of the renderer (tests/helpers.BatchStandIns.namespace), with the reference's forward_gs."""

    def forward_gs(self, x, p):
        if self.cfg.mlp_network_config is not None:
            x = self.mlp_net(x)
        return self.gs_net(x, p)


@pytest.mark.parametrize("use_rgb", [True, False])
def test_fuse_forward_gs_end_to_end_through_forward_single_batch(dev, use_rgb, monkeypatch):
    """A stand-in renderer with a real TrunkMLP in front of a GSLayer-shaped torch head, N = 400 points, run through
    forward_single_batch: the images and the gradient of the features after fuse_forward_gs against the unfused float32 forward_gs,
    both held to the run whose forward_gs computes in float64 (rounded once to float32) under the three-way rule. With a trainable
    trunk the same object takes the torch path and every parameter gets a gradient."""
    from guassianhand_amd import gs_head as H
    from guassianhand_amd import gs_trunk as T
    from guassianhand_amd.renderer import GaussianModel, forward_single_batch, gs_activations
    from helpers import BatchStandIns, batch_inputs

    st, inp = BatchStandIns(dev, use_rgb=use_rgb), batch_inputs()
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    widths = dict(xyz=3, scaling=3, rotation=4, opacity=1, shs=3 if use_rgb else 48)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = SimpleNamespace(feature_channels=dict(xyz=3, scaling=3, rotation=4, opacity=1, shs=48), use_rgb=use_rgb,
                                       xyz_offset=True, restrict_offset=True, clip_scaling=None)
            gen = torch.Generator().manual_seed(21)
            self.out_layers = torch.nn.ModuleList()
            for k in FIELDS:
                lin = torch.nn.Linear(32, widths[k])
                with torch.no_grad():
                    lin.weight.copy_(0.4 * torch.randn(widths[k], 32, generator=gen) * (3.0 if k == "opacity" else 1.0))
                    lin.bias.fill_(-5.0 if k == "scaling" else 0.0)
                self.out_layers.append(lin)

        def forward(self, x, pts):
            raw = {k: lin(x) for k, lin in zip(FIELDS, self.out_layers)}
            return gs_activations(raw, pts, use_rgb=use_rgb)

    torch.manual_seed(17)
    mlp = T.TrunkMLP(st.C, 32, 32, 2, "silu").to(dev).requires_grad_(False)

    def renderer(fuse_head=False):
        attrs = vars(st.namespace(dev))
        del attrs["forward_gs"]
        r = _StandIn(**attrs)
        r.cfg.mlp_network_config = dict(n_neurons=32, n_hidden_layers=2, activation="silu")
        r.mlp_net, r.gs_net = mlp, Net().to(dev).requires_grad_(False)      # (every Net carries the same weights: a seeded generator)
        return H.fuse_gs_head(r) if fuse_head else r

    def call(r):
        feat = d["feat"].clone().requires_grad_(True)
        out = forward_single_batch(r, feat, d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"], color_w=d["color_w"],
                                   xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"], vert3d_uv=[None], face_uv=None,
                                   face_uv_xy=None)
        out["comp_rgb"].square().mean().backward()
        return dict(comp_rgb=out["comp_rgb"].detach(), comp_mask=out["comp_mask"].detach(), grad_feat=feat.grad), out["3dgs"]

    calls = []
    real = T.gs_trunk
    monkeypatch.setattr(T, "gs_trunk", lambda x, *a, **kw: (calls.append(tuple(x.shape)), real(x, *a, **kw))[1])

    unfused = renderer()
    assert T.kernel_args(unfused, d["feat"], d["pts"]) is None             # a head with a forward of its own keeps it
    i32, gs32 = call(unfused)
    fused = renderer(fuse_head=True)                                       # what the ...Trunk config strings do: the head, then forward_gs
    assert T.fuse_forward_gs(fused) is fused and type(fused) is T.fused_forward_gs_cls(_StandIn)
    args = T.kernel_args(fused, d["feat"], d["pts"])
    assert args is not None

    def forward_gs64(x, p):
        trunk, W, b, kw = args
        gm = T._gs_trunk_ref(x, p, trunk, W, b, acc=torch.float64, **kw)
        return GaussianModel(*[t.float() for t in gm])

    r64 = renderer()
    r64.forward_gs = forward_gs64                                          # (an instance attribute: it goes ahead of the class's method)
    i64, _ = call(r64)
    assert calls == []
    ik, gsk = call(fused)
    assert len(calls) == 1 and calls[0][1] == st.C and calls[0][0] == gsk.xyz.shape[0]      # the kernels ran, once, over every row
    assert gsk.xyz.shape == gs32.xyz.shape and gsk.shs.shape == gs32.shs.shape
    three_way(ik, i32, i64, fields=("comp_rgb", "comp_mask", "grad_feat"), tag=f"seam use_rgb={use_rgb}")
    assert float(ik["comp_mask"].max()) > 0.5 and float(ik["comp_rgb"].std()) > 0.01 and float(ik["grad_feat"].abs().max()) > 0
    # a trainable trunk: the same fused object takes the torch path — mlp_net in torch, then the fused head, bit for bit what the
    # renderer with the fused head alone gives — and every parameter has a gradient
    mlp.requires_grad_(True)
    try:
        assert T.kernel_args(fused, d["feat"], d["pts"]) is None
        it, _ = call(fused)
        assert len(calls) == 1
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in mlp.parameters())
        ih, _ = call(renderer(fuse_head=True))
        assert torch.equal(it["comp_rgb"], ih["comp_rgb"])
    finally:
        mlp.requires_grad_(False)
