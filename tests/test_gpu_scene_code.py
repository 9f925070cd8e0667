"""The texture scene code on the device (include/gh_scene.h through guassianhand_amd/scene_code.py).

The fixture captured from the reference lies on exact grids: the kernels reproduce it bit for bit, in both layouts. For random float
inputs the criterion, per field, printed with its three errors:

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * scale

f64 is scene_code_ref with acc=torch.float64, torch32 is scene_code_ref in float32, both on the device. scale is the largest sum of
absolute terms of the field: the same formula run in float64 on |x|, |W|, |b|, |pb| (out) or on |W|, |g| (the gradients). The
additive term is about 6 times the float32 matrix instruction's measured chain error (<= 1.5e-7 sum|a b| for K <= 1024); it is there
because torch32 - f64 can be exactly 0 at Ci = 1.

Shapes (B, Ci, Co, Np, S) are where tiles and tails can go wrong: one of everything; exactly one 32-token tile and one 32-row tile;
36 tokens and 36 rows; three planes of 25 tokens across two batch elements; both limits; the config's shape at B = 1 and 3.
Bitwise properties (a batch element alone, the pair and its sum, the two layouts, inputs read in place, run to run, graph replay, the
bias-only backward) are asserted as equalities."""
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import plane
from guassianhand_amd import scene_code as SC
from tests.scene_code_cases import PlainUpsample, bound, load_fixture, make_inputs, make_module, run, scales, to_planes
from tests.self_attn_cases import errors

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (1, 2, 1, 2, 1), (2, 33, 7, 2, 3), (1, 64, 8, 2, 4), (1, 65, 9, 1, 6), (2, 96, 80, 3, 5), (1, 1024, 128, 1, 2),
          (1, 512, 80, 2, 32), (3, 512, 80, 2, 32)]
FIELDS = ("out", "d_tokens", "d_plane_bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def launches(monkeypatch):
    """(name, arguments) of every entry point scene_code.py calls, in order."""
    calls, real = [], SC.launch

    def spy(name, *a, **k):
        calls.append((name, a))
        return real(name, *a, **k)

    monkeypatch.setattr(SC, "launch", spy)
    return calls


_runs = {}


def case(dev, dims):
    """(module, inputs, kernel result) for one shape, computed once and left unchanged."""
    if dims not in _runs:
        m, inp = make_module(dims, dev=dev), make_inputs(dims, dev=dev)
        _runs[dims] = (m, inp, run("kernel", m, *inp))
    return _runs[dims]


def fields(r):
    out, da, db, dpb = r
    if da is not None and db is not None:
        assert torch.equal(da, db)                                     # the same tensor for both tokens
    return {"out": out, "d_tokens": da, "d_plane_bias": dpb}


def check(label, got, t32, f64, sc):
    bad = []
    for name in FIELDS:
        g, y, r = fields(got)[name], fields(t32)[name], fields(f64)[name]
        assert g.dtype == torch.float32 and g.shape == r.shape and bool(torch.isfinite(g).all()), name
        errors(f"{label} {name}", g, r, y, bound(sc[name]), bad)
    assert not bad, bad


# ---- the reference's recorded values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_cases_bit_for_bit_in_both_layouts(dev, golden_dir, tag):
    c = load_fixture(golden_dir)[0][tag]
    B, Ci, Co, Np, S = c.dims
    m = c.module.to(dev)
    a, b, pb, cot = (t.to(dev) for t in (c.a, c.b, c.pb, c.cot))
    out, da, db, dpb = run("kernel", m, a, b, pb, cot)
    assert torch.equal(out.cpu(), c.out) and torch.equal(da.cpu(), c.d_tokens) and torch.equal(db.cpu(), c.d_tokens)
    assert dpb.shape == c.pb.shape and torch.equal(dpb.cpu(), c.d_plane_bias)
    # the per-plane layout: the module's forward on detokenize's view; the plane bias is added outside
    la, lb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    up = m((la + lb).view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4))
    want = to_planes(c.out - torch.cat([c.pb[..., :2 * S]] * Np, dim=-1), Np)               # exact: everything lies on the grid
    assert up.shape == want.shape and torch.equal(up.detach().cpu(), want)
    (up * to_planes(cot, Np)).sum().backward()
    assert torch.equal(la.grad.cpu(), c.d_tokens) and torch.equal(lb.grad.cpu(), c.d_tokens)


# ---- the criterion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_forward_and_backward_meet_the_criterion(dev, dims):
    m, inp, got = case(dev, dims)
    B, Ci, Co, Np, S = dims
    assert got[0].shape == (B, 1, Co, 2 * S, Np * 2 * S) and got[1].shape == (B, Ci, Np * S * S) and got[3].shape == inp[2].shape
    check("x".join(map(str, dims)), got, run("torch32", m, *inp), run("f64", m, *inp), scales(m, *inp))
    assert float(got[3][..., 2 * S:].abs().max()) == 0.0                                    # exactly zero beyond column 2S


def test_without_biases_and_with_one_token_tensor(dev):
    """conv_bias NULL, plane_bias NULL and tok_b NULL: the forms the per-plane module and a bias-free convolution take."""
    dims = (1, 65, 9, 1, 6)
    m, (a, b, pb, cot), _ = case(dev, dims)
    nb = PlainUpsample(65, 9, 1).to(dev).requires_grad_(False)
    with torch.no_grad():
        nb.upsample.weight.copy_(m.upsample.weight)
    nb.upsample.bias = None
    got = run("kernel", nb, a, None, None, cot)
    sc = scales(nb, a, None, None, cot)
    bad = []
    for i, name in ((0, "out"), (1, "d_tokens")):
        errors(f"no bias {name}", got[i], run("f64", nb, a, None, None, cot)[i], run("torch32", nb, a, None, None, cot)[i], bound(sc[name]), bad)
    assert not bad, bad


# ---- bitwise properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 33, 7, 2, 3), (3, 512, 80, 2, 32)], ids=["small", "config"])
def test_a_batch_element_alone_gives_its_bits(dev, dims):
    m, (a, b, pb, cot), got = case(dev, dims)
    for i in range(dims[0]):
        alone = run("kernel", m, a[i:i + 1], b[i:i + 1], pb, cot[i:i + 1], need_pb=False)
        assert torch.equal(alone[0][0], got[0][i]) and torch.equal(alone[1][0], got[1][i])


@pytest.mark.parametrize("dims", [(2, 33, 7, 2, 3), (2, 96, 80, 3, 5)], ids=["small", "three-planes"])
def test_pair_layouts_and_inputs_read_in_place(dev, dims, launches):
    m, (a, b, pb, cot), got = case(dev, dims)
    B, Ci, Co, Np, S = dims
    x = a + b
    # a pair of tokens equals their float32 sum passed as one tensor
    one = run("kernel", m, x, None, pb, cot)
    assert torch.equal(one[0], got[0]) and torch.equal(one[1], got[1]) and torch.equal(one[3], got[3])
    # the joined and the per-plane layout hold the same values
    lx = x.clone().requires_grad_(True)
    del launches[:]
    up = m(lx.view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4))
    assert [n for n, _ in launches] == ["gh_scene_code_forward"] and launches[0][1][2].value == lx.data_ptr()    # detokenize's view, in place
    plain = run("kernel", m, x, None, None, cot)
    assert torch.equal(up.detach(), to_planes(plain[0], Np))
    (up * to_planes(cot, Np)).sum().backward()
    assert torch.equal(lx.grad, got[1])
    # the plane bias read in place through its first 2S columns equals a contiguous copy of them
    del launches[:]
    narrow = run("kernel", m, a, b, pb[..., :2 * S].contiguous(), cot)
    wide_view = run("kernel", m, a, b, pb[..., :2 * S], cot, need_pb=False)
    assert torch.equal(narrow[0], got[0]) and torch.equal(wide_view[0], got[0]) and torch.equal(narrow[3], got[3][..., :2 * S])
    fwd = [args for n, args in launches if n == "gh_scene_code_forward"]
    assert fwd[1][10].value == pb.data_ptr() and fwd[1][11] == pb.stride(0) and fwd[1][12] == pb.stride(1)    # no copy was made
    assert fwd[0][12] == 2 * S
    # tokens as a batch-strided and as a channel-strided slice of a larger tensor equal their contiguous copies
    big = torch.zeros(B, 2, Ci, Np * S * S, device=dev)
    big[:, 1] = a
    tall = torch.zeros(B, Ci, 3, Np * S * S, device=dev)
    tall[:, :, 2] = b
    del launches[:]
    sliced = run("kernel", m, big[:, 1], tall[:, :, 2], pb, cot)
    args = launches[0][1]
    assert args[2].value == big[:, 1].data_ptr() and args[3] == big.stride(0) and args[5].value == tall[:, :, 2].data_ptr() and args[7] == tall.stride(1)
    for s, g in zip(sliced, got):
        assert torch.equal(s, g)
    # a token tensor whose last stride is not 1 is copied, once, and gives the same bits
    turned = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert turned.stride(2) != 1 or Ci == 1
    for s, g in zip(run("kernel", m, turned, b, pb, cot), got):
        assert torch.equal(s, g)


def test_twice_gives_equal_results(dev):
    m, inp, got = case(dev, (1, 512, 80, 2, 32))
    again = run("kernel", m, *inp)
    for s, g in zip(again, got):
        assert torch.equal(s, g)


def test_graph_capture_on_a_side_stream_replays_the_eager_bits(dev):
    m, (a, b, pb, cot), got = case(dev, (2, 96, 80, 3, 5))
    la, lb, lpb = (t.clone().requires_grad_(True) for t in (a, b, pb))
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        out = SC.scene_code(m, (la, lb), lpb)                          # warm-up on the capture stream
        torch.autograd.grad((out * cot).sum(), (la, lb, lpb))
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = SC.scene_code(m, (la, lb), lpb)
        grads = torch.autograd.grad((out * cot).sum(), (la, lb, lpb))
    for _ in range(2):
        out.zero_()
        for g in grads:
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, got[0]) and torch.equal(grads[0], got[1]) and torch.equal(grads[1], got[2]) and torch.equal(grads[2], got[3])


def test_bias_only_backward_runs_no_token_product(dev, launches):
    """Only plane_bias requires a gradient — the fit that trains map_bias alone: the backward entry point gets d_tok = NULL."""
    m, (a, b, pb, cot), got = case(dev, (1, 512, 80, 2, 32))
    del launches[:]
    out, da, db, dpb = run("kernel", m, a, b, pb, cot, need_tok=False)
    assert [n for n, _ in launches] == ["gh_scene_code_forward", "gh_scene_code_backward"]
    args = launches[1][1]
    assert args[4] is None and args[5] is not None                     # d_tok NULL: no product; d_plane_bias given
    assert da is None and db is None and torch.equal(out, got[0]) and torch.equal(dpb, got[3])
    assert float(dpb[..., 64:].abs().max()) == 0.0
    # and the other way round: tokens only
    del launches[:]
    out, da, db, dpb = run("kernel", m, a, b, pb, cot, need_pb=False)
    assert launches[1][1][5] is None and dpb is None and torch.equal(da, got[1]) and torch.equal(db, got[2])


def test_empty_batch_launches_nothing(dev, launches):
    m = make_module((0, 33, 7, 2, 3), dev=dev)
    a, b, pb, cot = make_inputs((0, 33, 7, 2, 3), dev=dev)
    out, da, db, dpb = run("kernel", m, a, b, pb, cot)
    assert out.shape == (0, 1, 7, 6, 12) and da.shape == db.shape == (0, 33, 18) and dpb.shape == pb.shape
    assert float(dpb.abs().max()) == 0.0
    up = m(torch.zeros(0, 2, 33, 3, 3, device=dev))
    assert up.shape == (0, 2, 7, 6, 6)
    assert launches == []


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------------------
def test_fallbacks_take_torch(dev, launches):
    dims = (2, 33, 7, 2, 3)
    a, b, pb, cot = make_inputs(dims, dev=dev)

    def same(module, *inp):
        for p in module.parameters():
            p.grad = None
        got = run("kernel", module, *inp)
        pg = [p.grad for p in module.parameters()]
        for p in module.parameters():
            p.grad = None
        want = run("torch32", module, *inp)
        for g, w in zip(list(got) + pg, list(want) + [p.grad for p in module.parameters()]):
            assert (g is None) == (w is None)                          # a frozen parameter has no gradient on either path
            assert g is None or (g.dtype == w.dtype and torch.equal(g, w))
        return got

    trainable = make_module(dims, dev=dev, frozen=False)
    same(trainable, a, b, pb, cot)
    assert trainable.upsample.weight.grad is not None and trainable.upsample.bias.grad is not None
    assert same(make_module(dims, dev=dev).double(), a.double(), b.double(), pb.double(), cot)[0].dtype == torch.float64
    assert same(make_module(dims, dev=dev).bfloat16(), a.bfloat16(), b.bfloat16(), pb.bfloat16(), cot)[0].dtype == torch.bfloat16
    wide = (1, 8, 129, 1, 2)
    assert same(make_module(wide, dev=dev), *make_inputs(wide, dev=dev))[0].shape == (1, 1, 129, 4, 4)
    m = make_module(dims, dev=dev)
    assert torch.equal(SC.scene_code(m, (a, b), pb, ops="torch"), SC.scene_code_ref(m, (a, b), pb))
    assert launches == []


# ---- through the consumer --------------------------------------------------------------------------------------------------------------
def test_through_the_plane_fetch(dev):
    """plane.query_triplane_texture(vert_uv, scene_code(...)) at the config's shape: the path map_bias's gradient takes in the fit.
    The yardstick and the float64 referee are the same composition over scene_code_ref (the referee's fetch in plain torch)."""
    dims = (1, 512, 80, 2, 32)
    m, (a, b, pb, _), _ = case(dev, dims)
    g = torch.Generator().manual_seed(11)
    uv = (torch.rand(1, 1000, 2, generator=g) * 2 - 1).to(dev)
    cot = torch.randn(1, 1000, 80, generator=g).to(dev)
    fused = SimpleNamespace(cfg=SimpleNamespace(radius_texture=1.0))
    plain = SimpleNamespace(cfg=SimpleNamespace(radius_texture=1.0), plane_ops="torch")

    def post(mode, code):
        if mode == "f64":
            return plane.query_triplane_texture(plain, uv.double(), code)
        return plane.query_triplane_texture(fused, uv, code)

    got, t32, f64 = (run(mode, m, a, b, pb, cot, post=post) for mode in ("kernel", "torch32", "f64"))
    assert got[0].shape == (1, 1000, 80)
    check("fetch", got, t32, f64, scales(m, a, b, pb, cot, post=post))
    assert float(got[3][..., 64:].abs().max()) == 0.0 and float(got[3].abs().max()) > 0.0


# ---- the grafted class -----------------------------------------------------------------------------------------------------------------
def test_grafted_class_runs_the_per_plane_kernel(dev, launches):
    dims = (2, 96, 80, 3, 5)
    B, Ci, Co, Np, S = dims
    own, (a, b, pb, cot), _ = case(dev, dims)
    cls = SC.fused_upsample_cls(PlainUpsample)
    base = PlainUpsample(Ci, Co, Np).to(dev).requires_grad_(False)
    grafted = cls(Ci, Co, Np).to(dev).requires_grad_(False)
    for mod in (base, grafted):
        mod.load_state_dict(own.state_dict())
    x = (a + b)
    cot_p = to_planes(cot, Np)

    def through(mod, dt=torch.float32):
        lx = x.to(dt).clone().requires_grad_(True)
        up = mod(lx.view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4))      # detokenize's view
        (up * cot_p.to(dt)).sum().backward()
        return up.detach(), lx.grad

    del launches[:]
    got = through(grafted)
    assert [n for n, _ in launches] == ["gh_scene_code_forward", "gh_scene_code_backward"] and grafted.calls == 0
    mine = through(own)                                                # the standalone module: the same kernel form
    assert torch.equal(got[0], mine[0]) and torch.equal(got[1], mine[1])
    del launches[:]
    t32, f64 = through(base), through(base.double(), torch.float64)
    assert launches == [] and base.calls == 2
    sc = scales(own, a, b, None, cot)
    bad = []
    errors("grafted out", got[0], f64[0], t32[0], bound(sc["out"]), bad)
    errors("grafted d_tokens", got[1], f64[1], t32[1], bound(sc["d_tokens"]), bad)
    assert not bad, bad
    # a trainable upsample, and planes that are not square, go to the base class's forward
    del launches[:]
    grafted.requires_grad_(True)
    assert torch.equal(grafted(x.view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4)), PlainUpsample.forward(grafted, x.view(B, Ci, Np, S, S).permute(0, 2, 1, 3, 4)))
    grafted.requires_grad_(False)
    odd = torch.randn(1, Np, Ci, 2, 3, device=dev)
    assert torch.equal(grafted(odd), PlainUpsample.forward(grafted, odd))
    assert launches == [] and grafted.calls == 4
