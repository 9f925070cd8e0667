"""guassianhand_amd.perceptual on the device: the 3x3 convolution forward and backward-data, the 2x2 pooling, the perceptual loss and
the fit step that carries it (include/gh_conv.h).

Values are held to tests/res_block_cases.three_way — per field, max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64| — with the
float64 restatement on the CPU and the float32 torch statements (ops="torch") on the device, all on the same inputs. Every case that
compares gradients or pooled values first asserts the margins of tests/perceptual_cases.py on its float64 reference. What the header
promises bit for bit (position independence, run-to-run equality, the pooling against F.max_pool2d) is compared with torch.equal."""
import copy

import pytest
import torch

from tests import perceptual_cases as PC
from tests.res_block_cases import three_way

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def P():
    from guassianhand_amd import perceptual
    return perceptual


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", (False, True), ids=("linear", "relu"))
@pytest.mark.parametrize("case", PC.CONV_CASES, ids=PC.conv_id)
def test_conv_three_way(dev, case, relu):
    c = PC.make_conv(tuple(case[:5]), PC.conv_seed(case))
    f64, pre = PC.conv_f64(c, relu)
    tag = f"conv {PC.conv_id(case)} {'relu' if relu else 'linear'}"
    if relu:
        m = PC.relu_margin(pre)
        print(f"{tag} relu margin {m:.3e} (guard {PC.GUARD:.3e})")
        assert m > PC.GUARD, (tag, m)
    kernel = PC.conv_run(c, relu, "fused", case[5], dev)
    torch32 = PC.conv_run(c, relu, "torch", 0, dev)
    three_way(kernel, torch32, f64, fields=("y", "dx"), tag=tag)


def _fwd_bwd(P, x, w, b, g, relu, chunk=0):
    """(y, dx) of the kernels for contiguous device tensors."""
    xl = x.clone().requires_grad_(True)
    y = P.conv3x3(xl, w, b, relu, "fused", chunk=chunk)
    assert isinstance(y.grad_fn, P._Conv3x3Fn._backward_cls)                                 # the HIP path, not a fallback
    y.backward(g)
    return y.detach(), xl.grad


@pytest.mark.parametrize("relu", (False, True), ids=("linear", "relu"))
def test_conv_does_not_depend_on_the_position_in_the_batch(dev, P, relu):
    """An image alone against the same image as element 1 of a batch of 3 (its 135 pixels then start mid-tile and end in another), two
    runs of the same call, and every chunk of output channels: the same bits."""
    gen = torch.Generator().manual_seed(11)
    x, g = torch.randn(3, 9, 15, 33, generator=gen).to(dev), torch.randn(3, 9, 15, 70, generator=gen).to(dev)
    w, b = (torch.randn(70, 33, 3, 3, generator=gen) / 17).to(dev), torch.randn(70, generator=gen).to(dev)
    y3, d3 = _fwd_bwd(P, x, w, b, g, relu)
    y1, d1 = _fwd_bwd(P, x[1:2].contiguous(), w, b, g[1:2].contiguous(), relu)
    assert torch.equal(y3[1:2], y1) and torch.equal(d3[1:2], d1)
    again = _fwd_bwd(P, x, w, b, g, relu)
    assert torch.equal(again[0], y3) and torch.equal(again[1], d3)
    for chunk in (32, 64, 128):
        yc, dc = _fwd_bwd(P, x, w, b, g, relu, chunk)
        assert torch.equal(yc, y3) and torch.equal(dc, d3), chunk


@pytest.mark.parametrize("relu", (False, True), ids=("linear", "relu"))
def test_explicit_zeros_are_the_padding(dev, P, relu):
    """A 5x7 image against the same image centred in a 9x11 field of zeros: the same bits at the original pixels, forward and
    backward (the cotangent is zero outside them)."""
    gen = torch.Generator().manual_seed(12)
    x, g = torch.randn(1, 5, 7, 6, generator=gen).to(dev), torch.randn(1, 5, 7, 9, generator=gen).to(dev)
    w, b = (torch.randn(9, 6, 3, 3, generator=gen) / 7).to(dev), torch.randn(9, generator=gen).to(dev)
    X, G = torch.zeros(1, 9, 11, 6, device=dev), torch.zeros(1, 9, 11, 9, device=dev)
    X[:, 2:7, 2:9], G[:, 2:7, 2:9] = x, g
    y, d = _fwd_bwd(P, x, w, b, g, relu)
    Y, D = _fwd_bwd(P, X, w, b, G, relu)
    assert torch.equal(Y[:, 2:7, 2:9], y) and torch.equal(D[:, 2:7, 2:9], d)


def test_conv_fallbacks(dev, P):
    """A weight that trains takes the torch statements — the same values as ops="torch", and a weight gradient; an empty batch launches
    nothing."""
    c = PC.make_conv((1, 2, 3, 3, 5), 0)
    x, b, g = c.x.to(dev).requires_grad_(True), c.bias.to(dev), c.g.to(dev)
    w = c.weight.to(dev).requires_grad_(True)
    y = P.conv3x3(x, w, b, True, "fused")
    assert not isinstance(y.grad_fn, P._Conv3x3Fn._backward_cls)
    assert torch.equal(y, P.conv3x3(x, w.detach(), b, True, "torch"))
    y.backward(g)
    assert w.grad is not None and w.grad.shape == w.shape and float(w.grad.abs().max()) > 0 and x.grad is not None
    e = P.conv3x3(torch.zeros(0, 4, 4, 3, device=dev), c.weight.to(dev), b, True, "fused")
    assert e.shape == (0, 4, 4, 5)
    assert P.conv3x3(c.x.double().to(dev), c.weight.double().to(dev), b.double(), True, "fused").dtype == torch.float64


# ---- pooling ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", PC.POOL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_is_max_pool2d_bit_for_bit(dev, P, hw):
    x, g, has_special = PC.make_pool(*hw)
    if hw == (7, 8):
        assert has_special and bool(torch.isnan(x).any()) and bool(torch.isinf(x).any())
        w = torch.nn.functional.unfold(x.permute(0, 3, 1, 2).reshape(-1, 1, *hw), 2, stride=2).transpose(1, 2).reshape(-1, 4)
        for a, b_ in PC.PAIRS:                                                             # a window whose maximum is tied at exactly this pair
            others = [q for q in range(4) if q not in (a, b_)]
            assert bool(((w[:, a] == w[:, b_]) & (w[:, others] < w[:, a:a + 1]).all(1)).any()), (a, b_)
    want_y, want_choice, want_dx = PC.pool_cpu(x, g)
    y, choice = P._pool_forward(x.to(dev))
    assert y.shape == want_y.shape and torch.equal(PC.bits(y.cpu()), PC.bits(want_y)) and torch.equal(choice.cpu(), want_choice)
    xl = x.to(dev).requires_grad_(True)
    out = P.max_pool2x2(xl)
    assert torch.equal(PC.bits(out.detach().cpu()), PC.bits(want_y))
    out.backward(g.to(dev))
    assert xl.grad.shape == x.shape and torch.equal(PC.bits(xl.grad.cpu()), PC.bits(want_dx))


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.LOSS_CASES, ids=lambda c: f"{c[0]}x3x{c[1]}x{c[2]}")
def test_perceptual_loss_three_way(dev, P, case):
    B, H, W, seed = case
    feats = PC.make_features(PC.LOSS_WIDTHS, seed)
    x, y = PC.make_images(B, H, W, seed)
    tag = f"loss {B}x3x{H}x{W}"
    PC.assert_net_margins(feats, x, y, tag)
    f64 = PC.loss_f64(feats, x, y)
    fd = copy.deepcopy(feats).to(dev)

    def run(ops, cached):
        xl = x.to(dev).requires_grad_(True)
        mod = P.PerceptualLoss(fd)
        if cached:
            mod.set_target(y.to(dev), ops=ops)
            loss = mod(xl, ops=ops)
        else:
            loss = P.perceptual_loss(fd, xl, y.to(dev), ops=ops)
        loss.backward()
        return dict(loss=loss.detach().cpu(), dimg=xl.grad.cpu())

    kernel, torch32 = run("fused", True), run("torch", True)
    three_way(kernel, torch32, f64, fields=("loss", "dimg"), tag=tag)
    two = run("fused", False)
    assert torch.equal(two["loss"], kernel["loss"]) and torch.equal(two["dimg"], kernel["dimg"])
    if H == 8:
        assert [tuple(t.shape[1:3]) for t in fd(P._normalised(x.to(dev)))] == [(8, 8), (4, 4), (2, 2), (1, 1)]


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------
def test_fit_step_with_a_perceptual_term(dev, P):
    """One step() of a two-view fit with the term, keep_boundary_grads: its loss and its gradients at the rasteriser boundary, three-way.
    The render and its backward are the same HIP rasteriser on all three sides; what differs is the loss on the rendered images and its
    image gradient — the kernels (PerceptualLoss), the float32 torch statements (ops="torch") and, for the float64 side, fit_loss and
    perceptual_loss_ref in double on the CPU from the same rendered image, its gradient handed back to the render's backward."""
    from guassianhand_amd.fit import OneShotFit, fit_loss
    c = PC.fit_case(device=dev)
    pb, gt, mask, bbox, feats, args = c.pb, c.gt, c.mask, c.bbox, c.feats, c.args
    fd = copy.deepcopy(feats).to(dev)
    lam = 0.1

    def step(ops):
        fit = OneShotFit(pb["gs"], pb["uv"], map_hw=pb["map_hw"], perceptual=P.PerceptualLoss(fd, ops=ops), lambda_vgg=lam)
        fit.keep_boundary_grads = True
        loss = fit.step(*args)
        return fit, dict(loss=loss.detach().cpu(), **{k: v.cpu() for k, v in fit.boundary_grads.items()})

    fit, kernel = step("fused")
    _, torch32 = step("torch")
    with pytest.raises(NotImplementedError, match="perceptual"):
        fit.captured(*args)

    ref = OneShotFit(pb["gs"], pb["uv"], map_hw=pb["map_hw"])
    blend = ref.blend_values()
    names = ("color_w", "color_b", "opacity_b")
    leaves = {k: (v.detach().requires_grad_(True) if k in names else v) for k, v in blend.items()}
    out = ref.render(*args[:5], leaves)
    img, alpha = out["image_chw"], out["alpha"]
    i64, a64 = img.detach().cpu().double().requires_grad_(True), alpha.detach().cpu().double().requires_grad_(True)
    zeroed = i64 * (bbox.cpu()[:, None] != 0)
    target = gt.cpu().permute(0, 3, 1, 2)
    PC.assert_net_margins(feats, zeroed, target, "fit")
    loss64 = fit_loss(i64.permute(0, 2, 3, 1), a64[..., None].expand(-1, -1, -1, 3), gt.cpu().double(), mask.cpu().double(), bbox.cpu()) / 2 \
        + lam * P.perceptual_loss_ref(feats, zeroed, target, acc=torch.float64)
    gi, ga = torch.autograd.grad(loss64, [i64, a64])
    grads = torch.autograd.grad([img, alpha], [leaves[k] for k in names], [gi.float().to(dev), ga.float().to(dev)])
    f64 = dict(loss=loss64.detach(), **{k: g.cpu() for k, g in zip(names, grads)})
    assert float(f64["color_b"].abs().max()) > 0 and float(ga.abs().max()) > 0
    three_way(kernel, torch32, f64, fields=("loss",) + names, tag="fit step")
