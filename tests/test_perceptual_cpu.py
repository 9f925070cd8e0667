"""guassianhand_amd.perceptual without a GPU: the network's state dict against the committed list, both checkpoint spellings, the
plain-torch restatement against hand-written float64 loops, the CPU convention of ops="fused", the fit's new switch, and the C-ABI's
symbols and argument checks (the library cross-compiles for gfx950 here; nothing is launched)."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import _abi, _lib
from guassianhand_amd import perceptual as P
from tests import perceptual_cases as PC
from tests.helpers import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_is_the_committed_list_and_both_spellings_load():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "vgg19_slices.json")))
    net = P.VGG19Features()
    sd = net.state_dict()
    assert list(sd) == list(want) and all(list(sd[k].shape) == want[k] for k in want)
    assert not any(p.requires_grad for p in net.parameters())
    gen = torch.Generator().manual_seed(1)
    src = {k: torch.randn(v.shape, generator=gen) for k, v in sd.items()}
    tv = {"features." + k.split(".", 1)[1]: v for k, v in src.items()}                     # torchvision: features.N.weight
    tv["features.21.weight"], tv["classifier.0.bias"] = torch.zeros(512, 512, 3, 3), torch.zeros(4096)   # (the layers past relu4_1 are ignored)
    ref = {"vgg_loss.vgg_net." + k: v for k, v in src.items()}                             # the reference checkpoint
    ref["renderer.gs_net.out_layers.0.weight"] = torch.zeros(3, 3)
    for spelled in (src, tv, ref):
        m = P.VGG19Features()
        m.load_state_dict(spelled)
        got = m.state_dict()
        assert all(torch.equal(got[k], src[k]) for k in src)
    with pytest.raises(RuntimeError):
        P.VGG19Features().load_state_dict({k: v for k, v in tv.items() if not k.startswith("features.19.")})


def _loops(features, x, y):
    """VGGLoss.forward by hand in float64: Python loops over pixels, taps and channels."""
    mean, std = torch.tensor(P.MEAN, dtype=torch.float64), torch.tensor(P.STD, dtype=torch.float64)

    def conv_relu(h, w, b):                                                                  # h (C, H, W)
        Cn, H, W = h.shape
        out = torch.zeros(w.shape[0], H, W, dtype=torch.float64)
        for co in range(w.shape[0]):
            for i in range(H):
                for j in range(W):
                    s = float(b[co])
                    for ky in range(3):
                        for kx in range(3):
                            ii, jj = i + ky - 1, j + kx - 1
                            if 0 <= ii < H and 0 <= jj < W:
                                s += float((w[co, :, ky, kx] * h[:, ii, jj]).sum())
                    out[co, i, j] = max(s, 0.0)
        return out

    def pool(h):
        Cn, H, W = h.shape
        out = torch.zeros(Cn, H // 2, W // 2, dtype=torch.float64)
        for c in range(Cn):
            for i in range(H // 2):
                for j in range(W // 2):
                    out[c, i, j] = max(float(h[c, 2 * i + a, 2 * j + b]) for a in (0, 1) for b in (0, 1))
        return out

    def net(img):
        h = (img.double() - mean[:, None, None]) / std[:, None, None]
        taps = []
        for _, n, _, _ in P.CONVS:
            if n in P.POOL_BEFORE:
                h = pool(h)
            conv = features.conv(n)
            h = conv_relu(h, conv.weight.double(), conv.bias.double())
            if n in P.TAPS:
                taps.append(h)
        return taps

    total = 0.0
    for wt, f, t in zip(P.TAP_WEIGHTS, net(x[0]), net(y[0])):
        total += wt * float((f - t).abs().sum()) / f.numel()
    return total


def test_ref_is_the_hand_written_loops():
    feats = PC.make_features((3, 4, 3, 5), seed=2)
    x, y = PC.make_images(1, 8, 8, 7)
    want = _loops(feats, x, y)
    got = float(P.perceptual_loss_ref(feats, x, y, acc=torch.float64))
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert [tuple(t.shape) for t in feats(P._normalised(x))] == [(1, 8, 8, 3), (1, 4, 4, 4), (1, 2, 2, 3), (1, 1, 1, 5)]


def test_cpu_tensors_take_the_torch_statements():
    """The package's convention for the opt-in blocks: ops="fused" on a CPU tensor runs the plain-torch statements, bit for bit what
    ops="torch" gives, differentiable in everything."""
    c = PC.make_conv((1, 2, 3, 3, 5), 0)
    w = c.weight.clone().requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    a = P.conv3x3(x, w, c.bias, True, "fused")
    b = P.conv3x3(c.x, c.weight, c.bias, True, "torch")
    assert torch.equal(a, b) and torch.equal(a, torch.relu(F.conv2d(c.x.permute(0, 3, 1, 2), c.weight, c.bias, padding=1)).permute(0, 2, 3, 1))
    a.backward(c.g)
    assert w.grad is not None and x.grad is not None
    xp, _, _ = PC.make_pool(3, 5)
    assert torch.equal(PC.bits(P.max_pool2x2(xp)), PC.bits(P.max_pool2x2(xp, "torch")))
    feats = PC.make_features(PC.LOSS_WIDTHS)
    xi, yi = PC.make_images(1, 8, 8, 0)
    loss = P.PerceptualLoss(feats)
    loss.set_target(yi)
    assert torch.equal(loss(xi), P.perceptual_loss(feats, xi, yi)) and torch.equal(loss(xi), loss(xi, yi, ops="torch"))
    with pytest.raises(ValueError):
        P.conv3x3(c.x, c.weight, c.bias, ops="triton")
    with pytest.raises(ValueError):
        P.PerceptualLoss(feats)(xi)                                                          # no target


def test_pack_weights_layouts():
    w = torch.randn(5, 3, 3, 3, generator=torch.Generator().manual_seed(0))
    wf, wb = P.pack_weights(w)
    assert wf.shape == (9, 128, 3) and wb.shape == (9, 128, 5)
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(wf[3 * ky + kx, :5], w[:, :, ky, kx]) and torch.equal(wb[3 * ky + kx, :3], w[:, :, 2 - ky, 2 - kx].t())
    assert float(wf[:, 5:].abs().max()) == 0.0 and float(wb[:, 3:].abs().max()) == 0.0


def test_fit_takes_a_perceptual_term_and_does_not_capture_it():
    """OneShotFit(perceptual=...) on the CPU with the dense oracle renderer: the step's loss is the step's loss without the term plus
    lambda_vgg * VGGLoss of the bbox-zeroed render, and captured() refuses."""
    from guassianhand_amd.fit import OneShotFit
    from tests.helpers import oracle_render_views, tiny_fit_problem
    pb = tiny_fit_problem(P=40, n_views=2, hw=(8, 8), map_hw=(8, 16))
    gen = torch.Generator().manual_seed(3)
    gt, mask = torch.rand(2, 8, 8, 3, generator=gen), (torch.rand(2, 8, 8, generator=gen) > 0.5).float()
    bbox = torch.ones(2, 8, 8)
    bbox[:, :2] = 0
    feats = PC.make_features((4, 4, 8, 8))
    mk = lambda **kw: OneShotFit(pb["gs"], pb["uv"], map_hw=pb["map_hw"], render_fn=oracle_render_views, active_texels=False, **kw)
    args = (pb["w2c"], pb["K"], pb["H"], pb["W"], pb["bg"], gt, mask, bbox)
    plain, with_vgg = mk(), mk(perceptual=P.PerceptualLoss(feats), lambda_vgg=0.25)
    assert not any("slice" in k for k in with_vgg.state_dict())                               # the frozen network is no state of the fit
    base, total = float(plain.step(*args)), float(with_vgg.step(*args))
    img = oracle_render_views(pb["gs"], pb["w2c"], pb["K"], pb["H"], pb["W"], pb["bg"], color_w=torch.ones(48), xyz_b=torch.zeros(3),
                              color_b=torch.zeros(40, 48), opacity_b=torch.zeros(40, 1))["comp_rgb"]
    term = float(P.perceptual_loss_ref(feats, (img * bbox[..., None]).permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)))
    assert abs(total - (base + 0.25 * term)) <= 1e-5 * abs(total), (total, base, term)
    with pytest.raises(NotImplementedError, match="perceptual"):
        with_vgg.captured(*args)


def test_library_exports_the_conv_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.CONV_SYMBOLS:
        assert hasattr(L, sym), sym
    assert sorted(_abi.CONV_SYMBOLS) == header_symbols("gh_conv.h") and set(_abi.CONV_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    assert any(s.endswith("gh_conv.hip") for s in _lib.SOURCES) and any(h.endswith("gh_conv.h") for h in _lib.HEADERS)
    h = open(os.path.join(ROOT, "include", "gh_conv.h")).read()
    for name in ("GH_CONV_RELU", "GH_CONV_MAX_C", "GH_CONV_PIXELS", "GH_CONV_CHUNK", "GH_CONV_FILL"):
        assert f"#define {name} {getattr(_abi, name)} " in h, name


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes in the header's order (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    one, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2)
    INV, UNS, OK = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED, _abi.GH_OK

    def fwd(N=1, H=4, W=4, Cin=3, Cout=8, x=one, w=one, flags=0, chunk=0, y=one, gate=None):
        return L.gh_conv3x3_forward(x, N, H, W, Cin, Cout, w, one, flags, chunk, y, gate, None)

    def bwd(N=1, H=4, W=4, Cin=3, Cout=8, dy=one, w=one, flags=0, chunk=0, dx=one, gate=None):
        return L.gh_conv3x3_backward_data(dy, gate, N, H, W, Cin, Cout, w, flags, chunk, dx, None)

    for call in (fwd, bwd):
        assert call(N=-1) == call(Cin=0) == call(Cout=0) == call(flags=2) == call(chunk=48) == INV
        assert call(Cin=513) == call(Cout=513) == UNS
        assert call(N=0) == call(H=0, w=None) == OK                                          # empty: nothing is looked at, nothing launched
        assert call(w=None) == call(w=odd) == call(flags=_abi.GH_CONV_RELU) == INV           # a ReLU without its gate
    assert fwd(x=None) == fwd(y=None) == bwd(dy=None) == bwd(dx=None) == INV
    assert L.gh_conv3x3_weight_floats(3, 64) == 9 * 128 * 3 and L.gh_conv3x3_weight_floats(256, 129) == 9 * 256 * 256
    assert L.gh_conv3x3_weight_floats(0, 4) == L.gh_conv3x3_weight_floats(4, 513) == 0
    assert L.gh_maxpool2x2_forward(one, 1, 4, 4, 0, one, one, None) == L.gh_maxpool2x2_forward(one, -1, 4, 4, 2, one, one, None) == INV
    assert L.gh_maxpool2x2_forward(None, 1, 1, 1, 2, None, None, None) == OK                 # an empty output
    assert L.gh_maxpool2x2_forward(None, 1, 2, 2, 2, one, one, None) == L.gh_maxpool2x2_forward(one, 1, 2, 2, 2, None, None, None) == INV
    assert L.gh_maxpool2x2_backward(one, one, 0, 4, 4, 2, None, None) == OK
    assert L.gh_maxpool2x2_backward(one, one, 1, 4, 4, 2, None, None) == L.gh_maxpool2x2_backward(None, one, 1, 4, 4, 2, one, None) == INV
