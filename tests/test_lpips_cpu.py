"""guassianhand_amd.lpips without a GPU: the plain-torch statements against float64 and against their own invariants, the quantiser at
its ties and edges, the three checkpoint spellings, the evaluator's protocol against crop + quantise + lpips_ref written out by hand,
the Evaluator's new switch, and the C-ABI's symbols and argument checks (the library cross-compiles for gfx950 here; nothing is
launched)."""
import ctypes as C
import math
import os

import pytest
import torch

from guassianhand_amd import _abi, _lib
from guassianhand_amd import lpips as LP
from guassianhand_amd.metrics import Evaluator
from tests import lpips_cases as LC
from tests.helpers import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CASES = [c for c in LC.E2E_CASES if c[0] == LC.SMALL]


@pytest.mark.parametrize("case", SMALL_CASES, ids=LC.case_id)
def test_ref_float32_against_float64(case):
    """A feature carries about 2^-24 sqrt(R) <= 2^-18 of relative float32 rounding (R <= 3456 products in a chain), and the unit
    normalisation amplifies it by at most (largest norm / smallest non-zero norm) of the tap, which the case's float64 reference
    gives: |d32 - d64| <= 2^-18 / margin of the score."""
    widths, N, H, W, seed = case
    net, (x0, x1) = LC.make_net(widths, seed), LC.make_images(N, H, W, seed)
    norms = LC.tap_norms(net, x0, x1)
    LC.norm_guard(norms, LC.case_id(case))
    margin, _ = LC.norm_margin(norms)
    d32, t32 = LP.lpips_ref(net, x0, x1, terms=True)
    d64, t64 = LP.lpips_ref(net, x0, x1, acc=torch.float64, terms=True)
    assert d32.dtype == torch.float32 and d64.dtype == torch.float64 and t64.shape == (5, N)
    err = float((d32.double() - d64).abs().max())
    print(f"{LC.case_id(case)}: |d32 - d64| {err:.3e}, d64 {d64.tolist()}, bound {2.0 ** -18 / margin * float(d64.max()):.3e}")
    assert err <= 2.0 ** -18 / margin * float(d64.max())
    assert float(d64.min()) > 0 and torch.equal(d64, (((t64[0] + t64[1]) + t64[2]) + t64[3]) + t64[4])


def test_identical_images_score_zero_and_the_distance_is_symmetric():
    widths, N, H, W, seed = SMALL_CASES[1]
    net, (x0, x1) = LC.make_net(widths, seed), LC.make_images(N, H, W, seed)
    assert torch.equal(LP.lpips_ref(net, x0, x0.clone()), torch.zeros(N))
    assert torch.equal(LP.lpips_ref(net, x0, x1), LP.lpips_ref(net, x1, x0))
    assert torch.equal(LP.lpips_distance(net, x0, x1), LP.lpips_ref(net, x0, x1).double())   # a CPU tensor runs the torch statements
    with pytest.raises(ValueError, match="31"):
        LP.lpips_distance(net, x0[:, :, :30], x1[:, :, :30])
    with pytest.raises(ValueError):
        LP.lpips_distance(net, x0, x1, ops="triton")


def test_quantiser_rounds_ties_to_even_clamps_and_keeps_nan():
    ties = LC.quantiser_ties()
    assert sum(k % 2 == 0 for k in ties) >= 8 and sum(k % 2 == 1 for k in ties) >= 8, len(ties)
    v = torch.tensor([ties[k] for k in sorted(ties)], dtype=torch.float32)
    want_q = torch.tensor([k if k % 2 == 0 else k + 1 for k in sorted(ties)], dtype=torch.float64)
    assert torch.equal(LP.quantize_unit(v), (want_q / 127.5 - 1.0).float())
    edge = torch.tensor([-0.3, -1e-9, 0.0, 1.0, 1.0 + 1e-3, 1.7, float("inf"), float("-inf")])
    assert LP.quantize_unit(edge).tolist() == [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0]
    assert math.isnan(float(LP.quantize_unit(torch.tensor([float("nan")]))))
    grid = torch.arange(256, dtype=torch.float32) / 255.0                                 # what an 8-bit image holds survives the trip
    assert torch.equal(LP.quantize_unit(grid), (torch.arange(256, dtype=torch.float64) / 127.5 - 1.0).float())
    assert torch.equal(LP.quantize_unit(v, quantize=False), ((v * 255.0).double() / 127.5 - 1.0).float())


def test_load_state_dict_takes_the_three_key_forms():
    src_net = LC.make_net(LC.SMALL, 5)
    with torch.no_grad():
        src_net.shift.copy_(torch.tensor([0.1, 0.2, 0.3]))
        src_net.scale.copy_(torch.tensor([0.4, 0.5, 0.6]))
    own = src_net.state_dict()
    assert sorted(own) == sorted([f"conv{k}.{n}" for k in range(1, 6) for n in ("weight", "bias")] + [f"lin{k}" for k in range(1, 6)] +
                                 ["shift", "scale"])
    assert not any(p.requires_grad for p in src_net.parameters())
    idx = [c[0] for c in LP.CONVS]
    rest = {k: v for k, v in own.items() if not k.startswith("conv")}
    tv = dict(rest, **{f"features.{idx[k - 1]}.{n}": own[f"conv{k}.{n}"] for k in range(1, 6) for n in ("weight", "bias")})
    tv["classifier.1.weight"] = torch.zeros(3, 3)                                        # (ignored)
    pkgs = []
    for lin_key in ("lin{}.model.1.weight", "lins.{}.model.1.weight"):
        pkg = {f"net.slice{k}.{idx[k - 1]}.{n}": own[f"conv{k}.{n}"] for k in range(1, 6) for n in ("weight", "bias")}
        pkg.update({lin_key.format(k - 1): own[f"lin{k}"].view(1, -1, 1, 1) for k in range(1, 6)})
        pkg["scaling_layer.shift"], pkg["scaling_layer.scale"] = own["shift"].view(1, 3, 1, 1), own["scale"].view(1, 3, 1, 1)
        pkg["lin0.model.0.p"] = torch.zeros(1)                                            # (ignored)
        pkgs.append(pkg)
    x0, x1 = LC.make_images(1, 31, 31, 2)
    want = LP.lpips_ref(src_net, x0, x1)
    for spelled in (own, tv, *pkgs):
        m = LP.AlexLPIPS(LC.SMALL)
        m.load_state_dict(spelled)
        got = m.state_dict()
        assert all(torch.equal(got[k], own[k]) for k in own)
        assert torch.equal(LP.lpips_ref(m, x0, x1), want)
    with pytest.raises(RuntimeError):
        LP.AlexLPIPS(LC.SMALL).load_state_dict({k: v for k, v in own.items() if k != "lin3"})


def _views(Nv=3, H=48, W=52, seed=0):
    g = torch.Generator().manual_seed(7400 + seed)
    pred, gt = torch.rand(Nv, 3, H, W, generator=g) * 1.2 - 0.1, torch.rand(Nv, 3, H, W, generator=g)   # some values outside [0, 1]
    mask = torch.zeros(Nv, H, W)
    mask[0, 5:40, 7:45] = 1          # 38 wide, 35 high
    mask[1, 2, 3] = mask[1, 35, 40] = 1   # two corners: 38 wide, 34 high
    mask[2, 10:40, 4:44] = 1         # 40 wide, 30 high: under 31
    bbm = (torch.rand(Nv, H, W, generator=g) > 0.3).float()
    return pred, gt, mask, bbm


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("with_bbm", [False, True])
def test_scores_are_crop_quantise_ref_by_hand(layout, with_bbm):
    net = LC.make_net(LC.SMALL, 0)
    pred, gt, mask, bbm = _views()
    boxes = [(7, 5, 38, 35), (3, 2, 38, 34)]
    want = []
    for v, (bx, by, bw, bh) in enumerate(boxes):
        p, g = pred[v, :, by:by + bh, bx:bx + bw].clone(), gt[v, :, by:by + bh, bx:bx + bw]
        if with_bbm:
            p = p * bbm[v, by:by + bh, bx:bx + bw]
        q = lambda t: (torch.clamp(torch.round(t * 255.0), 0, 255).double() / 127.5 - 1.0).float()
        want.append(float(LP.lpips_ref(net, q(p)[None], q(g)[None])[0]))
    a, b = (pred, gt) if layout == "chw" else (pred.permute(0, 2, 3, 1).contiguous(), gt.permute(0, 2, 3, 1).contiguous())
    keep = (a.clone(), b.clone())
    got = LP.lpips_scores(net, a, b, mask, bbox_mask=bbm if with_bbm else None, layout=layout)
    assert got.dtype == torch.float64 and got.shape == (3,)
    assert got[:2].tolist() == want and math.isnan(float(got[2]))                         # a crop of 30 x 40 scores NaN
    assert torch.equal(a, keep[0]) and torch.equal(b, keep[1])
    whole = LP.lpips_scores(net, a, b, layout=layout, quantize=False)
    chw = (lambda t: t) if layout == "chw" else (lambda t: t.permute(0, 3, 1, 2))
    assert torch.equal(whole, LP.lpips_ref(net, LP.quantize_unit(chw(a), False), LP.quantize_unit(chw(b), False)).double())


def test_boxes_are_the_bounding_rects():
    _, _, mask, _ = _views()
    mask = torch.cat([mask, torch.zeros(1, *mask.shape[1:])])
    assert LP._boxes(mask).tolist() == [[7, 5, 38, 35], [3, 2, 38, 34], [4, 10, 40, 30], [0, 0, 0, 0]]


def test_evaluator_returns_three_keys_without_a_net_and_four_with_one():
    net = LC.make_net(LC.SMALL, 0)
    pred, gt, mask, _ = _views()
    plain = Evaluator().compute_score(pred[:1], gt[:1], mask_at_box=mask[:1])
    assert sorted(plain) == ["mse", "psnr", "ssim"]
    four = Evaluator(lpips=net).compute_score(pred[:1], gt[:1], mask_at_box=mask[:1])
    assert sorted(four) == ["lpips", "mse", "psnr", "ssim"] and all(isinstance(v, float) for v in four.values())
    assert {k: four[k] for k in plain} == plain
    assert four["lpips"] == float(LP.lpips_scores(net, pred[:1], gt[:1], mask[:1])[0]) and four["lpips"] > 0
    assert sorted(Evaluator().compute_score(pred[2:], gt[2:], mask_at_box=mask[2:])) == ["mse", "psnr", "ssim"]   # 40 x 30: SSIM is fine
    with pytest.raises(ValueError, match="31"):
        Evaluator(lpips=net).compute_score(pred[2:], gt[2:], mask_at_box=mask[2:])


def test_a_network_on_another_device_is_refused_before_any_launch(monkeypatch):
    """The images on one device, the network on another (the easy mistake Evaluator(lpips=AlexLPIPS()) with device images): ValueError
    on the host from every entry point, with nothing launched. The meta device stands in for the images' device here."""
    def no_launch(name, *a, **k):
        raise AssertionError(f"{name} was launched")
    monkeypatch.setattr(LP, "launch", no_launch)
    net = LC.make_net(LC.SMALL, 0)
    meta = torch.device("meta")
    x = torch.empty(2, 3, 35, 32, device=meta)
    with pytest.raises(ValueError, match="net.* is on cpu"):
        LP.lpips_distance(net, x, x)
    with pytest.raises(ValueError, match="net.* is on cpu"):
        LP.lpips_distance(net, x, x, ops="torch")
    with pytest.raises(ValueError, match="net.* is on cpu"):
        LP.lpips_scores(net, x, x)
    with pytest.raises(ValueError, match="net.* is on cpu"):
        LP._scores_with_boxes(net, x, x, None, [(0, 0, 32, 35)] * 2, None, "chw", True, "fused")
    with pytest.raises(ValueError, match="net.* is on cpu"):
        LP._forward_fused(net, torch.empty(4, 35, 32, 3, device=meta), 2, False)
    with pytest.raises(ValueError, match="ROCm"):
        LP.prepare_input(x, x, None, (35, 32), shift=net.shift, scale=net.scale)      # not a ROCm tensor: nothing to launch on
    LP._check_net(net, torch.device("cpu"))
    f32 = torch.float32
    LP._check_on(torch.device("cpu"), (("a", net.shift, f32), ("none", None, f32)))
    with pytest.raises(ValueError, match="shift is on cpu"):
        LP._check_on(meta, (("shift", net.shift, f32),))
    with pytest.raises(ValueError, match="expected torch.int32"):
        LP._check_on(torch.device("cpu"), (("bbox", torch.zeros(2, 4, dtype=torch.int64), torch.int32),))
    with pytest.raises(TypeError):
        LP._check_on(torch.device("cpu"), (("lin", [1.0], f32),))
    assert not LP._fused_applies(LC.make_net(LC.SMALL, 0).double(), torch.empty(1, device=meta))


def test_pack_conv_layout():
    w = torch.randn(5, 3, 11, 11, generator=torch.Generator().manual_seed(0))
    wp = LP.pack_conv(w)
    assert wp.shape == (128, 364)
    for ky in (0, 4, 10):
        for kx in (0, 7, 10):
            assert torch.equal(wp[:5, (11 * ky + kx) * 3:(11 * ky + kx) * 3 + 3], w[:, :, ky, kx])
    assert float(wp[5:].abs().max()) == 0.0 and float(wp[:, 363:].abs().max()) == 0.0


def test_library_exports_the_lpips_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.LPIPS_SYMBOLS:
        assert hasattr(L, sym), sym
    assert sorted(_abi.LPIPS_SYMBOLS) == header_symbols("gh_lpips.h") and set(_abi.LPIPS_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    assert any(s.endswith("gh_lpips.hip") for s in _lib.SOURCES) and any(h.endswith("gh_lpips.h") for h in _lib.HEADERS)
    h = open(os.path.join(ROOT, "include", "gh_lpips.h")).read()
    for name in ("GH_LPIPS_RELU", "GH_LPIPS_MAX_C", "GH_LPIPS_PIXELS", "GH_LPIPS_CHUNK", "GH_LPIPS_FILL", "GH_LPIPS_FLAT_CIN",
                 "GH_LPIPS_HEAD_PIXELS", "GH_LPIPS_TAPS", "GH_LPIPS_MIN_SIZE"):
        assert f"#define {name} {getattr(_abi, name)} " in h or f"#define {name} {getattr(_abi, name)}\n" in h, name
    for name in ("GH_LPIPS_PRED_HWC", "GH_LPIPS_GT_HWC", "GH_LPIPS_QUANTIZE", "GH_LPIPS_SIGNED"):
        assert f"#define {name} {getattr(_abi, name)}u " in h, name
    assert "specified by its mathematics, unpinned against the package" in h
    assert C.sizeof(_abi.GhLpipsWeights) == 15 * C.sizeof(C.c_void_p)
    assert (_abi.GH_VERSION_MAJOR, _abi.GH_VERSION_MINOR) == (0, 8)


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes in the header's order (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    one, odd, four = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)
    INV, UNS, OK = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED, _abi.GH_OK

    def conv(N=1, H=31, W=31, Cin=3, Cout=8, K=11, s=4, p=2, x=one, w=one, flags=0, chunk=0, y=one):
        return L.gh_conv2d_forward(x, N, H, W, Cin, Cout, K, s, p, w, one, flags, chunk, y, None)

    assert conv(N=-1) == conv(Cin=0) == conv(Cout=0) == conv(K=7) == conv(s=2) == conv(p=11) == conv(p=-1) == conv(flags=2) == conv(chunk=48) == INV
    assert conv(Cin=513) == conv(Cout=513) == UNS
    assert conv(Cin=513, K=7) == INV                                                      # the first group is judged first
    assert conv(N=0, x=None) == conv(H=6, w=None) == OK                                   # empty: H + 2p < K gives no output pixel
    assert conv(x=None) == conv(w=None) == conv(y=None) == conv(w=odd) == INV
    assert L.gh_conv2d_weight_floats(3, 64, 11) == 128 * 364 and L.gh_conv2d_weight_floats(192, 384, 3) == 384 * 1728
    assert L.gh_conv2d_weight_floats(3, 64, 7) == L.gh_conv2d_weight_floats(0, 4, 3) == L.gh_conv2d_weight_floats(4, 513, 3) == 0

    pool = lambda N=1, H=7, W=7, Cn=4, x=one, y=one: L.gh_maxpool3x3s2_forward(x, N, H, W, Cn, y, None)
    assert pool(N=-1) == pool(Cn=0) == INV and pool(Cn=513) == UNS
    assert pool(H=2, x=None, y=None) == pool(N=0, x=None) == OK
    assert pool(x=None) == pool(y=None) == pool(y=odd) == INV

    def layer(N=1, P=9, Cn=7, f=one, lin=one, score=one, term=None, ws=one, nbytes=1 << 12):
        return L.gh_lpips_layer(f, N, P, Cn, lin, 0, score, term, ws, nbytes, None)

    assert layer(N=-1) == layer(P=-1) == layer(Cn=0) == INV and layer(Cn=513) == UNS
    assert layer(N=0, f=None) == layer(P=0, f=None, score=None) == OK
    assert layer(f=None) == layer(lin=None) == layer(score=None) == layer(ws=None) == layer(score=four) == layer(term=four) == INV
    assert layer(nbytes=0) == INV and L.gh_lpips_layer_workspace(2, 257) == 256 and L.gh_lpips_layer_workspace(-1, 4) == 0

    def prep(N=1, H=40, W=40, h=31, w=32, flags=0, pred=one, gt=one, shift=one, x=one):
        return L.gh_lpips_prepare(pred, gt, None, None, N, H, W, h, w, flags, shift, one, x, None)

    assert prep(N=-1) == prep(h=-1) == prep(flags=16) == prep(flags=_abi.GH_LPIPS_QUANTIZE | _abi.GH_LPIPS_SIGNED) == prep(h=41) == prep(w=41) == INV
    assert prep(N=0, pred=None) == prep(h=0, x=None) == OK
    assert prep(pred=None) == prep(gt=None) == prep(shift=None) == prep(x=None) == prep(x=odd) == INV

    wts = _abi.GhLpipsWeights()
    for l in range(5):
        wts.w[l] = wts.b[l] = wts.lin[l] = one.value
    widths = lambda *w: (C.c_int * 5)(*w)
    small = widths(*LC.SMALL)
    nbytes = L.gh_lpips_workspace(2, 35, 32, small)
    assert nbytes > 0 and L.gh_lpips_workspace(2, 30, 40, small) == 0 and L.gh_lpips_workspace(2, 35, 32, widths(8, 0, 8, 8, 8)) == 0

    def fwd(N=2, h=35, w=32, wd=small, wt=C.byref(wts), x=one, scores=one, terms=None, ws=one, nb=nbytes):
        return L.gh_lpips_forward(x, N, h, w, wd, wt, scores, terms, ws, nb, None)

    assert fwd(N=-1) == fwd(wd=widths(8, 0, 8, 8, 8)) == fwd(wt=None) == fwd(wd=None) == INV
    assert fwd(wd=widths(8, 513, 8, 8, 8)) == fwd(h=30) == fwd(w=30) == UNS
    assert fwd(N=0, x=None) == OK
    assert fwd(x=None) == fwd(scores=None) == fwd(ws=None) == fwd(scores=four) == fwd(terms=four) == fwd(nb=nbytes - 1) == INV
    bad = _abi.GhLpipsWeights()
    assert fwd(wt=C.byref(bad)) == INV
