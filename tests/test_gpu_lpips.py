"""guassianhand_amd.lpips on the device: the dense convolution, the 3x3 stride-2 pooling, LPIPS' head, the whole chain, the evaluator's
protocol and the Evaluator's fourth number (include/gh_lpips.h).

Values are held to tests/res_block_cases.three_way — max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64| — with the float64
restatement on the CPU and the float32 torch statements (ops="torch") on the device, all on the same inputs. Every head and
end-to-end case first asserts tests/lpips_cases.norm_guard on its float64 reference. What the header promises bit for bit (the pooling
against F.max_pool2d, chunk and batch independence, run-to-run equality, the zero of identical inputs, the swap symmetry, a graph
replay) is compared with torch.equal."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_cases as LC
from tests.res_block_cases import three_way

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def LP():
    from guassianhand_amd import lpips
    return lpips


@pytest.fixture(scope="module")
def small(dev):
    """The small network on the CPU and on the device, and one pair of 35x32 images: shared, never written."""
    cpu = LC.make_net(LC.SMALL, 0)
    x0, x1 = LC.make_images(3, 35, 32, 0)
    return cpu, LC.make_net(LC.SMALL, 0).to(dev), x0, x1


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.CONV_CASES, ids=LC.case_id)
def test_conv_three_way_and_every_chunk_bitwise(dev, LP, case):
    Cin, Cout, K, s, p, N, H, W = case
    x, w, b = LC.make_conv(case)
    f64 = LP.conv2d_ref(x, w, b, s, p, relu=True, acc=torch.float64)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    packed = LP.pack_conv(wd)
    runs = [LP.conv2d(xd, wd, bd, s, p, relu=True, packed=packed, chunk=ch) for ch in LC.CHUNKS]
    torch32 = LP.conv2d(xd, wd, bd, s, p, relu=True, ops="torch")
    assert runs[0].shape == f64.shape and runs[0].is_contiguous()
    three_way({"y": runs[0].cpu()}, {"y": torch32.cpu()}, {"y": f64}, fields=("y",), tag=f"conv {LC.case_id(case)}")
    for ch, y in zip(LC.CHUNKS[1:], runs[1:]):
        assert torch.equal(y, runs[0]), ch
    lin = LP.conv2d(xd, wd, None, s, p, relu=False, packed=packed)                          # no bias, no ReLU
    three_way({"y": lin.cpu()}, {"y": LP.conv2d(xd, wd, None, s, p, ops="torch").cpu()}, {"y": LP.conv2d_ref(x, w, None, s, p, acc=torch.float64)},
              fields=("y",), tag=f"conv {LC.case_id(case)} linear")


def test_conv_does_not_depend_on_the_position_in_the_batch(dev, LP):
    """An image alone against the same image as element 1 of a batch of 3: its pixels then start mid-tile. Both reduction orders."""
    for case in (LC.CONV_CASES[1], LC.CONV_CASES[6], LC.CONV_CASES[2]):
        Cin, Cout, K, s, p, _, H, W = case
        x, w, b = (t.to(dev) for t in LC.make_conv(case[:5] + (3, H, W)))
        alone = LP.conv2d(x[1:2], w, b, s, p, relu=True)
        assert torch.equal(alone[0], LP.conv2d(x, w, b, s, p, relu=True)[1]), case


def test_conv_padding_tap_equals_an_explicit_zero_pixel(dev, LP):
    """fmaf(w, 0, acc) for a tap in the padding: the bits an explicitly padded image gives with padding 0."""
    for case in (LC.CONV_CASES[3], LC.CONV_CASES[6]):
        Cin, Cout, K, s, p, N, H, W = case
        x, w, b = (t.to(dev) for t in LC.make_conv(case))
        xp = F.pad(x, (0, 0, p, p, p, p))
        assert torch.equal(LP.conv2d(x, w, b, s, p), LP.conv2d(xp, w, b, s, 0)), case


# ---- pooling -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", LC.POOL_CHANNELS)
@pytest.mark.parametrize("shape", LC.POOL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_is_max_pool2d_bitwise(dev, LP, shape, C):
    x = LC.make_pool(shape, C)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    got = LP.max_pool3x3s2(x.to(dev)).cpu()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want).any())
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
    assert bool((want[1, 0, 0] == float("-inf")).all())                                     # the window of -inf stays -inf


# ---- the head -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", LC.HEAD_CHANNELS)
def test_head_three_way(dev, LP, C):
    f, lin = LC.make_head(C)
    LC.norm_guard(LC.head_norms(f), f"head C={C}")
    assert float(lin.min()) == 0.0 and float(f[0, 0, 0].abs().max()) == 0.0 and float(f[2, 0, 0].abs().max()) == 0.0
    assert float(f[1, 1, 2].abs().max()) == 0.0 and float(f[3, 1, 2].abs().max()) > 0.0
    f64 = LP.lpips_layer_ref(f, lin, acc=torch.float64)
    kernel = LP.lpips_layer(f.to(dev), lin.to(dev))
    assert kernel.dtype == torch.float64
    torch32 = LP.lpips_layer(f.to(dev), lin.to(dev), ops="torch")
    three_way({"d": kernel.cpu()}, {"d": torch32.cpu()}, {"d": f64}, fields=("d",), tag=f"head C={C}")
    same = torch.cat([f[:2], f[:2]]).to(dev)
    assert torch.equal(LP.lpips_layer(same, lin.to(dev)), torch.zeros(2, dtype=torch.float64, device=dev))
    swapped = torch.cat([f[2:], f[:2]]).to(dev)
    assert torch.equal(LP.lpips_layer(swapped, lin.to(dev)), kernel)


def test_head_sums_many_workgroups_in_order(dev, LP):
    """70 x 60 = 4200 pixels: 17 workgroups per pair, the last partial; against float64 and bit for bit against itself in another slot."""
    f, lin = LC.make_head(64, seed=1, N=2, h=70, w=60)
    LC.norm_guard(LC.head_norms(f), "head 70x60")
    kernel = LP.lpips_layer(f.to(dev), lin.to(dev))
    three_way({"d": kernel.cpu()}, {"d": LP.lpips_layer(f.to(dev), lin.to(dev), ops="torch").cpu()},
              {"d": LP.lpips_layer_ref(f, lin, acc=torch.float64)}, fields=("d",), tag="head 70x60")
    alone = LP.lpips_layer(torch.stack([f[1], f[3]]).to(dev), lin.to(dev))
    assert torch.equal(alone[0], kernel[1])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.E2E_CASES, ids=LC.case_id)
def test_distance_three_way_with_terms(dev, LP, case):
    widths, N, H, W, seed = case
    net, (x0, x1) = LC.make_net(widths, seed), LC.make_images(N, H, W, seed)
    LC.norm_guard(LC.tap_norms(net, x0, x1), LC.case_id(case))
    d64, t64 = LP.lpips_ref(net, x0, x1, acc=torch.float64, terms=True)
    nd = LC.make_net(widths, seed).to(dev)
    dk, tk = LP.lpips_distance(nd, x0.to(dev), x1.to(dev), terms=True)
    dt, tt = LP.lpips_distance(nd, x0.to(dev), x1.to(dev), ops="torch", terms=True)
    assert dk.dtype == torch.float64 and dk.shape == (N,) and tk.shape == (5, N)
    three_way({"lpips": dk.cpu(), "terms": tk.cpu()}, {"lpips": dt.cpu(), "terms": tt.cpu()}, {"lpips": d64, "terms": t64},
              fields=("lpips", "terms"), tag=LC.case_id(case))
    assert torch.equal(dk, (((tk[0] + tk[1]) + tk[2]) + tk[3]) + tk[4])


def test_fused_path_launches_the_kernels(dev, LP, small, monkeypatch):
    _, nd, x0, x1 = small
    seen = []
    real = LP.launch
    monkeypatch.setattr(LP, "launch", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    LP.lpips_distance(nd, x0.to(dev), x1.to(dev))
    assert seen == ["gh_lpips_prepare", "gh_lpips_forward"]
    seen.clear()
    LP.lpips_distance(nd, x0.to(dev), x1.to(dev), ops="torch")
    assert seen == []


def test_properties_bit_for_bit(dev, LP, small):
    _, nd, x0, x1 = small
    a, b = x0.to(dev), x1.to(dev)
    d = LP.lpips_distance(nd, a, b)
    assert torch.equal(LP.lpips_distance(nd, a, a.clone()), torch.zeros(3, dtype=torch.float64, device=dev))   # identical inputs: exactly 0
    assert torch.equal(LP.lpips_distance(nd, b, a), d)                                                           # the swap
    assert torch.equal(LP.lpips_distance(nd, a, b), d)                                                           # run to run
    assert float(d.min()) > 0
    pair = LP.lpips_distance(nd, a[1:2], b[1:2])                                                                 # alone ...
    batch = LP.lpips_distance(nd, torch.stack([a[1], a[0], a[1]]), torch.stack([b[1], b[0], b[1]]))              # ... and in slots 0 and 2 of 3
    assert torch.equal(pair[0], batch[0]) and torch.equal(pair[0], batch[2]) and torch.equal(pair[0], d[1])


def test_graph_replay_equals_eager(dev, LP, small):
    _, nd, x0, x1 = small
    a, b = x0.to(dev), x1.to(dev)
    eager = LP.lpips_distance(nd, a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        LP.lpips_distance(nd, a, b)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = LP.lpips_distance(nd, a, b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, eager)
    b.copy_(a)                                                        # new inputs in the same buffers: the replay follows them
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, torch.zeros_like(c))


# ---- the evaluator's protocol -----------------------------------------------------------------------------------------------------------
def _views(seed=0):
    """Nv = 3 views of 48x52 in [0, 1] and a little beyond: crops of 35x38 and 34x38 (two sizes) and one of 30x40 (under 31)."""
    g = torch.Generator().manual_seed(7400 + seed)
    Nv, H, W = 3, 48, 52
    pred, gt = torch.rand(Nv, 3, H, W, generator=g) * 1.2 - 0.1, torch.rand(Nv, 3, H, W, generator=g)
    mask = torch.zeros(Nv, H, W)
    mask[0, 5:40, 7:45] = 1
    mask[1, 2, 3] = mask[1, 35, 40] = 1
    mask[2, 10:40, 4:44] = 1
    bbm = (torch.rand(Nv, H, W, generator=g) > 0.3).float()
    return pred, gt, mask, bbm


@pytest.mark.parametrize("quantize", (True, False), ids=("q8", "raw"))
@pytest.mark.parametrize("with_bbm", (False, True), ids=("nomask", "bbm"))
@pytest.mark.parametrize("layout", ("chw", "hwc", "hwc-view"))
def test_scores_against_the_cpu_path(dev, LP, small, layout, with_bbm, quantize):
    cpu, nd, _, _ = small
    pred, gt, mask, bbm = _views()
    bb = bbm if with_bbm else None
    f32 = LP.lpips_scores(cpu, pred, gt, mask, bbox_mask=bb, quantize=quantize)             # the CPU path: torch float32
    f64 = _scores_f64(LP, cpu, pred, gt, bb, quantize)
    pd, gd = pred.to(dev), gt.to(dev)
    if layout == "hwc":
        pd, gd, lay = pd.permute(0, 2, 3, 1).contiguous(), gd.permute(0, 2, 3, 1).contiguous(), "hwc"
    elif layout == "hwc-view":
        pd, gd, lay = pd.permute(0, 2, 3, 1), gd.permute(0, 2, 3, 1), "hwc"                # the channel-last view of a channel-first image
    else:
        lay = "chw"
    keep = (pd.clone(), gd.clone())
    got = LP.lpips_scores(nd, pd, gd, mask.to(dev), bbox_mask=None if bb is None else bb.to(dev), layout=lay, quantize=quantize)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and got.shape == (3,)
    assert math.isnan(float(got[2])) and math.isnan(float(f32[2]))
    three_way({"s": got[:2].cpu()}, {"s": f32[:2]}, {"s": f64}, fields=("s",), tag=f"scores {layout} bbm={with_bbm} q={quantize}")
    assert torch.equal(pd, keep[0]) and torch.equal(gd, keep[1])


def _scores_f64(LP, net, pred, gt, bbm, quantize):
    """The protocol of the two scored views in float64 from the float32 network inputs (the quantiser's output is float32 by its
    definition; everything after it is float64)."""
    out = []
    for v, (bx, by, bw, bh) in enumerate([(7, 5, 38, 35), (3, 2, 38, 34)]):
        p, g = pred[v:v + 1, :, by:by + bh, bx:bx + bw], gt[v:v + 1, :, by:by + bh, bx:bx + bw]
        if bbm is not None:
            p = torch.where(bbm[v:v + 1, None, by:by + bh, bx:bx + bw] != 0, p, torch.zeros(()))
        out.append(LP.lpips_ref(net, LP.quantize_unit(p, quantize), LP.quantize_unit(g, quantize), acc=torch.float64)[0])
    return torch.stack(out)


def test_scores_guard_of_the_views(LP, small):
    """The norm guard of the crops the scores tests compare (on the float64 reference alone)."""
    cpu = small[0]
    pred, gt, _, bbm = _views()
    for quantize in (True, False):
        for bb in (None, bbm):
            for v, (bx, by, bw, bh) in enumerate([(7, 5, 38, 35), (3, 2, 38, 34)]):
                p, g = pred[v:v + 1, :, by:by + bh, bx:bx + bw], gt[v:v + 1, :, by:by + bh, bx:bx + bw]
                if bb is not None:
                    p = torch.where(bb[v:v + 1, None, by:by + bh, bx:bx + bw] != 0, p, torch.zeros(()))
                LC.norm_guard(LC.tap_norms(cpu, LP.quantize_unit(p, quantize), LP.quantize_unit(g, quantize)), f"view {v} q={quantize} bbm={bb is not None}")


def test_scores_nan_input_and_whole_image(dev, LP, small):
    cpu, nd, _, _ = small
    pred, gt, mask, _ = _views()
    LC.norm_guard(LC.tap_norms(cpu, LP.quantize_unit(pred), LP.quantize_unit(gt)), "whole image")
    whole = LP.lpips_scores(nd, pred.to(dev), gt.to(dev))                                  # no mask: the whole 48x52 image, one group of 3
    three_way({"s": whole.cpu()}, {"s": LP.lpips_scores(cpu, pred, gt)},
              {"s": LP.lpips_ref(cpu, LP.quantize_unit(pred), LP.quantize_unit(gt), acc=torch.float64)}, fields=("s",), tag="whole image")
    bad = pred.clone()
    bad[0, 1, 20, 20] = float("nan")
    got = LP.lpips_scores(nd, bad.to(dev), gt.to(dev), mask.to(dev))
    assert math.isnan(float(got[0])) and not math.isnan(float(got[1]))                      # a NaN makes that view's score NaN, no other


def test_prepare_refuses_a_view_of_another_size_with_nan(dev, LP, small):
    """A view whose device box disagrees with the host's crop size, or does not lie in the image, gets NaN inputs and reads nothing."""
    _, nd, _, _ = small
    pred, gt, _, _ = _views()
    bbox = torch.tensor([[7, 5, 38, 35], [3, 2, 38, 34], [20, 5, 38, 35]], dtype=torch.int32, device=dev)   # 20 + 38 > 52
    x = LP.prepare_input(pred.to(dev), gt.to(dev), bbox, (35, 38), shift=nd.shift, scale=nd.scale)
    assert x.shape == (6, 35, 38, 3)
    assert not bool(torch.isnan(x[0]).any()) and not bool(torch.isnan(x[3]).any())
    assert bool(torch.isnan(x[[1, 2, 4, 5]]).all())
    q = LP.quantize_unit(pred[0, :, 5:40, 7:45]).permute(1, 2, 0)
    assert torch.equal(x[0].cpu(), (q - cpu_t(nd.shift)) / cpu_t(nd.scale))


def cpu_t(t):
    return t.detach().cpu()


def test_prepare_quantises_ties_infinities_and_nan_as_quantize_unit_does(dev, LP, small):
    """The device quantiser on the values that tell rounding rules apart: every float32 v with v * 255 exactly a half (ties to even),
    values outside [0, 1], both infinities, a NaN and the 8-bit grid, bit for bit against quantize_unit, with and without rounding."""
    _, nd, _, _ = small
    v = LC.quantiser_values()
    n = v.numel()
    H, W = 12, -(-n // 12)
    img = torch.full((3 * H * W,), 0.25)
    img[:n], img[H * W:H * W + n], img[2 * H * W + 5:2 * H * W + 5 + n] = v, v.flip(0), v      # the three channels see them at other pixels
    img = img.view(1, 3, H, W)
    gt = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1))
    for quantize in (True, False):
        x = LP.prepare_input(img.to(dev), gt.to(dev), None, (H, W), quantize=quantize, shift=nd.shift, scale=nd.scale).cpu()
        for member, src in ((0, img), (1, gt)):
            want = ((LP.quantize_unit(src[0], quantize).permute(1, 2, 0) - cpu_t(nd.shift)) / cpu_t(nd.scale))
            assert torch.equal(torch.isnan(x[member]), torch.isnan(want)) and int(torch.isnan(want).sum()) == (3 if member == 0 else 0)
            assert torch.equal(torch.nan_to_num(x[member], nan=7.0), torch.nan_to_num(want, nan=7.0)), (quantize, member)


def test_views_of_one_size_that_are_not_one_run_are_gathered(dev, LP, small):
    """Views 0 and 2 share a crop size and view 1 has another: the gather branch (index_select, index_copy_), bit for bit against each
    view scored alone, with a bbox_mask and in both layouts."""
    _, nd, _, _ = small
    pred, gt, mask, bbm = _views()
    mask[2] = 0
    mask[2, 9:44, 11:49] = 1                                          # 38 wide, 35 high, as view 0, at another origin
    pd, gd, md, bd = pred.to(dev), gt.to(dev), mask.to(dev), bbm.to(dev)
    seen = []
    real = LP.launch
    try:
        LP.launch = lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1]
        got = LP.lpips_scores(nd, pd, gd, md, bbox_mask=bd)
    finally:
        LP.launch = real
    assert seen == ["gh_lpips_prepare", "gh_lpips_forward"] * 2        # two sizes, one chain each
    assert not bool(torch.isnan(got).any())
    for v in range(3):
        alone = LP.lpips_scores(nd, pd[v:v + 1], gd[v:v + 1], md[v:v + 1], bbox_mask=bd[v:v + 1])
        assert torch.equal(alone[0], got[v]), v
    hwc = LP.lpips_scores(nd, pd.permute(0, 2, 3, 1), gd.permute(0, 2, 3, 1).contiguous(), md, bbox_mask=bd, layout="hwc")
    assert torch.equal(hwc, got)


def test_tensors_on_another_device_or_of_another_dtype_are_refused_before_any_launch(dev, LP, small, monkeypatch):
    """A network left on the CPU with device images, and every single-kernel entry point handed a CPU or wrongly typed tensor:
    ValueError on the host, nothing launched. A float64 network on the device runs the torch statements."""
    from guassianhand_amd.metrics import Evaluator
    cpu, nd, x0, x1 = small
    launched = []
    real = LP.launch
    monkeypatch.setattr(LP, "launch", lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    a, b = x0.to(dev), x1.to(dev)
    pred, gt, mask, bbm = (t.to(dev) for t in _views())
    for call in (lambda: LP.lpips_distance(cpu, a, b), lambda: LP.lpips_scores(cpu, pred, gt, mask), lambda: LP.lpips_scores(cpu, pred, gt),
                 lambda: Evaluator(lpips=cpu).compute_score(pred[:1], gt[:1], mask_at_box=mask[:1]),
                 lambda: Evaluator(lpips=LP.AlexLPIPS(LC.SMALL)).compute_score(pred[:1], gt[:1], mask_at_box=mask[:1])):
        with pytest.raises(ValueError, match="is on cpu"):
            call()
    x, w, bias = LC.make_conv(LC.CONV_CASES[6])
    f, lin = LC.make_head(7)
    bbox = torch.tensor([[7, 5, 38, 35]] * 3, dtype=torch.int32, device=dev)
    prep = lambda **kw: LP.prepare_input(pred, gt, kw.pop("bbox", bbox), (35, 38), **{"shift": nd.shift, "scale": nd.scale, **kw})
    for call in (lambda: LP.conv2d(x.to(dev), w, bias.to(dev), 1, 1), lambda: LP.conv2d(x.to(dev), w.to(dev), bias, 1, 1),
                 lambda: LP.conv2d(x.to(dev), w.to(dev), None, 1, 1, packed=LP.pack_conv(w)), lambda: LP.conv2d(x.to(dev), w.to(dev).double(), None, 1, 1),
                 lambda: LP.lpips_layer(f.to(dev), lin), lambda: LP.lpips_layer(f.to(dev), lin.to(dev).double()),
                 lambda: prep(bbox=bbox.cpu()), lambda: prep(bbox=bbox.long()), lambda: prep(bbox_mask=bbm), lambda: prep(bbox_mask=bbm.cpu().to(torch.uint8)),
                 lambda: prep(shift=cpu.shift), lambda: prep(scale=nd.scale.double()), lambda: LP.prepare_input(pred, gt.cpu(), bbox, (35, 38), shift=nd.shift, scale=nd.scale)):
        with pytest.raises(ValueError):
            call()
    assert launched == []
    n64 = LC.make_net(LC.SMALL, 0).to(dev).double()
    d = LP.lpips_distance(n64, a, b)                                   # float64 parameters: the torch statements, in the images' dtype
    assert launched == [] and d.dtype == torch.float64 and d.shape == (3,)
    assert float((d - LP.lpips_distance(nd, a, b)).abs().max()) <= 1e-5
    assert launched == ["gh_lpips_prepare", "gh_lpips_forward"]


def test_evaluator_with_a_net_returns_four_floats_that_match_the_cpu_call(dev, LP, small):
    from guassianhand_amd.metrics import Evaluator
    cpu, nd, _, _ = small
    pred, gt, mask, _ = _views()
    want = Evaluator(lpips=cpu).compute_score(pred[:1], gt[:1], mask_at_box=mask[:1])
    got = Evaluator(lpips=nd).compute_score(pred[:1].to(dev), gt[:1].to(dev), mask_at_box=mask[:1].to(dev))
    assert sorted(got) == ["lpips", "mse", "psnr", "ssim"] and all(isinstance(v, float) for v in got.values())
    f64 = _scores_f64(LP, cpu, pred, gt, None, True)[:1]
    three_way({"s": torch.tensor([got["lpips"]], dtype=torch.float64)}, {"s": torch.tensor([want["lpips"]], dtype=torch.float64)}, {"s": f64},
              fields=("s",), tag="Evaluator lpips")
    assert abs(got["mse"] - want["mse"]) <= 1e-6 * want["mse"] and abs(got["psnr"] - want["psnr"]) <= 1e-4      # test_gpu_metrics' bounds
    assert abs(got["ssim"] - want["ssim"]) <= 1e-6
    assert sorted(Evaluator().compute_score(pred[:1].to(dev), gt[:1].to(dev), mask_at_box=mask[:1].to(dev))) == ["mse", "psnr", "ssim"]
    with pytest.raises(ValueError, match="31"):
        Evaluator(lpips=nd).compute_score(pred[2:].to(dev), gt[2:].to(dev), mask_at_box=mask[2:].to(dev))
