"""metrics.image_scores / metrics.Evaluator on CPU tensors (the float64 restatement the GPU tests compare against), and the
C-ABI surface of include/gh_metrics.h (argument checks only, nothing is launched)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd.metrics import Evaluator, image_scores
from tests.helpers import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full(n, h, w):
    return torch.ones(n, h, w, dtype=torch.uint8)


def test_identical_images_score_perfectly():
    g = torch.Generator().manual_seed(1)
    a = torch.rand(2, 3, 24, 31, generator=g)
    s = image_scores(a, a.clone(), _full(2, 24, 31))
    assert torch.equal(s.mse, torch.zeros(2, dtype=torch.float64))
    assert torch.isinf(s.psnr).all() and (s.psnr > 0).all()
    assert torch.allclose(s.ssim, torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-15)
    assert s.mse.dtype == s.psnr.dtype == s.ssim.dtype == torch.float64 and s.bbox.dtype == torch.int32


@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.0, 1.0), (0.5, 0.5), (0.9, 0.1)])
def test_constant_images_give_the_closed_form(a, b):
    pa, pb = torch.full((1, 3, 16, 12), a), torch.full((1, 3, 16, 12), b)
    s = image_scores(pa, pb, _full(1, 16, 12))
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    C1 = (0.01 * 2.0) ** 2                                     # R = 2 by default: the variances vanish, the C2 factor is 1
    want = (2 * a32 * b32 + C1) / (a32 ** 2 + b32 ** 2 + C1)
    assert abs(s.ssim.item() - want) < 1e-12
    assert abs(s.mse.item() - (a32 - b32) ** 2) < 1e-15


def test_data_range_defaults_to_two_and_can_be_overridden():
    pa, pb = torch.full((1, 3, 9, 9), 0.25), torch.full((1, 3, 9, 9), 0.5)
    m = _full(1, 9, 9)
    d = image_scores(pa, pb, m).ssim.item()
    assert d == image_scores(pa, pb, m, data_range=2.0).ssim.item()
    one = image_scores(pa, pb, m, data_range=1).ssim.item()
    closed = lambda R: (2 * 0.25 * 0.5 + (0.01 * R) ** 2) / (0.25 ** 2 + 0.5 ** 2 + (0.01 * R) ** 2)
    assert abs(d - closed(2.0)) < 1e-12 and abs(one - closed(1.0)) < 1e-12 and one < d
    with pytest.raises(ValueError):
        image_scores(pa, pb, m, data_range=0.0)


def _brute_rect(m):
    """cv2.boundingRect by a scan of every pixel."""
    H, W = m.shape
    xs = [x for y in range(H) for x in range(W) if m[y, x]]
    ys = [y for y in range(H) for x in range(W) if m[y, x]]
    if not xs:
        return [0, 0, 0, 0]
    return [min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1]


def _mask_cases(H, W):
    g = torch.Generator().manual_seed(5)
    full = torch.ones(H, W, dtype=torch.uint8)
    empty = torch.zeros(H, W, dtype=torch.uint8)
    single = torch.zeros(H, W, dtype=torch.uint8)
    single[H // 3, W // 2] = 1
    border = torch.zeros(H, W, dtype=torch.uint8)
    border[0, W - 3:] = 1                                      # touches the top and the right edge
    border[H - 1, 2] = 1                                       # and the bottom one
    blob = (torch.rand(H, W, generator=g) > 0.97).to(torch.uint8)
    return {"full": full, "empty": empty, "single": single, "border": border, "blob": blob}


def test_bbox_matches_a_brute_force_scan():
    H, W = 19, 23
    cases = _mask_cases(H, W)
    m = torch.stack(list(cases.values()))
    img = torch.rand(len(cases), 3, H, W)
    s = image_scores(img, img, m)
    for i, (name, mk) in enumerate(cases.items()):
        assert s.bbox[i].tolist() == _brute_rect(mk.numpy()), name
    assert s.bbox[1].tolist() == [0, 0, 0, 0]
    assert s.bbox[0].tolist() == [0, 0, W, H]


def test_crop_smaller_than_seven_gives_nan_and_evaluator_raises():
    H, W = 20, 20
    m = torch.zeros(2, H, W, dtype=torch.uint8)
    m[0, 4:10, 2:15] = 1                                       # 13 x 6
    m[1, 3:10, 5:12] = 1                                       # 7 x 7: the smallest that scores
    a = torch.rand(2, 3, H, W)
    b = torch.rand(2, 3, H, W)
    s = image_scores(a, b, m)
    assert math.isnan(s.ssim[0].item()) and math.isfinite(s.ssim[1].item())
    assert s.bbox[0].tolist() == [2, 4, 13, 6]
    with pytest.raises(ValueError):
        Evaluator().compute_score(a[:1], b[:1], None, m[:1], "0", "0", "0")
    with pytest.raises(ValueError):
        Evaluator().compute_score(a[:1], b[:1], None, torch.zeros(1, H, W), "0", "0", "0")   # empty mask
    r = Evaluator().compute_score(a[1:], b[1:], None, m[1:], "0", "0", "0")
    assert abs(r["ssim"] - s.ssim[1].item()) < 1e-15 and set(r) == {"mse", "psnr", "ssim"}


def _ssim_loops(x, y, R):
    """skimage 0.16 structural_similarity(multichannel=True), restated as a loop over the windows: x, y (h,w,3) float64."""
    h, w, _ = x.shape
    C1, C2, cov = (0.01 * R) ** 2, (0.03 * R) ** 2, 49.0 / 48.0
    means = []
    for c in range(3):
        acc = []
        for i in range(3, h - 3):
            for j in range(3, w - 3):
                a, b = x[i - 3:i + 4, j - 3:j + 4, c], y[i - 3:i + 4, j - 3:j + 4, c]
                ux, uy = a.mean(), b.mean()
                vx, vy = cov * ((a * a).mean() - ux * ux), cov * ((b * b).mean() - uy * uy)
                vxy = cov * ((a * b).mean() - ux * uy)
                acc.append((2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)))
        means.append(np.mean(acc))
    return float(np.mean(means))


def _reference_scores(pred_hwc, gt_hwc, mask, bbox_mask=None, R=2.0):
    """Steps 1-4 of the reference's test_step / compute_score in numpy, one view: pred / gt (H,W,3) float32."""
    pred = pred_hwc.copy()
    if bbox_mask is not None:
        pred[bbox_mask == 0] = 0
    mse = float(np.mean((pred.astype(np.float64) - gt_hwc.astype(np.float64)) ** 2))
    x, y, w, h = _brute_rect(mask.astype(np.uint8))
    ssim = _ssim_loops(pred[y:y + h, x:x + w].astype(np.float64), gt_hwc[y:y + h, x:x + w].astype(np.float64), R)
    return mse, ssim, [x, y, w, h]


@pytest.mark.parametrize("seed", range(4))
def test_random_crops_match_a_loop_over_windows(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(12, 22)), int(rng.integers(12, 22))
    gt = rng.random((2, H, W, 3), dtype=np.float32)
    pred = np.clip(gt + rng.normal(0, 0.1, gt.shape), 0, 1).astype(np.float32)
    mask = np.zeros((2, H, W), np.uint8)
    bb = (rng.random((2, H, W)) > 0.2).astype(np.float32)
    for v in range(2):
        y0, x0 = int(rng.integers(0, H - 9)), int(rng.integers(0, W - 9))
        mask[v, y0:y0 + int(rng.integers(7, H - y0 + 1)), x0:x0 + int(rng.integers(7, W - x0 + 1))] = 1
    s = image_scores(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(mask), bbox_mask=torch.from_numpy(bb),
                     layout="hwc")
    for v in range(2):
        mse, ssim, box = _reference_scores(pred[v], gt[v], mask[v], bb[v])
        assert s.bbox[v].tolist() == box
        assert abs(s.ssim[v].item() - ssim) < 1e-12
        assert abs(s.mse[v].item() - mse) <= 1e-12 * mse
        assert abs(s.psnr[v].item() + 10 * math.log10(mse)) < 1e-9
    # the same views, channel-first, give the same numbers
    c = image_scores(torch.from_numpy(pred).permute(0, 3, 1, 2), torch.from_numpy(gt).permute(0, 3, 1, 2), torch.from_numpy(mask),
                     bbox_mask=torch.from_numpy(bb), layout="chw")
    for k in ("mse", "psnr", "ssim", "bbox"):
        assert torch.equal(getattr(c, k), getattr(s, k)), k


def test_masks_are_converted_the_reference_way():
    """mask_at_box goes through .astype(np.uint8) (0.5 -> 0); bbox_mask is compared with 0 in its own dtype (0.5 keeps the pixel);
    a trailing channel of 3 is sliced to [..., 0]."""
    H, W = 12, 12
    a, b = torch.rand(1, 3, H, W), torch.rand(1, 3, H, W)
    m = torch.zeros(1, H, W)
    m[0, 1:10, 2:11] = 1.0
    m[0, 0, 0] = 0.5                                           # cast to uint8 0: not part of the box
    s = image_scores(a, b, m)
    assert s.bbox[0].tolist() == [2, 1, 9, 9]
    half = torch.full((1, H, W), 0.5)
    assert torch.equal(image_scores(a, b, m, bbox_mask=half).mse, s.mse)
    bb = torch.ones(1, H, W, 3)
    bb[0, :, :6, 0] = 0
    s2 = image_scores(a, b, m, bbox_mask=bb)
    a0 = a.clone()
    a0[:, :, :, :6] = 0
    assert torch.equal(s2.mse, image_scores(a0, b, m).mse)


def test_evaluator_is_a_drop_in():
    ev = Evaluator()
    assert ev.result_dir is None
    ev.result_dir = "/nonexistent"                             # set by the reference's test_step; never used
    H, W = 16, 14
    a, b = torch.rand(1, 3, H, W), torch.rand(1, 3, H, W)
    m = torch.ones(1, H, W)
    r = ev.compute_score(a, b, input_imgs=torch.rand(1, H, W, 3), mask_at_box=m, human_idx="3", frame_index="0", view_index="1",
                         ka_xy=None, vert_vis=None)
    s = image_scores(a, b, m)
    assert r == {"mse": s.mse.item(), "psnr": s.psnr.item(), "ssim": s.ssim.item()}
    assert all(type(v) is float for v in r.values())
    assert not os.path.exists("/nonexistent")


def test_skimage_agrees_if_installed():
    skm = pytest.importorskip("skimage.metrics")
    rng = np.random.default_rng(3)
    x = rng.random((20, 17, 3)).astype(np.float32)
    y = np.clip(x + rng.normal(0, 0.05, x.shape), 0, 1).astype(np.float32)
    try:
        want = skm.structural_similarity(x, y, multichannel=True, data_range=2.0)
    except TypeError:                                          # newer scikit-image: channel_axis
        want = skm.structural_similarity(x, y, channel_axis=-1, data_range=2.0)
    s = image_scores(torch.from_numpy(x)[None], torch.from_numpy(y)[None], torch.ones(1, 20, 17), layout="hwc")
    assert abs(s.ssim.item() - want) < 1e-9


# ---- C-ABI (include/gh_metrics.h) -----------------------------------------------------------------------------------------------
def test_metrics_header_declares_the_metrics_symbols():
    assert header_symbols("gh_metrics.h") == sorted(_abi.METRICS_SYMBOLS)
    assert not set(_abi.METRICS_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "gh_metrics.h")).read()
    for name in ("GH_METRICS_CHW", "GH_METRICS_PRED_HWC", "GH_METRICS_GT_HWC"):
        assert getattr(_abi, name) == int(re.search(rf"#define {name} (\d+)u", h).group(1)), name


def test_metrics_arguments_are_validated_before_any_launch(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    _abi.declare_metrics(L)
    n = L.gh_image_scores_workspace(8, 512, 334)
    assert n > 0 and n % 256 == 0 and L.gh_image_scores_workspace(8, 1024, 1024) > n
    assert L.gh_image_scores_workspace(0, 16, 16) == 0 and L.gh_image_scores_workspace(1, 0, 16) == 0
    one, two, three = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    call = lambda pred=one, gt=two, m=three, layout=0, R=2.0, nv=1, h=16, w=16, scores=one, ws=three, nbytes=1 << 30: \
        L.gh_image_scores(pred, gt, m, None, nv, h, w, layout, R, scores, two, ws, nbytes, None)
    assert call(pred=None) == _abi.GH_ERR_INVALID_ARG
    assert call(m=None) == _abi.GH_ERR_INVALID_ARG
    assert call(ws=None) == _abi.GH_ERR_INVALID_ARG
    assert call(nv=0) == _abi.GH_ERR_INVALID_ARG
    assert call(layout=4) == _abi.GH_ERR_INVALID_ARG
    assert call(R=0.0) == _abi.GH_ERR_INVALID_ARG and call(R=float("nan")) == _abi.GH_ERR_INVALID_ARG
    assert call(pred=C.c_void_p((1 << 20) + 2)) == _abi.GH_ERR_INVALID_ARG        # float alignment
    assert call(scores=C.c_void_p((1 << 20) + 4)) == _abi.GH_ERR_INVALID_ARG      # double alignment
    assert call(h=1 << 16, w=1 << 16) == _abi.GH_ERR_UNSUPPORTED
    assert call(nbytes=L.gh_image_scores_workspace(1, 16, 16) - 1) == _abi.GH_ERR_WORKSPACE_SMALL
