"""Image-quality scores of rendered views: MSE, PSNR and SSIM as the reference's test step computes them
(infer_one_shot.py:527-554 calling Evaluator.compute_score, evaluator.py:85-118), on the device (gh_image_scores,
include/gh_metrics.h). Per view, with images in [0,1]:

1. the prediction is taken as 0 wherever `bbox_mask == 0` (all channels); the target is not masked;
2. mse = mean((pred - gt)^2) over the whole image, psnr = -10 log10(mse) (+inf when mse == 0);
3. (x, y, w, h) = the tightest box around the non-zero pixels of `mask_at_box` (cv2.boundingRect); SSIM sees only that crop;
4. ssim = scikit-image 0.16's `structural_similarity(pred_crop, gt_crop, multichannel=True)` with its defaults: per channel in
   float64, 7x7 uniform window, sample covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = 2 (skimage 0.16 takes the range of a
   float image from its dtype, (-1, 1)), averaged over the pixels whose window lies inside the crop, then over the channels.
   NaN when the crop is smaller than 7 in either direction (skimage raises ValueError there; so does Evaluator.compute_score).

LPIPS is the fourth number of the reference's evaluator and lives in lpips.py (`lpips_scores`; Evaluator(lpips=net) adds it); the
reference's PNG dumps of the crops are not written. CPU tensors go through `_image_scores_cpu`, a plain float64
torch restatement of the same four steps (the yardstick of the GPU tests); ROCm tensors go through the HIP kernels only."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _abi
from ._call import launch, lib, ptr, workspace


class ImageScores(NamedTuple):
    mse: torch.Tensor        # (Nv,) float64
    psnr: torch.Tensor       # (Nv,) float64
    ssim: torch.Tensor       # (Nv,) float64, NaN where the crop is smaller than 7x7
    bbox: torch.Tensor       # (Nv, 4) int32: x, y, w, h of mask_at_box's bounding box, (0, 0, 0, 0) for an empty mask


def _images(t: torch.Tensor, layout: str, name: str):
    """(tensor, channel_last) for the kernel: float32 read in place where its memory is either (Nv,3,H,W) or (Nv,H,W,3), whatever
    the logical layout (render_views' comp_rgb is a channel-last view of a channel-first image)."""
    if t.dim() != 4 or t.shape[1 if layout == "chw" else 3] != 3:
        raise ValueError(f"{name}: expected ({'Nv,3,H,W' if layout == 'chw' else 'Nv,H,W,3'}), got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    hwc = layout == "hwc"
    if t.is_contiguous():
        return t, hwc
    if t.permute(*((0, 3, 1, 2) if hwc else (0, 2, 3, 1))).is_contiguous():
        return t, not hwc
    return t.contiguous(), hwc


def _mask(m: torch.Tensor, shape, name: str, box: bool) -> torch.Tensor:
    """(Nv,H,W) with a trailing channel of 3 sliced to [..., 0] as test_step does. mask_at_box is cast the reference's way
    (`.astype(np.uint8)`, then non-zero); bbox_mask is compared with 0 in its own dtype (`bbox_mask == 0`)."""
    m = torch.as_tensor(m).detach()
    if m.dim() == len(shape) + 1 and m.shape[-1] == 3:
        m = m[..., 0]
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)} (or with a trailing dim of 3), got {tuple(m.shape)}")
    if m.dtype not in (torch.uint8, torch.bool):
        m = m.to(torch.uint8) if box else (m != 0)
    return m.contiguous()


def image_scores(pred: torch.Tensor, gt: torch.Tensor, mask_at_box: torch.Tensor, *, bbox_mask: Optional[torch.Tensor] = None,
                 layout: str = "chw", data_range: float = 2.0) -> ImageScores:
    """Scores of Nv views. pred, gt: (Nv,3,H,W) for layout="chw" (what compute_score receives) or (Nv,H,W,3) for "hwc" (what
    render_views returns as comp_rgb); mask_at_box and bbox_mask: (Nv,H,W) of any dtype. data_range: R of the SSIM constants
    (2.0 reproduces the reference's values). Returns device tensors and never synchronises on ROCm tensors (graph capturable)."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout must be 'chw' or 'hwc', got {layout!r}")
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    R = float(data_range)
    if not (R > 0.0 and math.isfinite(R)):
        raise ValueError(f"data_range must be finite and > 0, got {data_range}")
    if pred.dim() != 4:
        raise ValueError(f"pred: expected a 4-d stack of views, got {tuple(pred.shape)}")
    Nv, H, W = (pred.shape[0], pred.shape[2], pred.shape[3]) if layout == "chw" else pred.shape[:3]
    mbox = _mask(mask_at_box, (Nv, H, W), "mask_at_box", True)
    bbm = None if bbox_mask is None else _mask(bbox_mask, (Nv, H, W), "bbox_mask", False)
    if not pred.is_cuda:
        return _image_scores_cpu(pred, gt, mbox, bbm, layout, R)
    dev = pred.device
    if gt.device != dev or mbox.device != dev or (bbm is not None and bbm.device != dev):
        raise ValueError("pred, gt and the masks must be on the same device")
    p, p_hwc = _images(pred, layout, "pred")
    g, g_hwc = _images(gt, layout, "gt")
    nbytes = lib().gh_image_scores_workspace(Nv, H, W)
    ws = workspace(nbytes, dev)
    scores = torch.empty(3, Nv, dtype=torch.float64, device=dev)
    bbox = torch.empty(Nv, 4, dtype=torch.int32, device=dev)
    flags = (_abi.GH_METRICS_PRED_HWC if p_hwc else 0) | (_abi.GH_METRICS_GT_HWC if g_hwc else 0)
    launch("gh_image_scores", dev, ptr(p), ptr(g), ptr(mbox), ptr(bbm), Nv, H, W, flags, R, ptr(scores), ptr(bbox), ptr(ws), nbytes)
    return ImageScores(scores[0], scores[1], scores[2], bbox)


# ---- CPU: float64 restatement (the yardstick of the device path) ------------------------------------------------------------
def _bounding_rect(m: torch.Tensor):
    """cv2.boundingRect of a (H,W) mask: (x, y, w, h) of the non-zero pixels, (0, 0, 0, 0) when there are none."""
    ys = torch.nonzero(m.any(dim=1)).flatten()
    if ys.numel() == 0:
        return 0, 0, 0, 0
    xs = torch.nonzero(m.any(dim=0)).flatten()
    return int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1)


def _ssim_crop(a: torch.Tensor, b: torch.Tensor, R: float) -> float:
    """skimage 0.16 structural_similarity of two (3,h,w) float64 crops, multichannel: the mean of the channel means of S over the
    pixels whose 7x7 window lies inside the crop (avg_pool2d without padding yields exactly those windows)."""
    box = lambda t: F.avg_pool2d(t.unsqueeze(0), 7, stride=1).squeeze(0)
    cov_norm = 49.0 / 48.0
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    ux, uy = box(a), box(b)
    uxx, uyy, uxy = box(a * a), box(b * b), box(a * b)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.mean(dim=(1, 2)).mean())


def _image_scores_cpu(pred, gt, mbox, bbm, layout: str, R: float) -> ImageScores:
    x, y = pred.detach().double(), gt.detach().double()
    if layout == "hwc":
        x, y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    if bbm is not None:
        x = torch.where(bbm.unsqueeze(1) != 0, x, torch.zeros((), dtype=x.dtype))
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    psnr = -10.0 * torch.log10(mse)
    ssim = torch.empty(x.shape[0], dtype=torch.float64)
    bbox = torch.empty(x.shape[0], 4, dtype=torch.int32)
    for v in range(x.shape[0]):
        bx, by, bw, bh = _bounding_rect(mbox[v] != 0)
        bbox[v] = torch.tensor([bx, by, bw, bh], dtype=torch.int32)
        ssim[v] = math.nan if bw < 7 or bh < 7 else _ssim_crop(x[v, :, by:by + bh, bx:bx + bw], y[v, :, by:by + bh, bx:bx + bw], R)
    return ImageScores(mse, psnr, ssim, bbox)


# ---- drop-in for the reference's evaluator.Evaluator ------------------------------------------------------------------------
class Evaluator:
    """`evaluator.Evaluator` without the PNG dumps: compute_score returns {'mse', 'psnr', 'ssim'} as Python floats from one
    device-to-host copy, and with `lpips` (a lpips.AlexLPIPS holding the weights) also 'lpips', the reference's fourth number, from a
    second one. `result_dir` is kept for the reference's test_step, which sets it, and is not used."""

    def __init__(self, data_range: float = 2.0, lpips=None):
        self.result_dir = None
        self.data_range = data_range
        self.lpips = lpips

    def compute_score(self, rgb_pred, rgb_gt, input_imgs=None, mask_at_box=None, human_idx=None, frame_index=None, view_index=None,
                      **ignored):
        """rgb_pred, rgb_gt: (1,3,H,W) in [0,1]; mask_at_box: (1,H,W) (or (H,W)). input_imgs, the indices and the keypoint
        arguments only named the reference's PNG dumps and are ignored."""
        pred, gt = torch.as_tensor(rgb_pred), torch.as_tensor(rgb_gt)
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
        if pred.dim() != 4 or pred.shape[0] != 1:
            raise ValueError(f"compute_score scores one view: expected (1,3,H,W), got {tuple(pred.shape)}")
        m = torch.as_tensor(mask_at_box).reshape(1, *pred.shape[2:])
        s = image_scores(pred, gt, m.to(pred.device), layout="chw", data_range=self.data_range)
        host = torch.cat([torch.stack([s.mse, s.psnr, s.ssim]).reshape(-1), s.bbox.reshape(-1).double()]).cpu()
        w, h = int(host[5]), int(host[6])
        if w < 7 or h < 7:
            raise ValueError(f"SSIM needs a crop of at least 7x7 pixels; mask_at_box's bounding box is {w}x{h} "
                             "(skimage's structural_similarity raises here too)")
        out = {"mse": float(host[0]), "psnr": float(host[1]), "ssim": float(host[2])}
        if self.lpips is not None:
            from .lpips import MIN_SIZE, _scores_with_boxes
            if w < MIN_SIZE or h < MIN_SIZE:
                raise ValueError(f"LPIPS needs a crop of at least {MIN_SIZE}x{MIN_SIZE} pixels (AlexNet's smallest input); "
                                 f"mask_at_box's bounding box is {w}x{h}")
            box = (int(host[3]), int(host[4]), w, h)
            out["lpips"] = float(_scores_with_boxes(self.lpips, pred, gt, s.bbox, [box], None, "chw", True, "fused")[0])
        return out
