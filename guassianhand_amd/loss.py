"""Fused image loss (gh_l1_loss, include/gh_raster.h): L = mean|img - gt| with dL/dimg produced by the same pass.

Counterpart of the L1 term of the reference's loss (utils.py:282-294, `lambda_l1 * l1_loss(rgb, gt)`), as used by
bench.py's metric definition. ROCm tensors only; raises if the HIP library is missing."""
from __future__ import annotations

import torch

from . import rasterizer as R
from ._call import launch, ptr

_N_PARTIALS = 1024


def _l1_kernel(image, target, guard=None):
    """(mean|image - target|, its gradient w.r.t. image) from one pass (gh_l1_loss). guard: device GhCounters of the
    forward that rendered `image` (overflow -> loss NaN, zero gradient)."""
    if not image.is_cuda:
        raise RuntimeError("gh_l1_loss runs on a ROCm device only (there is no CPU path)")
    a = image.detach().float().contiguous()
    b = target.detach().float().contiguous()
    if a.shape != b.shape:
        raise ValueError("image and target must have the same shape")
    # the kernel reads both as float4: a contiguous view into a larger buffer (img[1:]) may start off a 16-byte boundary, and
    # .contiguous() hands such a view back as it is. Only then is it copied (a fresh allocation is aligned).
    if a.data_ptr() % 16:
        a = a.clone()
    if b.data_ptr() % 16:
        b = b.clone()
    n = a.numel()
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    grad = torch.empty_like(a)
    nblk = max(1, min(_N_PARTIALS, (n // 4 + 255) // 256))
    partials = torch.empty(nblk, dtype=torch.float32, device=a.device)
    launch("gh_l1_loss", a.device, ptr(a), ptr(b), n, ptr(loss), ptr(grad), ptr(partials), nblk, ptr(guard))
    return loss, grad


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target):
        loss, grad = _l1_kernel(image, target)
        ctx.save_for_backward(grad)
        ctx.shape = image.shape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return (grad * grad_loss).reshape(ctx.shape), None


def l1_mean_loss(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean|image - target| (0-dim tensor), differentiable w.r.t. image."""
    return _L1Mean.apply(image, target)


def _fit_kernel(image, alpha, gt_rgb, gt_mask, bbox_mask, lambda_l1, lambda_mloss, scale, guard=None):
    """(loss, dL/dimage, dL/dalpha) of the fit's image loss from one pass (gh_fit_loss)."""
    if not image.is_cuda:
        raise RuntimeError("gh_fit_loss runs on a ROCm device only (there is no CPU path)")
    f32 = lambda t: None if t is None else t.detach().float().contiguous()
    im, al, gr, gm, bb = f32(image), f32(alpha), f32(gt_rgb), f32(gt_mask), f32(bbox_mask)
    NV, _, H, W = im.shape
    if al.shape != (NV, H, W) or gr.shape != (NV, H, W, 3) or gm.shape != (NV, H, W) or (bb is not None and bb.shape != (NV, H, W)):
        raise ValueError("fit_image_loss: image (Nv,3,H,W), alpha (Nv,H,W), gt_rgb (Nv,H,W,3), gt_mask / bbox (Nv,H,W)")
    loss = torch.empty((), dtype=torch.float32, device=im.device)
    dimg, dal = torch.empty_like(im), torch.empty_like(al)
    nblk = max(1, min(_N_PARTIALS, (NV * H * W + 255) // 256))
    partials = torch.empty(nblk, dtype=torch.float32, device=im.device)
    launch("gh_fit_loss", im.device, ptr(im), ptr(al), ptr(gr), ptr(gm), ptr(bb), NV, H, W, float(lambda_l1), float(lambda_mloss),
           float(scale), ptr(loss), ptr(dimg), ptr(dal), ptr(partials), nblk, ptr(guard))
    return loss, dimg, dal


class _FitImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, alpha, gt_rgb, gt_mask, bbox_mask, lambda_l1, lambda_mloss, scale, guard):
        loss, dimg, dal = _fit_kernel(image, alpha, gt_rgb, gt_mask, bbox_mask, lambda_l1, lambda_mloss, scale, guard)
        ctx.save_for_backward(dimg, dal)
        return loss

    @staticmethod
    def backward(ctx, g):
        dimg, dal = ctx.saved_tensors
        return dimg * g, dal * g, None, None, None, None, None, None, None


def fit_image_loss(image, alpha, gt_rgb, gt_mask, bbox_mask=None, lambda_l1: float = 10.0, lambda_mloss: float = 1.0,
                   scale: float = 1.0, guard=None) -> torch.Tensor:
    """scale * sum over views of [lambda_l1 * L1(rgb, gt) + lambda_mloss * MSE(clip(alpha, -0.001, 1), gt_mask)] — the
    image part of the reference's fit loss (fit.fit_loss is the torch restatement) — on the rasteriser's own layouts:
    image (Nv,3,H,W), alpha (Nv,H,W); gt_rgb (Nv,H,W,3), gt_mask / bbox_mask (Nv,H,W). Differentiable w.r.t. image, alpha."""
    return _FitImageLoss.apply(image, alpha, gt_rgb, gt_mask, bbox_mask, lambda_l1, lambda_mloss, scale, guard)


# ---------------------------------------------------------------------------------------------------
class _RenderedLoss(torch.autograd.Function):
    """Render + image loss as ONE autograd node (the render and the gradient routing are rasterize_views', rasterizer._views_*).
    The loss kernel leaves dL/dimage (and dL/dalpha) unscaled; the upstream dL/dloss reaches the render backward as a device scalar
    (GhGrads.upstream_scale) and is applied while the kernel reads its pixels, so the autograd product `dL/dimage * dL/dloss`
    costs no pass over the images."""

    @staticmethod
    def forward(ctx, a, cams, *gaussians):
        spec = a.spec
        if spec[0] == "l1":                          # the fused epilogue reads the target as it lies: float32, contiguous, image-shaped
            tgt = spec[1].detach().float().contiguous()
            if tuple(tgt.shape) != (cams.reshape(-1, 40).shape[0], 3, a.H, a.W):
                raise ValueError("image and target must have the same shape")
            image, radii, rctx = R._views_forward(ctx, a, cams, gaussians, l1_target=tgt)
            # the render kernel's epilogue has produced both (GhOutputs.l1_*) wherever the library fuses them; else one pass over the
            # image, with the forward's counters as the device-side overflow guard (an overflowed render: loss NaN, zero gradients)
            loss, dimg = rctx.l1 if rctx.l1 is not None else _l1_kernel(image, tgt, rctx.ws[:16])
            dal = None
        elif spec[0] == "fit":
            f32 = lambda t: None if t is None else t.detach().float().contiguous()
            fit = (f32(spec[1]), f32(spec[2]), f32(spec[3])) + tuple(spec[4:])
            image, radii, rctx = R._views_forward(ctx, a, cams, gaussians, fit_loss=fit)
            loss, dimg, dal = rctx.fit if rctx.fit is not None else _fit_kernel(image, rctx.alpha, *fit, guard=rctx.ws[:16])
        else:
            raise ValueError(spec[0])
        ctx.dimg, ctx.dal = dimg, dal
        alpha = rctx.alpha if rctx.alpha is not None else image.new_zeros(0)
        ctx.mark_non_differentiable(image, alpha, radii)
        return loss, image, alpha, radii

    @staticmethod
    def backward(ctx, g_loss, _gi, _ga, _gr):
        return R._views_backward(ctx, ctx.dimg, ctx.dal, g_loss)


def _rendered_loss(spec, cams, xyz, opacity, scaling, rotation, shs, **kw):
    """kw: rasterize_views' keywords (but return_alpha: the fit form renders alpha) and defer_loss."""
    return R._apply_views(_RenderedLoss, cams, xyz, opacity, scaling, rotation, shs, return_alpha=spec[0] == "fit", spec=spec, **kw)


def rendered_l1_loss(cams, xyz, opacity, scaling, rotation, shs, target, **kw):
    """mean|render - target| with the render (rasterizer.rasterize_views arguments) and the loss in one autograd node.
    Returns (loss, image (Nv,3,H,W) detached, radii). Same values as l1_mean_loss(rasterize_views(...)[0], target).
    defer_loss=True (GH_FLAG_DEFER_LOSS_SUM): where the loss comes from the render kernel's epilogue its final one-workgroup sum
    moves into the BACKWARD (a spare workgroup of the render backward): the returned loss tensor holds its value only once
    loss.backward() has been enqueued — for loops that look at the loss after the step (bench.py, the fit's log)."""
    loss, image, _alpha, radii = _rendered_loss(("l1", target), cams, xyz, opacity, scaling, rotation, shs, **kw)
    return loss, image, radii


def rendered_fit_loss(cams, xyz, opacity, scaling, rotation, shs, gt_rgb, gt_mask, bbox_mask=None, lambda_l1: float = 10.0,
                      lambda_mloss: float = 1.0, scale: float = 1.0, **kw):
    """The fit's image loss (fit_image_loss) of a fused RGB + alpha render, one autograd node.
    Returns (loss, image (Nv,3,H,W), alpha (Nv,H,W)) with image / alpha detached."""
    loss, image, alpha, _radii = _rendered_loss(("fit", gt_rgb, gt_mask, bbox_mask, float(lambda_l1), float(lambda_mloss), float(scale)),
                                                cams, xyz, opacity, scaling, rotation, shs, **kw)
    return loss, image, alpha
