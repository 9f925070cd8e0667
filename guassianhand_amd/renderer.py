"""Host-side mirror of the reference's per-view render path (tgs/models/renderer_one_shot.py).

Same names, argument meaning and outputs as the reference for the part of `GS3DRenderer` that sits on
the hot path: `GaussianModel` (:114-119), the GSLayer activations (:191-214) and the per-view loop of
`forward_single_batch` (:494-510) with its Gaussian selection (:468-477, `select_gaussians`), and the composition of the
whole of `forward_single_batch` (:448-512) over the reference's own sub-modules (`forward_single_batch`,
`fused_renderer_cls`). The feature networks above it (attention, MLPs) are out of scope and stay in the
reference: they are taken as callables of the renderer object.

`render_views(...)` is the MI355X form of the per-view loop: all views in one launch sequence, blend fused into the
kernels. The reference's own protocol (blend in torch, two `GaussianRasterizer` calls per view) needs nothing from this
module — the reference's unmodified `forward_single_view` runs on the import shim; the tests keep a restatement of it
(`tests/helpers.py::forward_single_view`) to compare the two forms.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _seam
from ._call import launch, lib, ptr
from .camera import pack_cameras_from_w2c
from .rasterizer import rasterize_views


class GaussianModel(NamedTuple):
    """renderer_one_shot.py:114-119."""
    xyz: torch.Tensor
    opacity: torch.Tensor
    rotation: torch.Tensor
    scaling: torch.Tensor
    shs: torch.Tensor


class _TruncExp(torch.autograd.Function):
    """tgs/utils/ops.py:37-53: forward exp(x), backward g * exp(clamp(x, max=15))."""

    @staticmethod
    def forward(ctx, x):
        x = x.float()
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


trunc_exp = _TruncExp.apply


def gs_activations(raw: Dict[str, torch.Tensor], pts: torch.Tensor, *, use_rgb: bool = True, xyz_offset: bool = True,
                   restrict_offset: bool = True, clip_scaling: Optional[float] = None) -> GaussianModel:
    """The activations of GSLayer.forward (renderer_one_shot.py:191-214) applied to the raw head outputs
    raw = {xyz, scaling, rotation, opacity, shs}; the linear heads themselves are dense GEMMs and stay in torch."""
    v = raw["xyz"]
    if restrict_offset:
        v = (torch.sigmoid(v) - 0.5) * (1.2 / 32)
    xyz = v + pts if xyz_offset else pts
    scaling = trunc_exp(raw["scaling"])
    if clip_scaling is not None:
        scaling = torch.clamp(scaling, min=0, max=clip_scaling)
    shs = raw["shs"]
    if use_rgb:
        shs = torch.sigmoid(shs)
    shs = torch.reshape(shs, (shs.shape[0], shs.shape[1] // 3, 3))       # (the reference's `-1` is ambiguous for zero rows)
    return GaussianModel(xyz=xyz, opacity=torch.sigmoid(raw["opacity"]), rotation=F.normalize(raw["rotation"]),
                         scaling=scaling, shs=shs)


class _SelectRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, points, features, lo, hi):
        dev = points.device
        if dev.type != "cuda":
            raise RuntimeError("select_gaussians needs tensors on a ROCm device (no CPU fallback)")
        N, Cf = points.shape[0], features.shape[1]
        sc = score.detach().reshape(-1).float().contiguous()
        pts, feat = points.detach().float().contiguous(), features.detach().float().contiguous()
        out = [torch.empty(N, 3, device=dev), torch.empty(N, Cf, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, Cf, device=dev)]
        idx = [torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)]
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(lib().gh_select_workspace_bytes(N), 8), dtype=torch.uint8, device=dev)
        launch("gh_select_rows", dev, ptr(sc), N, float(lo), float(hi), ptr(pts), ptr(feat), Cf, *[ptr(t) for t in out + idx],
               ptr(counts), ptr(ws), ws.numel())
        nv, nc = counts.tolist()                                  # the one host read-back (the reference makes four)
        ctx.shape = (N, Cf)
        ctx.save_for_backward(idx[0][:nv], idx[1][:nc])
        return out[0][:nv], out[1][:nv], out[2][:nc], out[3][:nc]

    @staticmethod
    def backward(ctx, g_vp, g_vf, g_cp, g_cf):
        iv, ic = ctx.saved_tensors
        N, Cf = ctx.shape
        gp = torch.zeros(N, 3, device=iv.device)
        gf = torch.zeros(N, Cf, device=iv.device)
        for g, i, dst in ((g_vp, iv, gp), (g_cp, ic, gp), (g_vf, iv, gf), (g_cf, ic, gf)):
            if g is not None and i.numel():
                dst.index_add_(0, i.long(), g.float())            # indices are unique within each of the two sets
        return None, gp, gf, None, None


def select_gaussians(if_gs_valid: torch.Tensor, query_points: torch.Tensor, gs_hidden_features: torch.Tensor,
                     threshold_low: float = 0.1, threshold_high: float = 0.9):
    """The Gaussian selection of forward_single_batch (renderer_one_shot.py:468-473) on the device: returns
    (query_points_valid, gs_hidden_features_valid, query_points_copied, gs_hidden_features_copied) — the rows whose validity
    score exceeds threshold_low, and (again) those above threshold_high, in index order, exactly what the four boolean-mask
    indexings of the reference produce, with ONE host read-back (the two counts) instead of four (`gh_select_rows`).
    The caller continues like the reference: refine the copied positions, concatenate (:474-477)."""
    return _SelectRows.apply(if_gs_valid, query_points, gs_hidden_features, threshold_low, threshold_high)


def render_views(gs: GaussianModel, w2cs: torch.Tensor, intrinsics: torch.Tensor, height: int, width: int,
                 background_color: torch.Tensor, ret_mask: bool = True, color_w=None, xyz_b=None, color_b=None,
                 opacity_b=None, *, use_rgb: bool = True, sh_degree: int = 3, scaling_modifier: float = 1.0,
                 sync: bool = True, cams: Optional[torch.Tensor] = None, geometry_cache=None) -> Dict[str, torch.Tensor]:
    """The view loop of forward_single_batch (renderer_one_shot.py:494-510) as ONE batched launch sequence:
    all cameras at once, the attribute blend fused into the projection kernel, and the RGB pass and the mask
    pass of every view (:338-346, :372-379) fused into one 4-channel walk (same preprocess, same sort).
    Returns stacked (Nv,H,W,3) maps like the reference's `torch.stack(v, dim=0)`; comp_mask repeats the
    accumulated alpha over 3 channels exactly as the reference's colour=1 render does.
    geometry_cache (rasterizer.GeometryCache, needs `cams`): the Gaussians' geometry and the cameras do not change from
    call to call — projection and sorts are done once, later calls only refresh opacities / colours."""
    if cams is None:                                    # callers that render the same cameras every step pass the packed records
        cams = pack_cameras_from_w2c(w2cs, intrinsics, height, width, background_color)
    img, alpha, _ = rasterize_views(cams, gs.xyz, gs.opacity, gs.scaling, gs.rotation, gs.shs, H=height, W=width,
                                    use_rgb=use_rgb, sh_degree=sh_degree, scale_modifier=scaling_modifier, xyz_b=xyz_b,
                                    opacity_b=opacity_b, color_w=color_w, color_b=color_b, sync=sync, return_alpha=True,
                                    geometry_cache=geometry_cache)
    out = {"comp_rgb": img.permute(0, 2, 3, 1), "comp_rgb_bg": background_color}
    if ret_mask:
        out["comp_mask"] = alpha.unsqueeze(-1).expand(-1, -1, -1, 3)
    out["image_chw"], out["alpha"] = img, alpha        # the rasteriser's own layouts (consumed by loss.fit_image_loss)
    out["3dgs"] = gs
    return out


# ---- forward_single_batch (renderer_one_shot.py:448-512), composed -------------------------------------------------------
def _lookup_uv_map(self, vert_uv: torch.Tensor, param_chw: torch.Tensor) -> torch.Tensor:
    """`self.query_triplane_texture(vert_uv, param.unsqueeze(0).unsqueeze(0)).squeeze(0)` (renderer_one_shot.py:420-446 at the
    call sites :489-492) for vert_uv (1,N,2): positions rescaled from [-radius_texture, radius_texture] to [-1, 1]
    (`scale_tensor`, tgs/utils/ops.py:23-34), bilinear, align_corners=True, zeros outside -> (N,C).
    The map arrives as the reference's (C,Hm,Wm) parameter; the kernel reads it channel-last, so a parameter whose MEMORY is
    (Hm,Wm,C) — `nn.Parameter(torch.zeros(Hm, Wm, C)).permute(2, 0, 1)` — is read in place, any other layout through one copy.
    UVs that carry a gradient (a differentiable `get_uvd` in full training) take torch's grid_sample, which differentiates
    w.r.t. the grid as well; the one-shot fit's UVs do not (infer_one_shot.py:340-343 trains maps, not UVs)."""
    from .uvmap import uv_sample
    r = float(getattr(self.cfg, "radius_texture", 1.0))
    pos = vert_uv[0]
    pos = (pos - (-r)) / (r - (-r))
    pos = pos * (1 - (-1)) + (-1)
    if pos.requires_grad or not param_chw.is_cuda:
        out = F.grid_sample(param_chw[None], pos[None, :, None, :], align_corners=True, mode="bilinear")
        return out[0, :, :, 0].transpose(0, 1)
    if pos.shape[0] == 0:
        return param_chw.new_zeros(0, param_chw.shape[0])
    return uv_sample(param_chw.permute(1, 2, 0), pos)


def forward_single_batch(self, gs_hidden_features: torch.Tensor, query_points: torch.Tensor, w2cs: torch.Tensor,
                         intrinsics: torch.Tensor, height: int, width: int, znear, zfar,
                         background_color: Optional[torch.Tensor], color_w=None, xyz_b=None, color_b=None, opacity_b=None,
                         vert3d_uv=None, face_uv=None, face_uv_xy=None):
    """GS3DRenderer.forward_single_batch (renderer_one_shot.py:448-512) with the reference's signature, over the reference's
    own sub-modules taken from `self` as callables — `gs_valid` (:468), `vert_pos_refinement` (:474), `forward_gs` (:478),
    `threshold_low` / `threshold_high`, `cfg.scaling_modifier` / `cfg.sh_degree` / `cfg.radius_texture`,
    `gs_net.cfg.use_rgb` — and `get_uvd` (livehand.input_encoder, :481; `self.get_uvd` if the object carries one):

        validity prune (> threshold_low)  U  duplicate-and-refine (> threshold_high)      select_gaussians: one read-back (:469-473)
        cat(valid, refined copies) / cat(valid features, copied features)                 :476-477
        forward_gs -> GaussianModel                                                       :478
        get_uvd -> UVs normalised to [-1, 1] (u / 1, v / 0.5)                             :481-486
        color_b / opacity_b maps looked up at the UVs                                     gh_uv_sample_forward (:489-492)
        all views in ONE launch sequence, blend fused, RGB + mask in one walk             render_views (:494-503)
        dict of stacked (Nv,H,W,3) maps + "3dgs"                                          :505-510

    znear / zfar are accepted and ignored exactly as the reference's Camera ignores them (:99-100 forces 0.01 / 1000)."""
    if_gs_valid = self.gs_valid(gs_hidden_features, query_points)
    pts_valid, feat_valid, pts_copied, feat_copied = select_gaussians(if_gs_valid.squeeze(1), query_points, gs_hidden_features,
                                                                      self.threshold_low, self.threshold_high)
    pts_copied = self.vert_pos_refinement(feat_copied, pts_copied)
    pts = torch.cat([pts_valid, pts_copied], dim=-2)
    feats = torch.cat([feat_valid, feat_copied], dim=-2)
    gs = self.forward_gs(feats, pts)

    get_uvd = getattr(self, "get_uvd", None)
    if get_uvd is None:
        from livehand.input_encoder import get_uvd          # the reference's own dependency (renderer_one_shot.py:19)
    vert_uv, _vert_d, _ = get_uvd(pts, vert3d_uv[0], face_uv, face_uv_xy)
    vert_uv = vert_uv.unsqueeze(0)
    vert_uv[..., 0] = 2.0 * (vert_uv[..., 0] / 1) - 1.0
    vert_uv[..., 1] = 2.0 * (vert_uv[..., 1] / 0.5) - 1.0
    if color_b is not None:
        color_b = _lookup_uv_map(self, vert_uv, color_b)
    if opacity_b is not None:
        opacity_b = _lookup_uv_map(self, vert_uv, opacity_b)

    nv = w2cs.shape[0]
    bg = background_color if background_color is not None else torch.zeros(3, dtype=torch.float32, device=pts.device)
    out = render_views(GaussianModel(gs.xyz, gs.opacity, gs.rotation, gs.scaling, gs.shs), w2cs, intrinsics, int(height), int(width), bg,
                       ret_mask=True, color_w=color_w, xyz_b=xyz_b, color_b=color_b, opacity_b=opacity_b,
                       use_rgb=bool(self.gs_net.cfg.use_rgb), sh_degree=int(self.cfg.sh_degree),
                       scaling_modifier=float(self.cfg.scaling_modifier))
    return {"comp_rgb": out["comp_rgb"], "comp_rgb_bg": bg.unsqueeze(0).expand(nv, -1) if nv else bg.new_zeros(0, 3),
            "comp_mask": out["comp_mask"], "3dgs": gs}


# ---- forward_single_batch of the EDIT renderer (renderer_one_shot_edit.py:440-520), composed ---------------------------------------
_EDIT_MAP_W, _EDIT_MAP_H = 2048, 1024           # the size of the colour-weight map the reference builds per call (:483)


def edit_color_w_rows(vert_uv: torch.Tensor, color_w: torch.Tensor, duplication: bool = False) -> torch.Tensor:
    """The per-Gaussian colour weights of the edit renderer, (N,48), without the map. The reference (renderer_one_shot_edit.py:483-493)
    fills a 16 x 3 x 1024 x 2048 tensor of ones ON THE HOST in every call — 403 MB — writes `color_w.view(-1,16,3)[0, k]` into the left
    half (k = 0, 1: the scale and shift of one hand) and the right half (k = 2, 3: the other hand) of its first two coefficient planes,
    copies it to the device and samples it bilinearly at the Gaussians' UVs (query_triplane_texture: grid_sample, align_corners=True,
    zeros outside). The map is constant inside a half, so the sample is a function of the UV alone: the four bilinear weights times
    the left / right constant of the corner's column (and 0 for a corner outside the map) — evaluated here per Gaussian with
    grid_sample's own arithmetic (unnormalise, floor, corner weights (x1 - x)(y1 - y).., products summed nw, ne, sw, se), O(N) on
    the device. render_edit['duplication'] copies the right half's constants onto the left half (:491-493).
    vert_uv: (1,N,2) in [-1, 1] (radius_texture = 1 is assumed like everywhere in the reference's configs)."""
    uv = vert_uv.reshape(-1, 2).float()
    w = color_w.reshape(-1, 16, 3)[0].float()                       # (16,3): rows 0..3 are used
    left = torch.stack([w[0], w[1]], 0)                             # (2 planes, 3): coefficient planes 0 and 1, columns < 1024
    right = torch.stack([w[2], w[3]], 0)
    if duplication:
        left = right
    W, H = _EDIT_MAP_W, _EDIT_MAP_H
    ix = ((uv[:, 0] + 1) / 2) * (W - 1)
    iy = ((uv[:, 1] + 1) / 2) * (H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    wnw, wne, wsw, wse = (x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)
    inx0, inx1 = (x0 >= 0) & (x0 <= W - 1), (x1 >= 0) & (x1 <= W - 1)
    iny0, iny1 = (y0 >= 0) & (y0 <= H - 1), (y1 >= 0) & (y1 <= H - 1)
    half = W // 2

    def corner(xc, inx, iny, wt):                                   # value of a corner x its weight, (N, planes, 3); ones elsewhere are handled below
        val = torch.where((xc < half)[:, None, None], left[None], right[None])
        return torch.where((inx & iny)[:, None, None], val * wt[:, None, None], torch.zeros_like(val))

    two = corner(x0, inx0, iny0, wnw) + corner(x1, inx1, iny0, wne) + corner(x0, inx0, iny1, wsw) + corner(x1, inx1, iny1, wse)
    # the other 14 coefficient planes hold ones everywhere: the sample is the sum of the in-bounds corner weights
    ones = (torch.where(inx0 & iny0, wnw, torch.zeros_like(wnw)) + torch.where(inx1 & iny0, wne, torch.zeros_like(wne)) +
            torch.where(inx0 & iny1, wsw, torch.zeros_like(wsw)) + torch.where(inx1 & iny1, wse, torch.zeros_like(wse)))
    out = ones[:, None, None].expand(-1, 16, 3).clone()
    out[:, 0:2, :] = two
    return out.reshape(-1, 48)


def forward_single_batch_edit(self, gs_hidden_features: torch.Tensor, query_points: torch.Tensor, w2cs: torch.Tensor,
                              intrinsics: torch.Tensor, height: int, width: int, znear, zfar,
                              background_color: Optional[torch.Tensor], color_w=None, xyz_b=None, color_b=None, opacity_b=None,
                              vert3d_uv=None, face_uv=None, face_uv_xy=None, render_edit=None):
    """GS3DRenderer.forward_single_batch of the EDIT / avatar-drive renderer (renderer_one_shot_edit.py:440-520; bound by
    config_one_shot_edit.yaml:179, config_one_shot_avatar_drive.yaml:179, config_one_shot_edit_drive.yaml:180) with the reference's
    signature over the reference's own sub-modules, as forward_single_batch above. What differs from the one-shot renderer:

        colour weights are PER GAUSSIAN: the two hands carry their own (scale, shift) pair, looked up by UV   edit_color_w_rows (:483-500)
            -> the rasteriser's (P,48) form, GH_FLAG_BLEND_W_PER_GAUSSIAN (the reference builds and uploads a 403 MB map per call)
        render_edit['duplication']     the right half's weights / colour biases serve both halves              (:491-493, :501-502)
        render_edit['edit_left_only']  the colour-bias map's left half is zeroed IN PLACE, as the reference does (:499-500)

    Everything else is forward_single_batch: selection, cat order, forward_gs, get_uvd, map lookups, one batched launch sequence."""
    if color_w is None:
        raise ValueError("the edit renderer's forward_single_batch needs color_w (renderer_one_shot_edit.py:484 reads it unconditionally)")
    if_gs_valid = self.gs_valid(gs_hidden_features, query_points)
    pts_valid, feat_valid, pts_copied, feat_copied = select_gaussians(if_gs_valid.squeeze(1), query_points, gs_hidden_features,
                                                                      self.threshold_low, self.threshold_high)
    pts_copied = self.vert_pos_refinement(feat_copied, pts_copied)
    pts = torch.cat([pts_valid, pts_copied], dim=-2)
    feats = torch.cat([feat_valid, feat_copied], dim=-2)
    gs = self.forward_gs(feats, pts)

    get_uvd = getattr(self, "get_uvd", None)
    if get_uvd is None:
        from livehand.input_encoder import get_uvd          # the reference's own dependency (renderer_one_shot_edit.py:19)
    vert_uv, _vert_d, _ = get_uvd(pts, vert3d_uv[0], face_uv, face_uv_xy)
    vert_uv = vert_uv.unsqueeze(0)
    vert_uv[..., 0] = 2.0 * (vert_uv[..., 0] / 1) - 1.0
    vert_uv[..., 1] = 2.0 * (vert_uv[..., 1] / 0.5) - 1.0
    dup = bool(render_edit is not None and render_edit["duplication"])
    color_w_rows = edit_color_w_rows(vert_uv, color_w, dup)
    if color_b is not None:
        if render_edit is not None:
            if render_edit["edit_left_only"]:
                color_b[..., :1024] = 0                       # (in place on the caller's map: the reference's own side effect, :500)
            if render_edit["duplication"]:
                color_b = torch.cat([color_b[..., 1024:], color_b[..., 1024:]], dim=-1)
        color_b = _lookup_uv_map(self, vert_uv, color_b)
    if opacity_b is not None:
        opacity_b = _lookup_uv_map(self, vert_uv, opacity_b)

    nv = w2cs.shape[0]
    bg = background_color if background_color is not None else torch.zeros(3, dtype=torch.float32, device=pts.device)
    out = render_views(GaussianModel(gs.xyz, gs.opacity, gs.rotation, gs.scaling, gs.shs), w2cs, intrinsics, int(height), int(width), bg,
                       ret_mask=True, color_w=color_w_rows, xyz_b=xyz_b, color_b=color_b, opacity_b=opacity_b,
                       use_rgb=bool(self.gs_net.cfg.use_rgb), sh_degree=int(self.cfg.sh_degree),
                       scaling_modifier=float(self.cfg.scaling_modifier))
    return {"comp_rgb": out["comp_rgb"], "comp_rgb_bg": bg.unsqueeze(0).expand(nv, -1) if nv else bg.new_zeros(0, 3),
            "comp_mask": out["comp_mask"], "3dgs": gs}


def fused_renderer_cls_edit(base):
    """fused_renderer_cls for tgs.models.renderer_one_shot_edit.GS3DRenderer (three of the reference's four YAML configs bind it):
    a subclass whose forward_single_batch is forward_single_batch_edit; `guassianhand_amd.tgs_renderer.GS3DRendererEdit`."""
    return _seam.graft((__name__, "fused_renderer_cls_edit"), base, {"forward_single_batch": forward_single_batch_edit}, "forward_single_batch")


def fused_renderer_cls(base):
    """The reference's plugin seam (`renderer_cls`, config/config_one_shot.yaml:175, resolved by tgs.find,
    tgs/__init__.py:4-9): a subclass of the given `GS3DRenderer` whose forward_single_batch is the composed MI355X path
    above; everything else — configure(), the feature fetch, SelfAttn, the batch loop of forward() (:514-648) — is the
    base class's. `guassianhand_amd.tgs_renderer.GS3DRenderer` is this class over tgs.models.renderer_one_shot.GS3DRenderer."""
    return _seam.graft((__name__, "fused_renderer_cls"), base, {"forward_single_batch": forward_single_batch}, "forward_single_batch")
