"""The composed forward_single_batch (guassianhand_amd/renderer.py) against the reference's own
GS3DRenderer.forward_single_batch (renderer_one_shot.py:448-512), captured in the build container
(tests/golden/make_batch_fixture.py -> batch_fixture.npz): same stand-in sub-modules, same inputs."""
import os

import numpy as np
import pytest
import torch

from helpers import BatchStandIns, GoldenNpz, batch_inputs, forward_single_view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "batch_fixture.npz"), allow_pickle=False)


def _run(dev, use_rgb, requires_grad=False):
    from guassianhand_amd.renderer import forward_single_batch
    st, inp = BatchStandIns(dev, use_rgb=use_rgb), batch_inputs()
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    if requires_grad:
        for k in ("feat", "pts", "color_w", "xyz_b", "color_b", "opacity_b"):
            d[k] = d[k].clone().requires_grad_(True)
    out = forward_single_batch(st.namespace(dev), d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"],
                               color_w=d["color_w"], xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"],
                               vert3d_uv=[None], face_uv=None, face_uv_xy=None)
    return st, d, out


@pytest.mark.parametrize("tag,use_rgb", [("rgb", True), ("sh", False)])
def test_composed_path_equals_the_reference_protocol_on_the_oracle(dev, fx, tag, use_rgb):
    """Keys, shapes and the Gaussians are the reference's; every view's comp_rgb / comp_mask equals the C oracle run on the very
    tensors the reference handed to its rasteriser (captured per call: blended means / opacities / colours, camera settings)."""
    from oracle.oracle_c import OracleRender
    st, d, out = _run(dev, use_rgb)
    assert sorted(out.keys()) == list(fx[f"{tag}_keys"])
    nv, H, W = d["w2cs"].shape[0], d["H"], d["W"]
    for k in ("comp_rgb", "comp_mask", "comp_rgb_bg"):
        assert tuple(out[k].shape) == tuple(fx[f"{tag}_shape_{k}"]), k
    assert np.array_equal(out["comp_rgb_bg"].cpu().numpy(), fx[f"{tag}_comp_rgb_bg"])
    for k in ("xyz", "opacity", "rotation", "scaling", "shs"):        # CPU vs GPU transcendental functions: a few ulps
        assert np.allclose(getattr(out["3dgs"], k).detach().cpu().numpy(), fx[f"{tag}_3dgs_{k}"], rtol=2e-6, atol=1e-7), k
    assert int(fx[f"{tag}_ncalls"]) == 2 * nv
    for v in range(nv):
        for ci, key in ((2 * v, "comp_rgb"), (2 * v + 1, "comp_mask")):
            t = lambda n: torch.tensor(fx[f"{tag}_call{ci}_{n}"])
            kw = dict(colors_precomp=t("colors_precomp")) if f"{tag}_call{ci}_colors_precomp" in fx.files else \
                dict(shs=t("shs"), sh_degree=int(fx[f"{tag}_call{ci}_sh_degree"]))
            orc = OracleRender(torch.tensor(fx[f"{tag}_call{ci}_cam"])[None], t("means3D"), t("opacities").reshape(-1), t("scales"),
                               t("rotations"), H=H, W=W, **kw)
            want = orc.image[0].permute(1, 2, 0)
            got = out[key][v].detach().cpu()
            assert (got - want).abs().max().item() <= 1e-4, (tag, v, key, (got - want).abs().max().item())
            orc.close()
    assert float(out["comp_mask"].max()) > 0.5 and float(out["comp_rgb"].std()) > 0.01      # something was drawn


@pytest.mark.parametrize("use_rgb", [True, False])
def test_composed_path_equals_the_two_call_protocol_with_gradients(dev, use_rgb):
    """The same composition written the reference's way on the same device — boolean-mask indexing, torch grid_sample lookups,
    forward_single_view's two GaussianRasterizer calls per view through the drop-in — images bit for bit, gradients of every
    differentiable input (features, points, blend parameters, UV maps) to rounding."""
    import torch.nn.functional as F
    from guassianhand_amd.camera import Camera
    st, d, out = _run(dev, use_rgb, requires_grad=True)
    gen = torch.Generator().manual_seed(3)
    w_rgb = torch.randn(out["comp_rgb"].shape, generator=gen).to(dev)
    w_msk = torch.randn(out["comp_mask"].shape, generator=gen).to(dev)
    leaves = ("feat", "pts", "color_w", "xyz_b", "color_b", "opacity_b")
    ((out["comp_rgb"] * w_rgb).sum() + (out["comp_mask"] * w_msk).sum()).backward()
    got = {k: d[k].grad.clone() for k in leaves}
    for k in leaves:
        d[k].grad = None
    # the reference's own statements (:468-510) over the same stand-ins
    s = st.gs_valid(d["feat"], d["pts"]).squeeze(1)
    pv, fv = d["pts"][s > st.threshold_low], d["feat"][s > st.threshold_low]
    pc, fc = d["pts"][s > st.threshold_high], d["feat"][s > st.threshold_high]
    pc = st.vert_pos_refinement(fc, pc)
    pts, feats = torch.cat([pv, pc], dim=-2), torch.cat([fv, fc], dim=-2)
    gs = st.forward_gs(feats, pts)
    uv, _, _ = st.get_uvd(pts, None, None, None)
    uv = uv.unsqueeze(0)
    uv[..., 0] = 2.0 * (uv[..., 0] / 1) - 1.0
    uv[..., 1] = 2.0 * (uv[..., 1] / 0.5) - 1.0
    look = lambda m: F.grid_sample(m[None], uv[:, :, None], align_corners=True, mode="bilinear").view(1, m.shape[0], -1).permute(0, 2, 1)[0]
    cb, ob = look(d["color_b"]), look(d["opacity_b"])
    rgb, msk = [], []
    for w2c, K in zip(d["w2cs"], d["Ks"]):
        r = forward_single_view(gs, Camera.from_w2c(w2c, K, d["H"], d["W"], 0.71, 1.42), d["bg"], color_w=d["color_w"], xyz_b=d["xyz_b"],
                                color_b=cb, opacity_b=ob, use_rgb=use_rgb)
        rgb.append(r["comp_rgb"]); msk.append(r["comp_mask"])
    rgb, msk = torch.stack(rgb), torch.stack(msk)
    assert torch.equal(gs.xyz, out["3dgs"].xyz) and torch.equal(gs.shs, out["3dgs"].shs)
    # (the kernel's bilinear weights and grid_sample's differ in the last bit, so "bit for bit" holds up to that lookup)
    assert (rgb - out["comp_rgb"]).abs().max().item() <= 2e-6 and (msk - out["comp_mask"]).abs().max().item() <= 2e-6
    ((rgb * w_rgb).sum() + (msk * w_msk).sum()).backward()
    for k in leaves:
        a, b = got[k], d[k].grad
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, k
        rel = ((a - b).norm() / (b.norm() + 1e-20)).item()
        assert rel <= 1e-4, (k, rel)


@pytest.mark.parametrize("lo,hi,what", [(0.1, 2.0, "no row is duplicated"), (2.0, 3.0, "no row survives the prune")])
def test_composed_path_with_empty_selections(dev, lo, hi, what):
    """The two degenerate outcomes of the selection (renderer_one_shot.py:469-473): nothing above threshold_high (the refinement network
    sees zero rows) and nothing above threshold_low (zero Gaussians: every view is the background, the mask is zero)."""
    from guassianhand_amd.renderer import forward_single_batch
    st, inp = BatchStandIns(dev, use_rgb=True), batch_inputs(N=150)
    st.threshold_low, st.threshold_high = lo, hi
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    out = forward_single_batch(st.namespace(dev), d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"],
                               color_w=d["color_w"], xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"], vert3d_uv=[None])
    s = d["feat"][:, 0]
    n = int((s > lo).sum()) + int((s > hi).sum())
    assert out["3dgs"].xyz.shape[0] == n and out["comp_rgb"].shape == (2, d["H"], d["W"], 3), what
    if n == 0:
        assert torch.equal(out["comp_rgb"], d["bg"].expand(2, d["H"], d["W"], 3)) and float(out["comp_mask"].abs().max()) == 0.0
    else:
        assert float(out["comp_mask"].max()) > 0.5


# ---- the edit / avatar-drive renderer (renderer_one_shot_edit.py:440-520; VERDICT r5 'next' item 8) ------------------------------------
@pytest.fixture(scope="module")
def efx(golden_dir):
    return GoldenNpz(os.path.join(golden_dir, "edit_batch_fixture.npz"))


_EDIT_VARIANTS = {"plain": None, "dup": dict(duplication=True, edit_left_only=False), "left": dict(duplication=False, edit_left_only=True)}


@pytest.mark.parametrize("tag,use_rgb", [("rgb", True), ("sh", False)])
@pytest.mark.parametrize("vtag", ["plain", "dup", "left"])
def test_composed_edit_path_equals_the_reference_protocol_on_the_oracle(dev, efx, tag, use_rgb, vtag):
    """forward_single_batch_edit against the reference's own method (captured: tests/golden/make_edit_batch_fixture.py): keys, shapes, the
    Gaussians; every view's comp_rgb / comp_mask == the C oracle on the tensors the REFERENCE handed to its rasteriser — which carry its
    per-Gaussian colour weights (looked up from the 403 MB map it builds per call), its colour / opacity biases and `render_edit`."""
    from guassianhand_amd.renderer import forward_single_batch_edit
    from helpers import edit_batch_inputs
    from oracle.oracle_c import OracleRender
    key = f"{tag}_{vtag}"
    st, inp = BatchStandIns(dev, use_rgb=use_rgb), edit_batch_inputs(n_views=2 if vtag == "plain" else 1)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    cb_map = d["color_b"].clone()
    out = forward_single_batch_edit(st.namespace(dev), d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"],
                                    color_w=d["color_w"], xyz_b=d["xyz_b"], color_b=cb_map, opacity_b=d["opacity_b"],
                                    vert3d_uv=[None], face_uv=None, face_uv_xy=None, render_edit=_EDIT_VARIANTS[vtag])
    assert sorted(out.keys()) == list(efx[f"{key}_keys"])
    nv, H, W = d["w2cs"].shape[0], d["H"], d["W"]
    for k in ("comp_rgb", "comp_mask", "comp_rgb_bg"):
        assert tuple(out[k].shape) == tuple(efx[f"{key}_shape_{k}"]), k
    for k in ("xyz", "opacity", "rotation", "scaling", "shs"):
        assert np.allclose(getattr(out["3dgs"], k).detach().cpu().numpy(), efx[f"{key}_3dgs_{k}"], rtol=2e-6, atol=1e-7), k
    # 'edit_left_only' zeroes the caller's map in place, as the reference does (:500); nothing else touches it
    assert int(efx[f"{key}_color_b_map_changed"]) == int(not torch.equal(cb_map, d["color_b"])) == int(vtag == "left")
    if vtag == "left":
        assert float(cb_map[..., :1024].abs().max()) == 0.0 and torch.equal(cb_map[..., 1024:], d["color_b"][..., 1024:])
    assert int(efx[f"{key}_ncalls"]) == 2 * nv
    for v in range(nv):
        for ci, okey in ((2 * v, "comp_rgb"), (2 * v + 1, "comp_mask")):
            t = lambda n: torch.tensor(efx[f"{key}_call{ci}_{n}"])
            kw = dict(colors_precomp=t("colors_precomp")) if f"{key}_call{ci}_colors_precomp" in efx.files else \
                dict(shs=t("shs"), sh_degree=int(efx[f"{key}_call{ci}_sh_degree"]))
            orc = OracleRender(torch.tensor(efx[f"{key}_call{ci}_cam"])[None], t("means3D"), t("opacities").reshape(-1), t("scales"),
                               t("rotations"), H=H, W=W, **kw)
            want = orc.image[0].permute(1, 2, 0)
            got = out[okey][v].detach().cpu()
            assert (got - want).abs().max().item() <= 1e-4, (key, v, okey, (got - want).abs().max().item())
            orc.close()
    assert float(out["comp_mask"].max()) > 0.5 and float(out["comp_rgb"].std()) > 0.01


def test_composed_edit_path_lookups_and_gradients(dev, efx):
    """The three lookups of the edit path on the device against the reference's captured ones (colour weights through
    edit_color_w_rows, biases through gh_uv_sample_forward), and the gradient of a loss on the render reaching the (48,) colour
    weights, the bias maps and the network-side inputs."""
    from guassianhand_amd import renderer as Rn
    from helpers import edit_batch_inputs
    st, inp = BatchStandIns(dev, use_rgb=True), edit_batch_inputs()
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    ns = st.namespace(dev)
    s = d["feat"][:, 0]
    pts = torch.cat([d["pts"][s > 0.1], st.vert_pos_refinement(d["feat"][s > 0.9], d["pts"][s > 0.9])])
    uv, _, _ = st.get_uvd(pts, None, None, None)
    uv = uv.unsqueeze(0).clone()
    uv[..., 0] = 2.0 * (uv[..., 0] / 1) - 1.0
    uv[..., 1] = 2.0 * (uv[..., 1] / 0.5) - 1.0
    rows = Rn.edit_color_w_rows(uv, d["color_w"], False).cpu()
    assert float((rows - torch.tensor(efx["rgb_plain_color_w_rows"])).abs().max()) <= 5e-7
    cb = Rn._lookup_uv_map(ns, uv, d["color_b"]).cpu()
    ob = Rn._lookup_uv_map(ns, uv, d["opacity_b"]).cpu()
    # (the UVs come from a sigmoid evaluated on the GPU here and on the CPU at capture: an ulp of u is 2e-4 texels of a 2048-wide map
    #  of independent random texels ~ N(0, 0.05^2) — the bias rows agree to 1e-4, not to float32 rounding; the weights above are
    #  piecewise constant and do)
    assert float((cb - torch.tensor(efx["rgb_plain_color_b_rows"])).abs().max()) <= 1e-4
    assert float((ob - torch.tensor(efx["rgb_plain_opacity_b_rows"])).abs().max()) <= 1e-4
    for k in ("feat", "pts", "color_w", "xyz_b", "color_b", "opacity_b"):
        d[k] = d[k].clone().requires_grad_(True)
    out = Rn.forward_single_batch_edit(ns, d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"],
                                       color_w=d["color_w"], xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"],
                                       vert3d_uv=[None], face_uv=None, face_uv_xy=None, render_edit=None)
    (out["comp_rgb"].square().mean() + out["comp_mask"].mean()).backward()
    gw = d["color_w"].grad.view(16, 3)
    assert float(gw[:2].abs().min()) > 0 and float(gw[2:4].abs().min()) > 0 and float(gw[4:].abs().max()) == 0.0     # RGB mode: (scale, shift) of both hands
    for k in ("feat", "pts", "xyz_b", "color_b", "opacity_b"):
        assert d[k].grad is not None and float(d[k].grad.abs().max()) > 0, k
