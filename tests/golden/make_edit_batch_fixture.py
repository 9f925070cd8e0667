#!/usr/bin/env python
"""Generate tests/golden/edit_batch_fixture.npz by running the REFERENCE's own edit / avatar-drive renderer,
tgs.models.renderer_one_shot_edit.GS3DRenderer.forward_single_batch (renderer_one_shot_edit.py:440-520), on CPU under the stub finder
of make_host_fixtures.py — the method three of the reference's four YAML configs bind (config_one_shot_edit.yaml:179,
config_one_shot_avatar_drive.yaml:179, config_one_shot_edit_drive.yaml:180).

Pinned: the composition of make_batch_fixture.py plus what the edit renderer adds — the per-Gaussian colour weights it looks up from the
16 x 3 x 1024 x 2048 map it builds per call (:483-494: the two hands' (scale, shift) pairs in the map's two halves), `render_edit`
('duplication': the right half serves both; 'edit_left_only': the colour-bias map's left half zeroed in place), and the tensors that
arrive at the rasteriser in consequence. Sub-modules outside the scope are tests/helpers.py::BatchStandIns, as in make_batch_fixture.py;
query_triplane_texture and forward_single_view are the reference's own methods (their sampled outputs are recorded too).

Runs only in the build container (needs /root/reference). Usage: python tests/golden/make_edit_batch_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cpu_numerics  # noqa: E402

cpu_numerics.apply(threads=1)      # the CPU arithmetic the tests check these values under (tests/cpu_numerics.py)
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
OUT = os.path.join(HERE, "edit_batch_fixture.npz")
VARIANTS = (("plain", None), ("dup", dict(duplication=True, edit_left_only=False)), ("left", dict(duplication=False, edit_left_only=True)))


def main():
    import make_host_fixtures as mh
    calls = []
    mh.install_stubs(calls)
    sys.path.insert(0, mh.REF)
    import tgs.models.renderer_one_shot_edit as ref
    from helpers import BatchStandIns, edit_batch_inputs

    out = {}
    for tag, use_rgb in (("rgb", True), ("sh", False)):
        for vtag, render_edit in VARIANTS:
            key = f"{tag}_{vtag}"
            st = BatchStandIns("cpu", use_rgb=use_rgb)
            inp = edit_batch_inputs(n_views=2 if vtag == "plain" else 1)
            ns = st.namespace("cpu")
            sampled = []
            qtt = types.MethodType(ref.GS3DRenderer.query_triplane_texture, ns)
            ns.query_triplane_texture = lambda uv, tp: (sampled.append(qtt(uv, tp)), sampled[-1])[1]     # records every lookup's result
            ns.forward_single_view = types.MethodType(ref.GS3DRenderer.forward_single_view, ns)
            ref.get_uvd = st.get_uvd
            calls.clear()
            color_b = inp["color_b"].clone()
            res = ref.GS3DRenderer.forward_single_batch(
                ns, inp["feat"], inp["pts"], inp["w2cs"], inp["Ks"], inp["H"], inp["W"], 0.71, 1.42, inp["bg"],
                color_w=inp["color_w"], xyz_b=inp["xyz_b"], color_b=color_b, opacity_b=inp["opacity_b"],
                vert3d_uv=[None], face_uv=None, face_uv_xy=None, render_edit=render_edit)
            out[f"{key}_keys"] = np.array(sorted(res.keys()))
            for k, v in res.items():
                if isinstance(v, torch.Tensor):
                    out[f"{key}_shape_{k}"] = np.array(v.shape)
            for k in ("xyz", "opacity", "rotation", "scaling", "shs"):
                out[f"{key}_3dgs_{k}"] = getattr(res["3dgs"], k).detach().numpy()
            out[f"{key}_ncalls"] = np.array(len(calls))
            # the three lookups in call order: colour weights (N,48), colour biases (N,48), opacity bias (N,1); kept where a test
            # checks them (the weights of every RGB variant, the biases of the plain one)
            if use_rgb:
                out[f"{key}_color_w_rows"] = sampled[0].squeeze(0).detach().numpy()
            if key == "rgb_plain":
                out[f"{key}_color_b_rows"] = sampled[1].squeeze(0).detach().numpy()
                out[f"{key}_opacity_b_rows"] = sampled[2].squeeze(0).detach().numpy()
            out[f"{key}_color_b_map_changed"] = np.array(int(not torch.equal(color_b, inp["color_b"])))     # 'edit_left_only' writes in place
            for ci, (rs, kw) in enumerate(calls):
                out[f"{key}_call{ci}_cam"] = np.concatenate([rs.viewmatrix.reshape(-1).numpy(), rs.projmatrix.reshape(-1).numpy(),
                                                             rs.campos.numpy(), [rs.tanfovx, rs.tanfovy], rs.bg.numpy()]).astype(np.float32)
                out[f"{key}_call{ci}_sh_degree"] = np.array(rs.sh_degree)
                for k, v in kw.items():
                    if v is not None and k != "means2D":
                        out[f"{key}_call{ci}_{k}"] = v.detach().numpy()
    from guassianhand_amd.renderer import forward_single_batch_edit, fused_renderer_cls_edit
    cls = fused_renderer_cls_edit(ref.GS3DRenderer)
    ok = issubclass(cls, ref.GS3DRenderer) and cls.forward_single_batch is forward_single_batch_edit and cls.forward is ref.GS3DRenderer.forward
    import inspect
    same_sig = list(inspect.signature(forward_single_batch_edit).parameters) == list(inspect.signature(ref.GS3DRenderer.forward_single_batch).parameters)
    out["seam_ok"] = np.array([int(ok), int(same_sig)])
    # every distinct array once: a repeat (the same Gaussians in every variant and rasteriser call) is stored as an entry of
    # `aliases` ("name=stored name"), resolved by tests/helpers.py::GoldenNpz
    stored, aliases = {}, []
    for k, v in out.items():
        same = next((s for s, w in stored.items() if w.dtype == v.dtype and w.shape == v.shape and np.array_equal(w, v)), None)
        if same is None:
            stored[k] = v
        else:
            aliases.append(f"{k}={same}")
    np.savez_compressed(OUT, aliases=np.array(aliases), **stored)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes; seam {out['seam_ok']}")


if __name__ == "__main__":
    main()
