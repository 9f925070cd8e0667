#!/usr/bin/env python
"""Generate tests/golden/cond_fixture.npz by running the REFERENCE's SpatialEncoder(sp_level=4) (spatial.py) and
additional_features_fc(852, 51) (tgs/models/verts_refinement.py:119-131) on the CPU in eval() mode, over the concatenation
TGS._forward builds (infer_one_shot.py:273-274).

Runs only where the reference tree is present; the resulting .npz is data (inputs, parameters and recorded outputs) and is committed;
nothing of the reference travels. The reference modules are imported under the stub modules of make_host_fixtures.py. The module is
built the reference's way, its initial state dict is recorded (keys and shapes), then random non-zero parameters (LayerNorm weight
and bias and every bias too) are loaded and forward + backward run on B = 2 batch elements of N = 32 points, with two different pose
vectors.

Stored small: quantised arrays are int8 (`*_q`, value = q * scale, the LayerNorm weight 1 + q * scale).

    uv, xyz                       (2,32,2), (2,32,3) float32
    flag                          (2,32,1) bool: the reference's mink_idxs_inter
    code_q, pose_q                identity_code_vert (2,32,33) and pose_feats (2,1,768)
    ln_weight_q, ln_bias_q, fc1_weight_q, fc2_weight_q; fc1_bias, fc2_bias (float32)
    scales                        code, pose, ln, fc1, fc2, cot
    uv_sp, xyz_sp                 the reference's SpatialEncoder outputs (bit patterns the restatement must reproduce)
    out                           additional_features_fc(cat(...)), (2,32,51)
    cot_q                         the fixed cotangent
    grad_code                     the gradient of sum(out * cot) with respect to identity_code_vert
    init.<key>                    the shape of every entry of the initial state dict

Usage: python tests/golden/make_cond_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cond_fixture.npz")
B, N, CC, DE, D, HD, SEED = 2, 32, 33, 768, 852, 51, 11
SCALES = {"code": 1.0 / 64, "pose": 1.0 / 32, "ln": 1.0 / 256, "fc1": 1.0 / 512, "fc2": 1.0 / 256, "cot": 1.0 / 8}
KEYS = {"ln_weight": "ff1.layer_norm.weight", "ln_bias": "ff1.layer_norm.bias", "fc1_weight": "ff1.fc1.weight", "fc1_bias": "ff1.fc1.bias",
        "fc2_weight": "ff1.fc2.weight", "fc2_bias": "ff1.fc2.bias"}


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    from spatial import SpatialEncoder
    from tgs.models.verts_refinement import additional_features_fc

    g = torch.Generator().manual_seed(SEED)

    def q(lo, hi, *shape):
        t = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8)
        t[t == 0] = 1
        return t

    uv = torch.rand(B, N, 2, generator=g)
    xyz = 0.1 * torch.randn(B, N, 3, generator=g)
    flag = torch.rand(B, N, 1, generator=g) < 0.4
    code_q, pose_q = q(-64, 64, B, N, CC), q(-96, 96, B, 1, DE)
    qs = {"ln_weight": q(-77, 77, D), "ln_bias": q(-60, 60, D), "fc1_weight": q(-48, 48, HD, D), "fc2_weight": q(-80, 80, HD, HD)}
    vals = {"ln_weight": 1.0 + qs["ln_weight"].float() * SCALES["ln"], "ln_bias": qs["ln_bias"].float() * SCALES["ln"],
            "fc1_weight": qs["fc1_weight"].float() * SCALES["fc1"], "fc1_bias": 0.2 * torch.randn(HD, generator=g),
            "fc2_weight": qs["fc2_weight"].float() * SCALES["fc2"], "fc2_bias": 0.2 * torch.randn(HD, generator=g)}
    out = {"uv": uv.numpy(), "xyz": xyz.numpy(), "flag": flag.numpy(), "code_q": code_q.numpy(), "pose_q": pose_q.numpy(),
           "scales": np.array([SCALES[k] for k in ("code", "pose", "ln", "fc1", "fc2", "cot")]),
           "fc1_bias": vals["fc1_bias"].numpy(), "fc2_bias": vals["fc2_bias"].numpy()}
    for k, v in qs.items():
        out[f"{k}_q"] = v.numpy()

    torch.manual_seed(5)
    m = additional_features_fc(D, HD).eval()
    sd = m.state_dict()
    for k, v in sd.items():
        out[f"init.{k}"] = np.array(v.shape)
    assert sorted(sd) == sorted(KEYS.values())
    with torch.no_grad():
        for k, key in KEYS.items():
            assert float(vals[k].abs().min()) > 0, k
            sd[key].copy_(vals[k])

    sp = SpatialEncoder(sp_level=4)
    code = (code_q.float() * SCALES["code"]).requires_grad_(True)
    pose = pose_q.float() * SCALES["pose"]
    assert not torch.equal(pose[0], pose[1])
    uv_sp, xyz_sp = sp(uv), sp(xyz)
    feats = torch.cat([uv, uv_sp, xyz, xyz_sp, flag, code, pose.repeat(1, N, 1)], dim=-1)     # infer_one_shot.py:273
    assert tuple(feats.shape) == (B, N, D)
    y = m(feats)
    assert tuple(y.shape) == (B, N, HD)
    cq = torch.randint(-24, 25, y.shape, generator=g, dtype=torch.int8)
    (y * (cq.float() * SCALES["cot"])).sum().backward()
    out.update(uv_sp=uv_sp.numpy(), xyz_sp=xyz_sp.numpy(), out=y.detach().numpy(), cot_q=cq.numpy(), grad_code=code.grad.numpy())
    assert float((y > 0).float().mean()) > 0.2 and float(code.grad.abs().max()) > 0

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
