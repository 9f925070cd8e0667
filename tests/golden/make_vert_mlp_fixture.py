#!/usr/bin/env python
"""Generate tests/golden/vert_mlp_fixture.npz by running the REFERENCE's vert_valid and vert_pos_refinement
(tgs/models/verts_refinement.py:35-83) on the CPU in eval() mode.

Runs only where the reference tree is present; the resulting .npz is data (inputs, parameters and recorded outputs) and is committed;
nothing of the reference travels. The reference module is imported under the stub modules of make_host_fixtures.py. Both modules are
built the reference's way for Cf = 131, their initial state dicts are recorded (keys and shapes), then random non-zero parameters
(LayerNorm weight and bias and every Linear bias too) are loaded and forward + backward run on P = 64 points.

Stored small: features are multiples of 1/16 and the two large weights multiples of 1/256, kept as int8 (`*_q`, value = q * scale).
Per module <m> (v = vert_valid, r = vert_pos_refinement):

    <m>_<param>                   ln_weight, ln_bias, fc1_bias, fc2_bias, fc_weight, fc_bias (float32); <m>_fc1_weight_q, <m>_fc2_weight_q
    <m>_out                       the module's output on (x, pts)
    <m>_cot_q                     the fixed cotangent (int8, multiples of 1/8)
    <m>_grad_pts, <m>_grad_x8     the gradients of sum(out * cot): positions, every 8th row of the features
    <m>_grad_<param>              and every parameter
    init_<m>.<key>                the shape of every entry of the initial state dict

The gate's `fc` weight is scaled so that its logits spread over roughly +-4, and the script ASSERTS (exit status non-zero otherwise)
that at least 8 rows score below 0.1, at least 8 between 0.1 and 0.9, at least 8 above 0.9, and that no score lies within 1e-3 of
either threshold: a rounding difference of about 1e-6 can then never change which rows the two thresholds select.

Usage: python tests/golden/make_vert_mlp_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vert_mlp_fixture.npz")
P, CF, SEED = 64, 131, 7
X_SCALE, W_SCALE, C_SCALE = 1.0 / 16, 1.0 / 256, 1.0 / 8
KEYS = {"ln_weight": "ff.layer_norm.weight", "ln_bias": "ff.layer_norm.bias", "fc1_weight": "ff.fc1.weight", "fc1_bias": "ff.fc1.bias",
        "fc2_weight": "ff.fc2.weight", "fc2_bias": "ff.fc2.bias", "fc_weight": "fc.weight", "fc_bias": "fc.bias"}
QUANTISED = ("fc1_weight", "fc2_weight")


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    import tgs.models.verts_refinement as ref

    g = torch.Generator().manual_seed(SEED)
    D, Hd = CF + 3, (CF + 3) // 4
    xq = torch.randint(-40, 41, (P, CF), generator=g, dtype=torch.int8)
    pts = 0.1 * torch.randn(P, 3, generator=g)
    x0 = xq.float() * X_SCALE
    out = {"x_q": xq.numpy(), "pts": pts.numpy(), "scales": np.array([X_SCALE, W_SCALE, C_SCALE]), "radius": np.array(0.001)}

    for tag, make, K in (("v", lambda: ref.vert_valid(CF), 1), ("r", lambda: ref.vert_pos_refinement(CF, radius=0.001), 3)):
        torch.manual_seed(5)
        m = make().eval()
        for k, v in m.state_dict().items():
            out[f"init_{tag}.{k}"] = np.array(v.shape)
        vals = {"ln_weight": 1.0 + 0.3 * torch.randn(D, generator=g), "ln_bias": 0.2 * torch.randn(D, generator=g),
                "fc1_weight": torch.randint(-48, 49, (Hd, D), generator=g, dtype=torch.int8),
                "fc1_bias": 0.2 * torch.randn(Hd, generator=g),
                "fc2_weight": torch.randint(-80, 81, (Hd, Hd), generator=g, dtype=torch.int8),
                "fc2_bias": 0.2 * torch.randn(Hd, generator=g),
                "fc_weight": 0.4 * torch.randn(K, Hd, generator=g), "fc_bias": 0.1 * torch.randn(K, generator=g)}
        for k in QUANTISED:
            vals[k][vals[k] == 0] = 1                                # non-zero weights
            out[f"{tag}_{k}_q"] = vals[k].numpy()
            vals[k] = vals[k].float() * W_SCALE
        sd = m.state_dict()

        def load():
            with torch.no_grad():
                for k, key in KEYS.items():
                    sd[key].copy_(vals[k])

        load()
        if tag == "v":                                               # spread the gate's logits over roughly +-4 ...
            with torch.no_grad():
                logit = m.fc(m.ff(torch.cat([x0, pts], dim=-1)))
            raw = logit - vals["fc_bias"]
            scale = 2.5 / float(raw.std())
            vals["fc_weight"] = vals["fc_weight"] * scale
            vals["fc_bias"] = vals["fc_bias"] - scale * float(raw.mean())          # ... around its bias
            load()
        for k in KEYS:
            if k not in QUANTISED:
                out[f"{tag}_{k}"] = vals[k].numpy()
            assert float(vals[k].abs().min()) > 0, k
        x = x0.clone().requires_grad_(True)
        p = pts.clone().requires_grad_(True)
        y = m(x, p)
        assert tuple(y.shape) == (P, K)
        cq = torch.randint(-24, 25, y.shape, generator=g, dtype=torch.int8)
        (y * (cq.float() * C_SCALE)).sum().backward()
        out[f"{tag}_out"], out[f"{tag}_cot_q"] = y.detach().numpy(), cq.numpy()
        out[f"{tag}_grad_pts"], out[f"{tag}_grad_x8"] = p.grad.numpy(), x.grad[::8].numpy()
        params = dict(m.named_parameters())
        for k, key in KEYS.items():
            out[f"{tag}_grad_{k}"] = params[key].grad.numpy()
        if tag == "v":
            s = y.detach()[:, 0]
            n_lo, n_mid, n_hi = int((s < 0.1).sum()), int(((s > 0.1) & (s < 0.9)).sum()), int((s > 0.9).sum())
            margin = float(torch.minimum((s - 0.1).abs(), (s - 0.9).abs()).min())
            print(f"scores: {n_lo} below 0.1, {n_mid} between, {n_hi} above 0.9; closest to a threshold {margin:.3e}")
            if min(n_lo, n_mid, n_hi) < 8 or margin < 1e-3:
                sys.exit(f"seed {SEED} does not meet the fixture's conditions")

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
