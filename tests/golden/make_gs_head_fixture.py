#!/usr/bin/env python
"""Generate tests/golden/gs_head_fixture.npz by running the REFERENCE's GSLayer (tgs/models/renderer_one_shot.py:156-214) on the CPU.

Runs only where the reference tree is present; the resulting .npz is data (inputs, weights and recorded outputs) and is committed;
nothing of the reference travels. The reference module is imported under the stub modules of make_host_fixtures.py; GSLayer is built
the reference's way (configure() on a stand-in cfg), its initial state dict is recorded, then random non-zero weights are loaded and
forward + backward run on P = 64 points for four configurations that between them cover Cin in {128, 131}, the RGB head and the
48-wide SH head, clip_scaling None and 0.005, and both offset forms:

    a   Cin 128   use_rgb   restrict_offset   clip None          c   Cin 128   SH-3   restrict_offset   clip 0.005
    b   Cin 131   use_rgb   free offset       clip 0.005         d   Cin 131   SH-3   free offset       clip None

Stored small: features are multiples of 1/16 and weights multiples of 1/256, kept as int8 (`*_q`, value = q * scale) — their
products and 131-term sums are exact in float32 (the biases lie on the same grid), so the five separate nn.Linear calls of the reference and one concatenated
F.linear give the same pre-activations bit for bit on any host. Per configuration <t>:

    <t>_cfg                       Cin, shs width, use_rgb, restrict_offset, xyz_offset, clip (-1 = None)
    <t>_bias                      the five heads' biases concatenated in feature_channels order (weights: W_q[:O, :Cin])
    <t>_{xyz,scaling,rotation,opacity,shs}          GSLayer.forward's outputs
    <t>_cot_<field>_q             the fixed cotangents (int8, multiples of 1/8); <t>_grad_pts, <t>_grad_bias, <t>_grad_x16 (every 16th
                                  row of grad_x) and, for `a`, <t>_grad_weight: the gradients of sum(output * cotangent)
    init_<rgb|sh>.<key>           the state dict configure() leaves (zero weights are stored as their shape only)

Usage: python tests/golden/make_gs_head_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gs_head_fixture.npz")
P, CMAX, OMAX = 64, 131, 59
X_SCALE, W_SCALE, C_SCALE = 1.0 / 16, 1.0 / 256, 1.0 / 8
FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
CASES = {"a": (128, True, True, None), "b": (131, True, False, 0.005), "c": (128, False, True, 0.005), "d": (131, False, False, None)}


def make_layer(ref, cin, use_rgb, restrict, clip):
    m = ref.GSLayer.__new__(ref.GSLayer)
    torch.nn.Module.__init__(m)
    m.cfg = types.SimpleNamespace(in_channels=cin, feature_channels={"xyz": 3, "scaling": 3, "rotation": 4, "opacity": 1, "shs": 48},
                                  xyz_offset=True, restrict_offset=restrict, use_rgb=use_rgb, clip_scaling=clip, init_scaling=-5.0,
                                  init_density=0.1)
    m.configure()
    return m


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    import tgs.models.renderer_one_shot as ref

    g = torch.Generator().manual_seed(31)
    xq = torch.randint(-40, 41, (P, CMAX), generator=g, dtype=torch.int8)
    wq = torch.randint(-24, 25, (OMAX, CMAX), generator=g, dtype=torch.int8)
    wq[wq == 0] = 1                                                   # non-zero weights
    pts = 0.1 * torch.randn(P, 3, generator=g)
    out = {"x_q": xq.numpy(), "W_q": wq.numpy(), "scales": np.array([X_SCALE, W_SCALE, C_SCALE]), "pts": pts.numpy()}

    for tag, use_rgb in (("rgb", True), ("sh", False)):
        torch.manual_seed(5)                                          # (the RGB head keeps nn.Linear's own random initialisation)
        for k, v in make_layer(ref, 128, use_rgb, False, None).state_dict().items():
            out[f"init_{tag}.{k}"] = np.array(v.shape) if float(v.abs().max()) == 0 else v.numpy()

    for t, (cin, use_rgb, restrict, clip) in CASES.items():
        m = make_layer(ref, cin, use_rgb, restrict, clip)
        width = 3 if use_rgb else 48
        O = 11 + width
        bias = 0.5 * torch.randn(O, generator=g)
        bias[3:6] -= 5.0                                              # around the reference's init_scaling
        if clip is not None:
            bias[3:6] = float(np.log(clip))                           # raw scalings on both sides of log(clip)
        bias = torch.round(bias / W_SCALE) * W_SCALE                  # exact sums need the bias on the products' grid too
        W = wq[:O, :cin].float() * W_SCALE
        o = 0
        with torch.no_grad():
            for layer in m.out_layers:
                n = layer.out_features
                layer.weight.copy_(W[o:o + n]); layer.bias.copy_(bias[o:o + n])
                o += n
        assert o == O
        x = (xq[:, :cin].float() * X_SCALE).requires_grad_(True)
        p = pts.clone().requires_grad_(True)
        gm = m(x, p)
        loss = 0
        for k in FIELDS:
            v = getattr(gm, k)
            cq = torch.randint(-24, 25, v.shape, generator=g, dtype=torch.int8)
            cot = cq.float() * C_SCALE
            out[f"{t}_{k}"], out[f"{t}_cot_{k}_q"] = v.detach().numpy(), cq.numpy()
            loss = loss + (v * cot).sum()
        loss.backward()
        out[f"{t}_cfg"] = np.array([cin, width, int(use_rgb), int(restrict), 1, -1.0 if clip is None else clip])
        out[f"{t}_bias"] = bias.numpy()
        out[f"{t}_grad_pts"], out[f"{t}_grad_x16"] = p.grad.numpy(), x.grad[::16].numpy()
        out[f"{t}_grad_bias"] = torch.cat([layer.bias.grad for layer in m.out_layers]).numpy()
        if t == "a":
            out[f"{t}_grad_weight"] = torch.cat([layer.weight.grad for layer in m.out_layers]).numpy()
        if clip is not None:
            s = torch.nn.functional.linear(x.detach(), W[3:6], bias[3:6])
            assert (s < np.log(clip)).any() and (s > np.log(clip)).any(), "raw scalings on one side of the clamp only"

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
