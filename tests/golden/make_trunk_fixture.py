#!/usr/bin/env python
"""Generate tests/golden/trunk_fixture.npz by running the REFERENCE's forward_gs statements (tgs/models/renderer_one_shot.py:254-257:
`x = self.mlp_net(x)`, `return self.gs_net(x, p)`) on the CPU, with its own MLP (tgs/models/networks.py:57-105) and GSLayer.

Runs only where the reference tree is present; the resulting .npz is data (inputs, weights and recorded outputs) and is committed;
nothing of the reference travels. The reference modules are imported under the stub modules of make_host_fixtures.py. Forward and
backward run on P = 64 points for four configurations:

    a   silu   Cin 131   H 128   RGB head, restrict_offset             c   relu   Cin 131   H 128   RGB head, free offset
    b   silu   Cin 128   H 128   SH-48 head, clip_scaling 0.005        d   silu   Cin 131   H 64    RGB head, restrict_offset

Stored small: features, weights and cotangents as int8 (`*_q`, value = q * scale, `scales` = x, w, cotangent); every case uses the
leading rows and columns of the same four weight matrices. Per configuration <t>:

    <t>_cfg                       Cin, H, Cout, shs width, use_rgb, restrict_offset, relu, clip (-1 = None)
    <t>_b1, _b2, _b3, _bh         the biases (float32; bh: the five heads' concatenated in feature_channels order)
    <t>_{xyz,scaling,rotation,opacity,shs}          the outputs
    <t>_cot_<field>_q             the fixed cotangents; <t>_grad_pts and <t>_grad_x16 (every 16th row of grad_x): the gradients of
                                  sum(output * cotangent)
    init_keys, init_shapes        the state dict MLP(131, 128, n_neurons=128, n_hidden_layers=2, activation="silu") starts with

For the ReLU case every float64 hidden pre-activation, and for the clip case every exp(raw scaling) - clip, lies farther than
2^-16 * the field's largest magnitude from its kink, with values on both sides: SEED is the first seed for which both hold (the
search runs here, on the CPU, and is asserted again on every run).

Usage: python tests/golden/make_trunk_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trunk_fixture.npz")
P, CMAX, HMAX, OMAX = 64, 131, 128, 59
X_SCALE, W_SCALE, C_SCALE = 1.0 / 16, 1.0 / 192, 1.0 / 8
GUARD = 2.0 ** -16
FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
#            activation, Cin, H, use_rgb, restrict_offset, clip
CASES = {"a": ("silu", 131, 128, True, True, None), "b": ("silu", 128, 128, False, True, 0.005),
         "c": ("relu", 131, 128, True, False, None), "d": ("silu", 131, 64, True, True, None)}


def make_head(ref, cin, use_rgb, restrict, clip):
    m = ref.GSLayer.__new__(ref.GSLayer)
    torch.nn.Module.__init__(m)
    m.cfg = types.SimpleNamespace(in_channels=cin, feature_channels={"xyz": 3, "scaling": 3, "rotation": 4, "opacity": 1, "shs": 48},
                                  xyz_offset=True, restrict_offset=restrict, use_rgb=use_rgb, clip_scaling=clip, init_scaling=-5.0,
                                  init_density=0.1)
    m.configure()
    return m


def draw(seed):
    """The shared inputs and weights of one seed, and each case's biases."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, dtype=torch.int8)
    d = {"x_q": ri(-40, 40, P, CMAX), "W1_q": ri(-31, 31, HMAX, CMAX), "W2_q": ri(-31, 31, HMAX, HMAX), "W3_q": ri(-31, 31, HMAX, HMAX),
         "Wh_q": ri(-31, 31, OMAX, HMAX), "pts": 0.1 * torch.randn(P, 3, generator=g)}
    for t, (_, _, H, use_rgb, _, clip) in CASES.items():
        O = 11 + (3 if use_rgb else 48)
        d[f"{t}_b1"], d[f"{t}_b2"], d[f"{t}_b3"] = (0.2 * torch.randn(n, generator=g) for n in (H, H, HMAX))
        bh = 0.5 * torch.randn(O, generator=g)
        bh[3:6] = float(np.log(clip)) if clip is not None else bh[3:6] - 5.0     # raw scalings on both sides of log(clip)
        d[f"{t}_bh"] = bh
    return d


def weights(d, t):
    _, cin, H, use_rgb, _, _ = CASES[t]
    O = 11 + (3 if use_rgb else 48)
    f = lambda k: d[k].float() * W_SCALE
    return (f("W1_q")[:H, :cin].contiguous(), d[f"{t}_b1"], f("W2_q")[:H, :H].contiguous(), d[f"{t}_b2"], f("W3_q")[:, :H].contiguous(),
            d[f"{t}_b3"], f("Wh_q")[:O].contiguous(), d[f"{t}_bh"])


def kinks_ok(d):
    """The margins of the ReLU case's hidden pre-activations and of the clip case's scalings, in float64."""
    act, cin, _, _, _, _ = CASES["c"]
    W1, b1, W2, b2 = (w.double() for w in weights(d, "c")[:4])
    x = d["x_q"][:, :cin].double() * X_SCALE
    v1 = F.linear(x, W1, b1)
    v2 = F.linear(torch.relu(v1), W2, b2)
    ok = all(float(v.abs().min()) > GUARD * float(v.abs().max()) and bool((v > 0).any()) and bool((v < 0).any()) for v in (v1, v2))
    _, cin, _, _, _, clip = CASES["b"]
    W1, b1, W2, b2, W3, b3, Wh, bh = (w.double() for w in weights(d, "b"))
    x = d["x_q"][:, :cin].double() * X_SCALE
    y = F.linear(F.silu(F.linear(F.silu(F.linear(x, W1, b1)), W2, b2)), W3, b3)
    s = torch.exp(F.linear(y, Wh[3:6], bh[3:6]))
    return ok and float((s - clip).abs().min()) > GUARD * float(s.abs().max()) and bool((s > clip).any()) and bool((s < clip).any())


SEED = next(s for s in range(1000) if kinks_ok(draw(s)))


def main():
    host.install_stubs([])
    sys.path.insert(0, host.REF)
    import tgs.models.renderer_one_shot as ref
    from tgs.models.networks import MLP

    d = draw(SEED)
    assert kinks_ok(d)
    out = {k: v.numpy() for k, v in d.items()}
    out["scales"], out["seed"] = np.array([X_SCALE, W_SCALE, C_SCALE]), np.array(SEED)
    sd = MLP(131, 128, n_neurons=128, n_hidden_layers=2, activation="silu").state_dict()
    out["init_keys"], out["init_shapes"] = np.array(list(sd)), np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()])

    g = torch.Generator().manual_seed(1000 + SEED)
    for t, (act, cin, H, use_rgb, restrict, clip) in CASES.items():
        W1, b1, W2, b2, W3, b3, Wh, bh = weights(d, t)
        mlp = MLP(cin, HMAX, n_neurons=H, n_hidden_layers=2, activation=act)
        head = make_head(ref, HMAX, use_rgb, restrict, clip)
        width = 3 if use_rgb else 48
        with torch.no_grad():
            for layer, W, b in zip((mlp.layers[0], mlp.layers[2], mlp.layers[4]), (W1, W2, W3), (b1, b2, b3)):
                layer.weight.copy_(W); layer.bias.copy_(b)
            o = 0
            for layer in head.out_layers:
                n = layer.out_features
                layer.weight.copy_(Wh[o:o + n]); layer.bias.copy_(bh[o:o + n])
                o += n
        assert o == 11 + width
        x = (d["x_q"][:, :cin].float() * X_SCALE).requires_grad_(True)
        p = d["pts"].clone().requires_grad_(True)
        gm = head(mlp(x), p)                                          # forward_gs's two statements
        loss = 0
        for k in FIELDS:
            v = getattr(gm, k)
            cq = torch.randint(-24, 25, v.shape, generator=g, dtype=torch.int8)
            out[f"{t}_{k}"], out[f"{t}_cot_{k}_q"] = v.detach().numpy(), cq.numpy()
            loss = loss + (v * (cq.float() * C_SCALE)).sum()
        loss.backward()
        out[f"{t}_cfg"] = np.array([cin, H, HMAX, width, int(use_rgb), int(restrict), int(act == "relu"), -1.0 if clip is None else clip])
        out[f"{t}_grad_pts"], out[f"{t}_grad_x16"] = p.grad.numpy(), x.grad[::16].numpy()

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 200_000, size
    print(f"wrote {OUT}: seed {SEED}, {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
