#!/usr/bin/env python
"""Generate tests/golden/self_attn_fixture.npz by running the REFERENCE's SelfAttn(131) (tgs/models/self_attn.py:36-85) on the CPU in
eval() mode.

Runs only where the reference tree is present; the resulting .npz is data (inputs, parameters and recorded outputs) and is committed;
nothing of the reference travels. The reference module is imported under the stub modules of make_host_fixtures.py. The module is built
the reference's way, its initial state dict is recorded (keys and shapes), then random non-zero parameters (every bias and both
LayerNorms' weights too) are loaded and forward + backward run on V = 48 rows, once for the whole module and once for `self_attn`
alone.

Stored small (the six 131-wide matrices and their gradients would be 0.8 MB as float32): the input is multiples of 1/16 and the six
matrices are +-1 or +-2 times a per-matrix scale, kept as int8 (`*_q`, value = q * scale); outputs and the gradient of x keep every
fourth row; of the gradients of the six matrices every 64th row is kept, and of ALL their rows one signed sum each (`_proj`: row i
times the fixed signs s_j = +1, -1, -1, +1, -1, ... of `proj_signs`, summed in float64 and rounded once), so that no row and no element
of a matrix's gradient goes unseen.

    x_q, x_scale                   the (1, 48, 131) input
    <key>_q, <key>_scale           w_qs.weight, w_ks.weight, w_vs.weight, fc.weight, ff.fc1.weight, ff.fc2.weight
    <key>                          every bias and LayerNorm tensor (float32)
    cot_q, cot_scale               the fixed cotangent of the module output (and of self_attn's)
    out_r4, grad_x_r4              rows ::4 of module(x) and of the gradient of sum(out * cot) in x
    attn_out_r4, attn_grad_x_r4    the same for module.self_attn(x) alone
    grad.<key>                     the module run's gradient of every parameter (`grad.<key>_r64`: rows ::64 of the six matrices,
                                   `grad.<key>_proj`: the signed sum of every row)
    init.<key>                     the shape of every entry of the initial state dict
    score_max                      the largest |score| (q.k / norm) of the module run

`w_qs.weight` is scaled so that the largest |score| is 8, and the script ASSERTS (exit status non-zero otherwise) that scores reach
below -5 and above 5 in every head and that the largest probability of a row averages above 0.2 (uniform would be 1/48): the softmax
is far from uniform, so an error in the running maximum or sum shows.

Usage: python tests/golden/make_self_attn_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "self_attn_fixture.npz")
V, F_DIM, SEED = 48, 131, 11
X_SCALE, C_SCALE = 1.0 / 16, 1.0 / 2
MATRICES = {"w_qs.weight": 1.0 / 16, "w_ks.weight": 1.0 / 16, "w_vs.weight": 1.0 / 16, "fc.weight": 1.0 / 16, "ff.fc1.weight": 1.0 / 16,
            "ff.fc2.weight": 1.0 / 32}
ROWS, W_ROWS = 4, 64


def proj_signs(n):
    """+-1 per column, fixed: the parity of j + j // 3 + j // 7 (tests/self_attn_cases.py restates it)."""
    j = torch.arange(n)
    return (1 - 2 * ((j + j // 3 + j // 7) % 2)).double()


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    import tgs.models.self_attn as ref

    g = torch.Generator().manual_seed(SEED)
    torch.manual_seed(5)
    m = ref.SelfAttn(F_DIM).eval()
    sd = m.state_dict()
    out = {f"init.{k}": np.array(v.shape) for k, v in sd.items()}
    xq = torch.randint(-40, 41, (1, V, F_DIM), generator=g, dtype=torch.int8)
    x0 = xq.float() * X_SCALE
    out.update(x_q=xq.numpy(), x_scale=np.array(X_SCALE))

    vals, quant, scale = {}, {}, dict(MATRICES)
    for key, t in sd.items():
        if key in MATRICES:
            w = torch.randint(1, 3, t.shape, generator=g, dtype=torch.int8)
            quant[key] = w * (torch.randint(0, 2, t.shape, generator=g, dtype=torch.int8) * 2 - 1)
        elif key.endswith("layer_norm.weight"):
            vals[key] = 1.0 + 0.3 * torch.randn(t.shape, generator=g)
        else:
            vals[key] = 0.2 * torch.randn(t.shape, generator=g)

    def load():
        with torch.no_grad():
            for key in sd:
                sd[key].copy_(quant[key].float() * scale[key] if key in quant else vals[key])

    def scores():
        with torch.no_grad():
            z = m.layer_norm(x0)
            q = m.w_qs(z).view(1, V, m.n_heads, m.d_q).transpose(1, 2)
            k = m.w_ks(z).view(1, V, m.n_heads, m.d_q).transpose(1, 2)
            return torch.matmul(q, k.transpose(-1, -2)) / m.norm

    load()
    s = scores()
    # the scores are linear in w_qs.weight up to its bias's share: two steps land the largest |score| on 8
    for _ in range(4):
        scale["w_qs.weight"] *= 8.0 / float(s.abs().max())
        load()
        s = scores()
    smax = float(s.abs().max())
    per_head_lo, per_head_hi = s.amin(dim=(0, 2, 3)), s.amax(dim=(0, 2, 3))
    peak = float(torch.softmax(s, -1).amax(-1).mean())
    print(f"scores: max |s| {smax:.4f}, per head min {per_head_lo.tolist()}, max {per_head_hi.tolist()}; mean row peak {peak:.3f}")
    if abs(smax - 8.0) > 0.05 or float(per_head_lo.max()) > -5 or float(per_head_hi.min()) < 5 or peak < 0.2:
        sys.exit(f"seed {SEED} does not meet the fixture's conditions")
    out["score_max"] = np.array(smax)

    for key in sd:
        if key in quant:
            assert int((quant[key] == 0).sum()) == 0, key
            out[f"{key}_q"], out[f"{key}_scale"] = quant[key].numpy(), np.array(scale[key], dtype=np.float32)
            scale[key] = float(np.float32(scale[key]))                # what a reader of the file multiplies by
        else:
            assert float(vals[key].abs().min()) > 0, key
            out[key] = vals[key].numpy()
    load()

    cq = torch.randint(-4, 5, (1, V, F_DIM), generator=g, dtype=torch.int8)
    cot = cq.float() * C_SCALE
    out.update(cot_q=cq.numpy(), cot_scale=np.array(C_SCALE))

    x = x0.clone().requires_grad_(True)
    y = m(x)
    assert tuple(y.shape) == (1, V, F_DIM)
    (y * cot).sum().backward()
    out["out_r4"], out["grad_x_r4"] = y.detach()[:, ::ROWS].numpy(), x.grad[:, ::ROWS].numpy()
    for key, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, key
        if key in quant:
            out[f"grad.{key}_r64"] = p.grad[::W_ROWS].numpy().copy()                 # (the second run below adds to p.grad)
            out[f"grad.{key}_proj"] = (p.grad.double() @ proj_signs(p.shape[1])).float().numpy()
        else:
            out[f"grad.{key}"] = p.grad.numpy().copy()
    xa = x0.clone().requires_grad_(True)
    ya = m.self_attn(xa)
    (ya * cot).sum().backward()
    out["attn_out_r4"], out["attn_grad_x_r4"] = ya.detach()[:, ::ROWS].numpy(), xa.grad[:, ::ROWS].numpy()

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
