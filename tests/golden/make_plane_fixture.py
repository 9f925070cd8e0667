#!/usr/bin/env python
"""Generate tests/golden/plane_fixture.npz by running the REFERENCE's GS3DRenderer.query_triplane_texture
(tgs/models/renderer_one_shot.py:420-446) on the CPU.

Runs only where the reference tree is present; the resulting .npz is data (inputs and recorded outputs) and is committed; nothing of
the reference travels. The reference module is imported under the stub modules of make_host_fixtures.py and the method is called
unbound on an object that carries `cfg.radius_texture` alone.

Two planes, N = 64 points: `big` is C = 80 on 64 x 128 (the texture code's shape), `small` is C = 3 on 5 x 7. Per plane the UVs hold
the four corners (exactly +-1), the centre, two points on an edge, four points just outside the map (|u| or |v| = 1 + 2^-10 and
1.05) and uniform points in [-1, 1]. Per radius_texture r in (1.0, 0.5) the positions are uv * r, and the method runs batched
((1,N,2), (1,1,C,Hp,Wp)) and unbatched ((N,2), (1,C,Hp,Wp)).

Stored small: plane values are multiples of 1/4 in [-3/4, 3/4] kept as int8 (`*_plane_q`, value = q / 4), cotangents multiples of
1/8 as int8 (`*_cot_q`); an array that equals an earlier one bit for bit is stored once and listed in `aliases` as
"name=stored name" (tests/helpers.py: GoldenNpz) — the unbatched results, where they equal the batched ones.

    <p>_plane_q, <p>_uv, <p>_cot_q                 p = big | small
    <p>_r<r>_pos                                   positions for radius r (r = 1.0 | 0.5)
    <p>_r<r>_<form>_out                            form = batched | unbatched: the method's result, as (N,C)
    <p>_r<r>_<form>_grad                           the autograd gradient of sum(out * cot) with respect to the plane, (C,Hp,Wp)

Usage: python tests/golden/make_plane_fixture.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = host.REF
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_fixture.npz")
N, SEED = 64, 11
SHAPES = {"big": (80, 64, 128), "small": (3, 5, 7)}
RADII = (1.0, 0.5)


def make_uv(g):
    uv = torch.rand(N, 2, generator=g) * 2.0 - 1.0
    eps = 2.0 ** -10
    fixed = [[-1, -1], [1, -1], [-1, 1], [1, 1], [0, 0], [1, 0.25], [-0.5, -1],
             [1 + eps, 0.3], [-0.2, -1 - eps], [1.05, 1.05], [-1.05, 0.7]]
    uv[:len(fixed)] = torch.tensor(fixed, dtype=torch.float32)
    return uv


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    import tgs.models.renderer_one_shot as ref

    g = torch.Generator().manual_seed(SEED)
    out, aliases = {"radii": np.array(RADII)}, []

    def store(name, value):
        value = np.ascontiguousarray(value)
        for k, v in out.items():
            if v.shape == value.shape and v.dtype == value.dtype and v.tobytes() == value.tobytes():
                aliases.append(f"{name}={k}")
                return
        out[name] = value

    for tag, (C, Hp, Wp) in SHAPES.items():
        pq = torch.randint(-3, 4, (C, Hp, Wp), generator=g, dtype=torch.int8)
        uv = make_uv(g)
        cq = torch.randint(-24, 25, (N, C), generator=g, dtype=torch.int8)
        out[f"{tag}_plane_q"], out[f"{tag}_uv"], out[f"{tag}_cot_q"] = pq.numpy(), uv.numpy(), cq.numpy()
        plane, cot = pq.float() / 4.0, cq.float() / 8.0
        for r in RADII:
            me = SimpleNamespace(cfg=SimpleNamespace(radius_texture=r))
            pos = uv * r
            out[f"{tag}_r{r}_pos"] = pos.numpy()
            for form in ("batched", "unbatched"):
                p = plane.clone().requires_grad_(True)
                if form == "batched":
                    res = ref.GS3DRenderer.query_triplane_texture(me, pos[None], p[None, None])
                    assert tuple(res.shape) == (1, N, C)
                    (res[0] * cot).sum().backward()
                else:
                    res = ref.GS3DRenderer.query_triplane_texture(me, pos, p[None])
                    assert tuple(res.shape) == (N, C)
                    (res * cot).sum().backward()
                store(f"{tag}_r{r}_{form}_out", res.detach().numpy().reshape(N, C))
                store(f"{tag}_r{r}_{form}_grad", p.grad.numpy())
    out["aliases"] = np.array(aliases)
    print("aliases:", aliases)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 600_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
