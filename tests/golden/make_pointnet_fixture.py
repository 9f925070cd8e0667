#!/usr/bin/env python
"""Generate tests/golden/pointnet_fixture.npz by running the REFERENCE's LocalPoolPointnet
(tgs/models/pointclouds/pointnet_texture.py) on the CPU.

Runs only where the reference tree is present; the resulting .npz is data (inputs, weights and recorded outputs) and is
committed; nothing of the reference travels. The reference module is imported under the stub modules of make_host_fixtures.py;
its two torch_scatter functions are replaced by the pure-torch stand-ins below, which follow torch_scatter's documented
semantics (argmax returned, T for empty cells, the gradient of a maximum sent to the argmax only) with the lowest point index
winning a tie. For scatter_type "max" and "mean" it records

    p                    the input cloud (1,T,D); its first two columns choose the UV cell
    w.<key>              the state dict (shared by both types)
    <type>_index         the per-point cell index the reference computes
    <type>_pooled<k>_cells   what pool_local returned before block k = 1..4, one row per cell: pooled = cells[index]
    <type>_plane         the returned (1, c_dim, plane, plane) features
    cot, <type>_grad_p, <type>_grad_fc_pos_w    a fixed cotangent of the plane and its gradients
    max_scatter_out / max_scatter_arg           scatter_max's two outputs for the first pooled layer
    <type>_op_*          one pool_local and one plane call on recorded inputs with their gradients (the per-op checks)

Usage: python tests/golden/make_pointnet_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pointnet_fixture.npz")
T, D, HID, CDIM, PLANE, BLOCKS, RADIUS = 2000, 6, 16, 16, 8, 5, 1.0


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    B, C, N = src.shape
    idx = index.expand(B, C, N)
    s = src.detach()
    amax = torch.full((B, C, dim_size), float("-inf")).scatter_reduce(2, idx, s, "amax", include_self=True)
    pts = torch.arange(N).expand(B, C, N)
    cand = torch.where(s == amax.gather(2, idx), pts, torch.full_like(pts, N))
    arg = torch.full((B, C, dim_size), N, dtype=torch.int64).scatter_reduce(2, idx, cand, "amin", include_self=True)
    vals = src.gather(2, arg.clamp(max=N - 1))
    return torch.where(arg == N, torch.zeros_like(vals), vals), arg


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    B, C, N = src.shape
    n = out.shape[2] if out is not None else dim_size
    sums = torch.zeros(B, C, n).scatter_add(2, index.expand(B, C, N), src)
    cnt = torch.zeros(B, 1, n).scatter_add(2, index, torch.ones(B, 1, N)).clamp(min=1)
    res = sums / cnt
    if out is None:
        return res
    out.add_(res)
    return out


def make_input(g):
    """A dense blob (cells with hundreds of points), a thin uniform spray reaching beyond both clamp edges (cells with one point,
    cells with none), points exactly on the edges, and a few exact duplicate rows (ties of every channel's maximum)."""
    blob = torch.tensor([0.3, -0.2]) + 0.22 * torch.randn(T - 60, 2, generator=g)
    spray = (torch.rand(44, 2, generator=g) * 2 - 1) * 1.3
    edge = torch.tensor([[1.0, 0.1], [-1.0, 0.2], [0.4, 1.0], [0.3, -1.0], [2.0, 2.0], [-2.0, -2.0], [1.0, -1.0], [-1.0, 1.0]])
    uv = torch.cat([blob, spray, edge])
    p = torch.cat([uv, torch.randn(uv.shape[0], D - 2, generator=g)], dim=1)
    p = torch.cat([p, p[[5, 5, 17, 400, 401, 1999 - 60, 3, 3]]])          # duplicates (the second of a pair has the higher index)
    assert p.shape == (T, D), p.shape
    return p[torch.randperm(T, generator=g)].unsqueeze(0).contiguous()


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    import tgs.models.pointclouds.pointnet_texture as ref
    ref.scatter_max, ref.scatter_mean = scatter_max, scatter_mean

    g = torch.Generator().manual_seed(20)
    p = make_input(g)
    out = {"p": p.numpy(), "dims": np.array([T, D, HID, CDIM, PLANE, BLOCKS]), "radius": np.array(RADIUS)}
    cot = torch.randn(1, CDIM, PLANE, PLANE, generator=g)
    op_cot = torch.randn(T, HID, generator=g)
    out["cot"], out["op_pool_cot"] = cot.numpy(), op_cot.numpy()
    weights = None
    for kind in ("max", "mean"):
        m = ref.LocalPoolPointnet.__new__(ref.LocalPoolPointnet)
        torch.nn.Module.__init__(m)
        m.cfg = types.SimpleNamespace(input_channels=D, c_dim=CDIM, hidden_dim=HID, scatter_type=kind, plane_size=PLANE,
                                      n_blocks=BLOCKS, radius=RADIUS)
        m.configure()
        if weights is None:
            weights = {}
            for k, v in m.state_dict().items():
                w = torch.randn(v.shape, generator=g) * (v.shape[-1] ** -0.5 if v.dim() == 2 else 0.1)
                weights[k] = w
                out[f"w.{k}"] = w.numpy()
        m.load_state_dict(weights)
        nets, pooled, cs, idxs = [], [], [], []
        orig_pool, orig_c2i = m.pool_local, m.coordinate2index

        def rec_pool(xy, index, c):
            r = orig_pool(xy, index, c)
            nets.append(c.detach().clone())
            pooled.append(r.detach().clone())
            return r

        def rec_index(x):
            r = orig_c2i(x)
            idxs.append(r.clone())
            return r

        m.pool_local, m.coordinate2index = rec_pool, rec_index
        m.fc_c.register_forward_hook(lambda mod, a, o: cs.append(o.detach().clone()))
        pin = p.clone().requires_grad_(True)
        plane = m(pin)
        plane.backward(cot)
        index = idxs[0][0, 0]
        assert len(pooled) == BLOCKS - 1 and plane.shape == (1, CDIM, PLANE, PLANE)
        out[f"{kind}_index"] = index.numpy()
        for k, t in enumerate(pooled, 1):
            # every point of a cell holds the same row: stored once per cell (zeros for empty cells), pooled = cells[index]
            cells = torch.zeros(PLANE ** 2, HID)
            cells[index] = t[0]
            assert torch.equal(cells[index], t[0])
            out[f"{kind}_pooled{k}_cells"] = cells.numpy()
        out[f"{kind}_plane"] = plane.detach().numpy()
        out[f"{kind}_grad_p"] = pin.grad.numpy()
        out[f"{kind}_grad_fc_pos_w"] = m.fc_pos.weight.grad.numpy()
        # per-op records on recorded inputs
        x1 = nets[0].clone().requires_grad_(True)
        r = orig_pool({"xy": None}, {"xy": idxs[0]}, x1)
        r.backward(op_cot.unsqueeze(0))
        assert torch.equal(r.detach(), pooled[0])
        out[f"{kind}_op_pool_in"], out[f"{kind}_op_pool_grad"] = nets[0][0].numpy(), x1.grad[0].numpy()
        c1 = cs[0].clone().requires_grad_(True)
        pl = m.generate_plane_features(idxs[0], c1)
        pl.backward(cot)
        assert torch.equal(pl.detach(), plane.detach())
        out[f"{kind}_op_plane_in"], out[f"{kind}_op_plane_grad"] = cs[0][0].numpy(), c1.grad[0].numpy()
        if kind == "max":
            v, a = scatter_max(nets[0].permute(0, 2, 1), idxs[0], dim_size=PLANE ** 2)
            out["max_scatter_out"], out["max_scatter_arg"] = v[0].numpy(), a[0].numpy()
            counts = torch.bincount(index, minlength=PLANE ** 2)
            uv = p[0, :, :2]
            assert (counts == 0).any(), "no empty cell"
            assert (counts == 1).any(), "no cell with one point"
            assert counts.max() >= 200, f"fullest cell holds {int(counts.max())}"
            assert (uv[:, 0] >= RADIUS).any() and (uv[:, 0] <= -RADIUS).any(), "no point on both clamp edges of x"
            assert (uv[:, 1] >= RADIUS).any() and (uv[:, 1] <= -RADIUS).any(), "no point on both clamp edges of y"
            assert index.min() >= 0 and index.max() < PLANE ** 2
            print(f"cells: {int((counts == 0).sum())} empty, {int((counts == 1).sum())} with one point, fullest {int(counts.max())}")
        else:
            assert torch.equal(index, torch.from_numpy(out["max_index"]))

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
