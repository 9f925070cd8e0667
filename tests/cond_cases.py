"""What tests/test_gpu_cond.py and tests/row_block_edge_cases.py share: the layouts and random inputs of the point conditioning
(guassianhand_amd/cond.py) and one forward + backward of it in the three modes of the three-way rule. Nothing here touches a device
unless it is handed one."""
import torch

from guassianhand_amd import cond

# name: (uv, xyz, flag, Cc, De, Hd, L)
LAYOUTS = {"full": (1, 1, 1, 33, 768, 51, 4), "de0": (1, 1, 1, 33, 0, 51, 4), "de1": (1, 1, 1, 33, 1, 51, 4),
           "nocode": (1, 1, 1, 0, 768, 51, 4), "uvcode": (1, 0, 0, 33, 768, 51, 4), "wide": (1, 1, 1, 64, 768, 64, 4),
           "hd1": (1, 1, 1, 33, 768, 1, 4), "l1": (1, 1, 1, 33, 768, 51, 1), "l8": (1, 1, 1, 33, 768, 51, 8)}


def make_case(dev, B, N, layout="full", seed=0, e_scale=1.0):
    """uv ~ U(0,1), xyz ~ N(0, 0.1^2), flag ~ Bernoulli(0.4), code ~ U(-1,1), broadcast ~ e_scale * N(0,1); LayerNorm weight
    1 + N(0, 0.3^2); Linear weights N(0, 1/fan_in); every bias non-zero; one cotangent."""
    uv, xyz, flag, Cc, De, Hd, L = LAYOUTS[layout]
    g = torch.Generator().manual_seed(1000 * seed + 31 * B + N + 7 * sorted(LAYOUTS).index(layout))
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"uv": torch.rand(B, N, 2, generator=g) if uv else None, "xyz": 0.1 * r(B, N, 3) if xyz else None,
         "flag": (torch.rand(B, N, 1, generator=g) < 0.4) if flag else None, "code": 2 * torch.rand(B, N, Cc, generator=g) - 1 if Cc else None,
         "e": e_scale * r(B, 1, De) if De else None}
    Dv = (4 + 4 * L if uv else 0) + (6 + 6 * L if xyz else 0) + (1 if flag else 0) + Cc
    D = Dv + De
    params = [1.0 + 0.3 * r(D), 0.2 * r(D), r(Hd, D) / D ** 0.5, 0.2 * r(Hd), r(Hd, Hd) / Hd ** 0.5, 0.2 * r(Hd)]
    mv = lambda v: None if v is None else v.to(dev)
    return {k: mv(v) for k, v in t.items()}, [p.to(dev) for p in params], r(B, N, Hd).to(dev), L


def point_rows(t, L, code=None):
    return cond.PointRows(uv=t["uv"], xyz=t["xyz"], flag=t["flag"], code=t["code"] if code is None else code,
                          broadcast=() if t["e"] is None else (t["e"],), levels=L)


def run(mode, case):
    """One forward + backward -> {out, grad_code}. mode: 'f64' | 'torch32' | 'kernel'."""
    t, params, cot, L = case
    code = None if t["code"] is None else t["code"].detach().clone().requires_grad_(True)
    rows = point_rows(t, L, code)
    if mode == "f64":
        out = cond._cond_mlp_ref(rows, params, acc=torch.float64)
    else:
        out = cond.cond_mlp(rows, params, ops="torch" if mode == "torch32" else "fused")
    res = {"out": out.detach()}
    if code is not None:
        (out * cot.to(out.dtype)).sum().backward()
        res["grad_code"] = code.grad
    return res
