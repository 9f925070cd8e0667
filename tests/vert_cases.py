"""What tests/test_gpu_vert_mlp.py and tests/row_block_edge_cases.py share: the random inputs of the fused vertex MLP block
(guassianhand_amd/vert_mlp.py) and one forward + backward of it in the three modes of the three-way rule. Nothing here touches a
device unless it is handed one."""
import torch

ACT = {1: "sigmoid", 3: "tanh_offset"}


def names():
    from guassianhand_amd import vert_mlp as V
    return ("grad_x", "grad_pts") + tuple(f"grad_{k}" for k in V.PARAMS)


def make_inputs(dev, P, Cf=131, K=1, seed=0):
    """x ~ N(0,1), pts ~ N(0, 0.1^2); LayerNorm weight 1 + N(0, 0.3^2); Linear weights N(0, 1/fan_in) (the gate's head twice that, so that
    its scores leave the middle); every bias non-zero; one cotangent."""
    from guassianhand_amd import vert_mlp as V
    g = torch.Generator().manual_seed(1000 * seed + P + 7 * Cf + K)
    D = Cf + 3
    Hd = D // 4
    r = lambda *s: torch.randn(*s, generator=g)
    x, pts = r(P, Cf), 0.1 * r(P, 3)
    params = [1.0 + 0.3 * r(D), 0.2 * r(D), r(Hd, D) / D ** 0.5, 0.2 * r(Hd), r(Hd, Hd) / Hd ** 0.5, 0.2 * r(Hd),
              (2.0 if K == 1 else 1.0) * r(K, Hd) / Hd ** 0.5, 0.2 * r(K)]
    assert [tuple(p.shape) for p in params] == list(V.param_shapes(Cf, K))
    return [t.to(dev) for t in [x, pts] + params], r(P, K).to(dev)


def run(mode, inputs, cot, K, frozen=False, radius=0.001):
    """One forward + backward -> {out, grad_x, grad_pts, grad_<param>}. mode: 'f64' | 'torch32' | 'kernel'."""
    from guassianhand_amd import vert_mlp as V
    leaves = [t.detach().clone().requires_grad_(not (frozen and i >= 2)) for i, t in enumerate(inputs)]
    kw = dict(act=ACT[K], radius=radius, eps=1e-6)
    if mode == "f64":
        out = V._vert_block_ref(leaves[0], leaves[1], leaves[2:], **kw, acc=torch.float64)
    else:
        out = V.vert_block(leaves[0], leaves[1], leaves[2:], **kw, ops="torch" if mode == "torch32" else "fused")
    res = {"out": out.detach()}
    (out * cot.to(out.dtype)).sum().backward()
    for name, leaf in zip(names(), leaves):
        if leaf.requires_grad:
            res[name] = leaf.grad
    return res
