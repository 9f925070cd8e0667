"""What tests/test_self_attn_cpu.py and tests/test_gpu_self_attn.py share: the captured fixture as tensors, a stand-in for someone
else's SelfAttn class (the class `fuse_self_attn` grafts onto), and the error table of the criterion."""
import os

import numpy as np
import torch
import torch.nn as nn

from guassianhand_amd import attention as A

MATRICES = ("w_qs.weight", "w_ks.weight", "w_vs.weight", "fc.weight", "ff.fc1.weight", "ff.fc2.weight")
KEYS = tuple(f"{m}.{p}" for m in ("w_qs", "w_ks", "w_vs", "layer_norm", "fc", "ff.layer_norm", "ff.fc1", "ff.fc2") for p in ("weight", "bias"))
F_DIM, ROWS, W_ROWS = 131, 4, 64


def load_fixture(golden_dir):
    """(fx, x (1, 48, 131), cot, state dict) of tests/golden/self_attn_fixture.npz."""
    fx = np.load(os.path.join(golden_dir, "self_attn_fixture.npz"), allow_pickle=False)
    x = torch.tensor(fx["x_q"]).float() * float(fx["x_scale"])
    cot = torch.tensor(fx["cot_q"]).float() * float(fx["cot_scale"])
    state = {k: torch.tensor(fx[f"{k}_q"]).float() * float(fx[f"{k}_scale"]) if k in MATRICES else torch.tensor(fx[k]) for k in KEYS}
    return fx, x, cot, state


def sampled(key, grad):
    """The rows of a parameter's gradient that the fixture keeps, and the fixture's name for them."""
    return (f"grad.{key}_r64", grad[::W_ROWS]) if key in MATRICES else (f"grad.{key}", grad)


def proj_signs(n):
    """The fixture's +-1 per column: the parity of j + j // 3 + j // 7 (make_self_attn_fixture.py)."""
    j = torch.arange(n)
    return (1 - 2 * ((j + j // 3 + j // 7) % 2)).double()


def projected(key, grad, round32=True):
    """Every row of a matrix's gradient as one signed sum, formed in float64 (and rounded once to float32, as the fixture stores it;
    round32=False keeps the float64 value: the referee's), and the fixture's name for it."""
    p = grad.double() @ proj_signs(grad.shape[1]).to(grad.device)
    return f"grad.{key}_proj", (p.float() if round32 else p)


class PlainSelfAttn(nn.Module):
    """Someone else's SelfAttn: the same sub-modules and attributes under the same names, `self_attn` as torch statements with both
    dropouts, `forward` with the LayerNorm, the residual and `ff`. Not a subclass of attention.SelfAttn, so fuse_self_attn grafts it."""

    def __init__(self, f_dim=F_DIM, dropout=0.1):
        super().__init__()
        src = A.SelfAttn(f_dim, dropout=dropout)
        for name, child in src.named_children():
            setattr(self, name, child)
        self.n_heads, self.d_q, self.d_v, self.norm, self.f_dim = src.n_heads, src.d_q, src.d_v, src.norm, src.f_dim
        self.calls = 0

    def self_attn(self, x):
        self.calls += 1
        return A.SelfAttn._torch_self_attn(self, x)

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm(x))
        return self.ff(x)


def run_module(m, x, cot):
    """(output, grad of x, {key: grad}) of sum(m(x) * cot)."""
    for p in m.parameters():
        p.grad = None
    xx = x.detach().clone().requires_grad_(True)
    y = m(xx)
    (y * cot.to(y.dtype)).sum().backward()
    return y.detach(), xx.grad, {k: p.grad for k, p in m.named_parameters()}


def errors(name, got, ref64, yard, bound, bad):
    """Print the three errors of one field and note it in `bad` when got misses bound(e_yard)."""
    got, yard = got.double().reshape(ref64.shape), yard.double().reshape(ref64.shape)
    e_got, e_yard = float((got - ref64).abs().max()) if ref64.numel() else 0.0, float((yard - ref64).abs().max()) if ref64.numel() else 0.0
    limit = bound(e_yard)
    print(f"{name:28s} got-f64 {e_got:.3e}  yardstick-f64 {e_yard:.3e}  bound {limit:.3e}")
    if not e_got <= limit:
        bad.append((name, e_got, e_yard, limit))
