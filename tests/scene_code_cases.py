"""What tests/test_scene_code_cpu.py and tests/test_gpu_scene_code.py share: the captured fixture as tensors, a stand-in for someone
else's TriplaneUpsampleNetwork (the class `fused_upsample_cls` grafts onto), one way to run forward + backward on any path, and the
scales of the criterion."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from guassianhand_amd import scene_code as SC


class PlainUpsample(nn.Module):
    """Someone else's TriplaneUpsampleNetwork: `upsample` and `cfg.n_plane` under the reference's names, `forward` as torch
    statements. Not a subclass of scene_code.TriplaneUpsampleNetwork, so fused_upsample_cls grafts it."""

    def __init__(self, in_channels, out_channels, n_plane, kernel_size=2, stride=2):
        super().__init__()
        self.cfg = SimpleNamespace(in_channels=in_channels, out_channels=out_channels, n_plane=n_plane)
        self.upsample = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride)
        self.calls = 0

    def forward(self, triplanes):
        self.calls += 1
        B, Np = triplanes.shape[:2]
        y = self.upsample(triplanes.reshape(B * Np, *triplanes.shape[2:]))
        return y.view(B, Np, *y.shape[1:])


def load_fixture(golden_dir):
    """{tag: SimpleNamespace(dims, module, a, b, pb, cot, out, d_tokens, d_plane_bias)} and the raw npz of
    tests/golden/scene_code_fixture.npz. The module is a frozen scene_code.TriplaneUpsampleNetwork holding the fixture's weights."""
    fx = np.load(os.path.join(golden_dir, "scene_code_fixture.npz"), allow_pickle=False)
    xs, ws, cs = (float(v) for v in fx["scales"])
    cases = {}
    for t in ("a", "b"):
        B, Ci, Co, Np, S = (int(v) for v in fx[f"{t}_dims"])
        m = SC.TriplaneUpsampleNetwork(Ci, Co, Np)
        with torch.no_grad():
            m.upsample.weight.copy_(torch.tensor(fx[f"{t}_weight_q"]).float() * ws)
            m.upsample.bias.copy_(torch.tensor(fx[f"{t}_bias_q"]).float() * ws)
        m.requires_grad_(False)
        cases[t] = SimpleNamespace(
            dims=(B, Ci, Co, Np, S), module=m, a=torch.tensor(fx[f"{t}_tok_a_q"]).float() * xs, b=torch.tensor(fx[f"{t}_tok_b_q"]).float() * xs,
            pb=torch.tensor(fx[f"{t}_plane_bias_q"]).float() * ws, cot=torch.tensor(fx[f"{t}_cot_q"]).float() * cs,
            out=torch.tensor(fx[f"{t}_out"]), d_tokens=torch.tensor(fx[f"{t}_d_tokens"]), d_plane_bias=torch.tensor(fx[f"{t}_d_plane_bias"]))
    return cases, fx


def make_module(dims, seed=0, dev="cpu", cls=None, frozen=True):
    """A module of the given (B, Ci, Co, Np, S) with nn.ConvTranspose2d's own random initialisation under a fixed seed."""
    _, Ci, Co, Np, _ = dims
    torch.manual_seed(100 + seed)
    m = (cls or SC.TriplaneUpsampleNetwork)(Ci, Co, Np).to(dev)
    return m.requires_grad_(not frozen)


def make_inputs(dims, seed=0, dev="cpu", wide=2):
    """(a, b, pb, cot): two token tensors, a (Co, 2S, wide * 2S) plane bias and the cotangent of the joined output, standard normal."""
    B, Ci, Co, Np, S = dims
    g = torch.Generator().manual_seed(1000 * seed + 31 * Ci + 7 * Co + S)
    a, b = torch.randn(B, Ci, Np * S * S, generator=g), torch.randn(B, Ci, Np * S * S, generator=g)
    pb = torch.randn(Co, 2 * S, wide * 2 * S, generator=g)
    cot = torch.randn(B, 1, Co, 2 * S, Np * 2 * S, generator=g)
    return a.to(dev), b.to(dev), pb.to(dev), cot.to(dev)


def to_planes(t, Np):
    """The joined (B, 1, Co, 2S, Np 2S) layout as (B, Np, Co, 2S, 2S)."""
    B, _, Co, H, W = t.shape
    return t.view(B, Co, H, Np, W // Np).permute(0, 3, 1, 2, 4).contiguous()


def run(mode, module, a, b, pb, cot, need_tok=True, need_pb=True, post=None):
    """(out, d_a, d_b, d_pb) of sum(out * cot). mode: 'kernel' (scene_code) | 'torch32' (scene_code_ref) | 'f64' (scene_code_ref
    with acc=float64 on float64 leaves). b and pb may be None; gradients that were not asked for are None. post(mode, scene code)
    is what consumes the scene code, when something does: `out` and `cot` are then its result and that result's cotangent."""
    dt = torch.float64 if mode == "f64" else a.dtype
    leaf = lambda t, need: None if t is None else t.detach().to(dt).requires_grad_(need)      # no copy: a view stays the view it is
    la, lb, lpb = leaf(a, need_tok), leaf(b, need_tok), leaf(pb, need_pb)
    tokens = la if lb is None else (la, lb)
    if mode == "kernel":
        out = SC.scene_code(module, tokens, lpb)
    else:
        out = SC.scene_code_ref(module, tokens, lpb, acc=torch.float64 if mode == "f64" else None)
    if post is not None:
        out = post(mode, out)
    if need_tok or (need_pb and lpb is not None) or any(p.requires_grad for p in module.parameters()):
        (out * cot.to(out.dtype)).sum().backward()
    return out.detach(), la.grad, None if lb is None else lb.grad, None if lpb is None else lpb.grad


def scales(module, a, b, pb, cot, post=None):
    """The largest sum of absolute terms of out, d_tokens and d_plane_bias: the formula run in float64 on |x|, |W|, |b|, |pb| and on
    |W|, |g| (through `post`, whose weights must not be negative, when given)."""
    m = copy.deepcopy(module).requires_grad_(False)
    with torch.no_grad():
        m.upsample.weight.abs_()
        if m.upsample.bias is not None:
            m.upsample.bias.abs_()
    x = a if b is None else a + b
    out, d_tok, _, d_pb = run("f64", m, x.abs(), None, None if pb is None else pb.abs(), cot.abs(), post=post)
    mx = lambda t: 0.0 if t is None or t.numel() == 0 else float(t.max())
    return {"out": mx(out), "d_tokens": mx(d_tok), "d_plane_bias": mx(d_pb)}


def bound(scale):
    """max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 scale."""
    return lambda e: 4 * e + 2.0 ** -20 * scale
