"""The cases of tests/test_gpu_gs_trunk.py: random trunks and heads for guassianhand_amd.gs_trunk, and their kink margins.

A case is (P, Cin, H, Cout, shs width, activation, restrict_offset, clip_scaling, seed). P runs over the kernel's tile and tail forms
— R = GH_TRUNK_ROWS = 128 rows per workgroup, 32 per wave — and between them the cases reach every (Cin, H, Cout) of the issue, both
head widths, both activations and both offset forms. The seeds were chosen (on the CPU, `python -m tests.gs_trunk_cases`) so that in
the ReLU cases no float64 hidden pre-activation, and in the clip case no exp(raw scaling) - clip, lies within 2^-16 of the field's
largest magnitude of its kink, with values on both sides: a ReLU or a clamp that flips for rounding would change a result by far
more than the tolerance allows, and no such flip can be excused as rounding. The GPU test asserts the margins again on its own
float64 reference before it compares anything."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

R = 128
GUARD = 2.0 ** -16
FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
OUT = FIELDS + ("grad_x", "grad_pts")

CASES = (
    (1, 131, 128, 128, 3, "silu", True, None, 0), (31, 128, 128, 128, 48, "silu", False, None, 0), (32, 3, 32, 32, 3, "relu", True, None, 0),
    (33, 131, 64, 96, 48, "relu", False, None, 0), (R - 1, 131, 128, 128, 3, "relu", False, None, 1), (R, 131, 128, 128, 48, "silu", True, None, 0),
    (R + 1, 128, 128, 128, 48, "silu", False, 0.005, 1), (2 * R + 1, 131, 128, 128, 3, "silu", True, None, 0),
    (2 * R + 1, 131, 64, 96, 3, "silu", True, None, 0), (2 * R + 1, 3, 32, 32, 48, "relu", False, None, 4),
)


def case_id(case):
    P, Cin, H, Cout, width, act, restrict, clip, seed = case
    return f"P{P}-Cin{Cin}-H{H}-Cout{Cout}-O{11 + width}-{act}-{'restrict' if restrict else 'free'}{'-clip' if clip else ''}-s{seed}"


def make(case, device="cpu"):
    """The tensors of one case on `device` (float32): x, pts, the trunk's six, the head's two, the keywords of gs_trunk and one
    cotangent per output."""
    P, Cin, H, Cout, width, act, restrict, clip, seed = case
    g = torch.Generator().manual_seed(9000 + 131 * seed + P + 7 * Cin + H + width)
    rn = lambda *s: torch.randn(*s, generator=g)
    O = 11 + width
    x, pts = rn(P, Cin), 0.1 * rn(P, 3)
    trunk = [rn(H, Cin) / math.sqrt(Cin), 0.2 * rn(H), rn(H, H) / math.sqrt(H), 0.2 * rn(H), rn(Cout, H) / math.sqrt(H), 0.2 * rn(Cout)]
    Wh, bh = rn(O, Cout) / math.sqrt(Cout), 0.5 * rn(O)
    bh[3:6] = math.log(clip) if clip is not None else bh[3:6] - 5.0
    cot = {k: rn(P, n) for k, n in zip(FIELDS, (3, 3, 4, 1, width))}
    cot["shs"] = cot["shs"].reshape(P, width // 3, 3)
    kw = dict(shs_width=width, use_rgb=width == 3, xyz_offset=True, restrict_offset=restrict, clip_scaling=clip, activation=act)
    to = lambda t: t.to(device)
    return SimpleNamespace(x=to(x), pts=to(pts), trunk=[to(t) for t in trunk], Wh=to(Wh), bh=to(bh), kw=kw, cot={k: to(v) for k, v in cot.items()})


def run(c, mode, used=FIELDS, x=None):
    """One forward + backward -> the five outputs, grad_x and grad_pts. mode: "f64" the restatement in float64, "torch32" it in
    float32 (ops="torch"), "kernel" the HIP path. The weights are frozen; `used` names the outputs that enter the loss."""
    from guassianhand_amd import gs_trunk as T
    xl = (c.x if x is None else x).detach().requires_grad_(True)
    pl = c.pts.detach().clone().requires_grad_(True)
    if mode == "f64":
        gm = T._gs_trunk_ref(xl, pl, c.trunk, c.Wh, c.bh, acc=torch.float64, **c.kw)
    else:
        gm = T.gs_trunk(xl, pl, c.trunk, c.Wh, c.bh, ops="torch" if mode == "torch32" else "fused", **c.kw)
    out = {k: getattr(gm, k).detach() for k in FIELDS}
    sum((getattr(gm, k) * c.cot[k].to(getattr(gm, k).dtype)).sum() for k in used).backward()
    out["grad_x"], out["grad_pts"] = xl.grad, pl.grad if pl.grad is not None else torch.zeros_like(pl)   # (pts enters xyz alone)
    return out


def layers64(c):
    """(v1, v2, y) in float64: the two hidden pre-activations and the trunk's output, as the statements give them."""
    W1, b1, W2, b2, W3, b3 = (t.double() for t in c.trunk)
    act = F.relu if c.kw["activation"] == "relu" else F.silu
    v1 = F.linear(c.x.double(), W1, b1)
    v2 = F.linear(act(v1), W2, b2)
    return v1, v2, F.linear(act(v2), W3, b3)


def margins(c):
    """(ReLU: min over v1, v2 of min|v| / max|v| and whether both signs occur; clip: min|exp(raw) - clip| / max exp(raw) and whether
    both sides occur) in float64; None where the case has no such kink."""
    v1, v2, y = layers64(c)
    relu = clip = None
    if c.kw["activation"] == "relu":
        relu = (min(float(v.abs().min() / v.abs().max()) for v in (v1, v2)), all(bool((v > 0).any() and (v < 0).any()) for v in (v1, v2)))
    if c.kw["clip_scaling"] is not None:
        s = torch.exp(F.linear(y, c.Wh.double()[3:6], c.bh.double()[3:6]))
        t = c.kw["clip_scaling"]
        clip = (float((s - t).abs().min() / s.abs().max()), bool((s > t).any() and (s < t).any()))
    return relu, clip


def assert_margins(c, tag=""):
    for name, m in zip(("relu", "clip"), margins(c)):
        if m is not None:
            print(f"{tag} {name} margin {m[0]:.3e} (guard {GUARD:.3e}), both sides: {m[1]}")
            assert m[0] > GUARD and m[1], (tag, name, m)


if __name__ == "__main__":                                   # the seed search: prints, per case, the margins of its seed
    for case in CASES:
        r, cl = margins(make(case))
        ok = all(m is None or (m[0] > GUARD and m[1]) for m in (r, cl))
        print(f"{case_id(case)}: relu {r}, clip {cl} {'ok' if ok else 'TOO CLOSE'}")
