"""Shared by tests/test_res_block_cpu.py and tests/test_gpu_res_block.py: the row-kernel cases of guassianhand_amd.res_block, their
float64 and unfolded float32 yardsticks, and the three-way rule of tests/test_gpu_vert_mlp.py.

A case is a ResNet block over torch.cat([x, m[row_of]], dim=1): x (T,Cin) the per-point half, m (R,H) the per-cell half. The block's
fc_0 and shortcut are (H, Cin + H) parameters whose left windows W[:, :Cin] the kernel reads in place; the tables are
u = W0[:, Cin:] . relu(m) + b0 and s = Ws[:, Cin:] . m + b1. Two table layouts:

    "one"   R = 1, row_of = None (block 0's form: one row for every point)
    "plan"  R = 6 from a 5-cell plan: cell 2 is empty, cell 4 holds point 0 alone, the last point's index is out of range and
            takes row 5, the zero row (T >= 4)

|x| >= 0.05 by construction, and the seeds in ROW_CASES were chosen (on the CPU, `python -m tests.res_block_cases`) so that no
float64 h lies within 2^-16 max|h| of zero: a ReLU that flips for rounding would change a result by far more than the tolerance
allows, and no such flip can be excused as rounding."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from guassianhand_amd import res_block
from guassianhand_amd.pool import PoolPlan

GUARD = 2.0 ** -16
FIELDS = ("out", "dx", "du", "ds")

# (T, H, Cin / H, tables, x as a column window of a wider buffer, seed)
ROW_CASES = (
    (1, 32, 1, "one", False, 0), (31, 32, 2, "one", True, 0), (32, 128, 1, "plan", False, 1), (33, 32, 1, "plan", True, 1),
    (127, 128, 2, "one", False, 2), (128, 32, 2, "plan", False, 0), (129, 128, 1, "plan", True, 64), (257, 32, 1, "one", False, 3),
    (257, 128, 2, "plan", True, 297), (257, 128, 1, "plan", False, 8), (129, 96, 1, "plan", False, 6), (1, 128, 2, "one", False, 0),
)


def case_id(case):
    T, H, k, tables, window, seed = case
    return f"T{T}-H{H}-Cin{k * H}-{tables}{'-window' if window else ''}-s{seed}"


def make_rows(case, device="cpu", w1_scale=1.0):
    """The tensors of one case on `device` (float32): x (a window of a (T, Cin + 7) buffer when asked), m, row_of, plan, the block's
    parameters W0, Ws (H, Cin + H), W1, b0, b1, and the cotangent g."""
    T, H, k, tables, window, seed = case
    Cin = k * H
    gen = torch.Generator().manual_seed(7000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    xv = rn(T, Cin)
    xv = torch.where(xv < 0, xv - 0.05, xv + 0.05)
    if window:
        buf = rn(T, Cin + 7)
        buf[:, 3:3 + Cin] = xv
        x = buf.to(device)[:, 3:3 + Cin]
    else:
        x = xv.to(device)
    if tables == "one":
        m, row_of, plan = rn(1, H), None, None
    else:
        assert T >= 4
        idx = torch.tensor([0, 1, 3])[torch.randint(0, 3, (T,), generator=gen)]
        idx[0], idx[T - 1] = 4, 7
        m = torch.cat([rn(5, H), torch.zeros(1, H)])
        m[2] = 0.0                                                      # the empty cell's pooled row
        plan = PoolPlan(idx.to(device), 5)
        row_of = res_block.row_index(plan)
    sc = (Cin + H) ** -0.5
    c = SimpleNamespace(T=T, H=H, Cin=Cin, x=x, m=m.to(device), row_of=row_of, plan=plan,
                        W0=(sc * rn(H, Cin + H)).to(device), Ws=(sc * rn(H, Cin + H)).to(device),
                        W1=(w1_scale * H ** -0.5 * rn(H, H)).to(device), b0=(0.1 * rn(H)).to(device), b1=(0.1 * rn(H)).to(device),
                        g=rn(T, H).to(device))
    return c


def tables(c, dtype=None):
    """(u, s) of the case, computed in `dtype` (default: the case's own float32)."""
    cv = (lambda t: t.to(dtype)) if dtype is not None else (lambda t: t)
    u = F.linear(torch.relu(cv(c.m)), cv(c.W0)[:, c.Cin:], cv(c.b0))
    s = F.linear(cv(c.m), cv(c.Ws)[:, c.Cin:], cv(c.b1))
    return u, s


def _rows_index(c):
    return torch.zeros(c.T, dtype=torch.long, device=c.x.device) if c.row_of is None else c.row_of.long()


def run_rows(c, mode):
    """out, dx, du, ds of a case. mode: "f64" the restatement in float64; "torch32" the unfolded statements of ResnetBlockFC over
    the materialised concatenation in float32 (du, ds from the gradient of fc_0's output and from g, summed per table row with
    index_add); "fused" / "torch": res_block.res_rows with that ops. The tables are leaves computed in the mode's precision."""
    dt = torch.float64 if mode == "f64" else torch.float32
    x = c.x.detach().to(dt).clone().requires_grad_(True)
    g = c.g.to(dt)
    if mode == "torch32":
        W0, Ws, W1, b0, b1 = c.W0, c.Ws, c.W1, c.b0, c.b1
        cat = torch.cat([x, c.m.index_select(0, _rows_index(c))], dim=1)
        h = F.linear(torch.relu(cat), W0, b0)
        h.retain_grad()
        out = F.linear(cat, Ws) + F.linear(torch.relu(h), W1, b1)
        out.backward(g)
        R = c.m.shape[0]
        du = torch.zeros(R, c.H, device=x.device).index_add_(0, _rows_index(c), h.grad)
        ds = torch.zeros(R, c.H, device=x.device).index_add_(0, _rows_index(c), g)
        return dict(out=out.detach(), dx=x.grad, du=du, ds=ds)
    u, s = (t.detach().requires_grad_(True) for t in tables(c, dt))
    W0, Ws, W1 = c.W0[:, :c.Cin], c.Ws[:, :c.Cin], c.W1
    if mode == "f64":
        out = res_block._res_rows_ref(x, u, s, c.row_of, W0, Ws, W1, acc=torch.float64)
    else:
        out = res_block.res_rows(x, u, s, c.row_of, W0, Ws, W1, ops=mode, plan=c.plan)
    out.backward(g)
    return dict(out=out.detach(), dx=x.grad, du=u.grad, ds=s.grad)


def relu_margin(c):
    """(min|h| / max|h|, min|x| / max|x|) in float64: how far every ReLU argument of the case is from its kink."""
    u, _ = tables(c, torch.float64)
    h = u.index_select(0, _rows_index(c)) + F.linear(torch.relu(c.x.double()), c.W0.double()[:, :c.Cin])
    x = c.x.double()
    return float(h.abs().min() / h.abs().max()), float(x.abs().min() / x.abs().max())


def three_way(kernel, torch32, f64, fields=FIELDS, tag=""):
    """max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64| per field; prints the three errors before asserting."""
    bad = []
    for k in fields:
        ref = f64[k].double()
        e_k, e_t, m = float((kernel[k].double() - ref).abs().max()), float((torch32[k].double() - ref).abs().max()), float(ref.abs().max())
        print(f"{tag} {k}: kernel-f64 {e_k:.3e}  torch32-f64 {e_t:.3e}  max|f64| {m:.3e}")
        if not e_k <= 4 * e_t + 2.0 ** -20 * m:
            bad.append((k, e_k, e_t, m))
    assert not bad, (tag, bad)


def encoder(cfg, seed=0, device="cpu", dtype=torch.float32, **kw):
    """A pool.LocalPoolPointnet with random weights and a non-zero fc_1 in every block (the reference initialises it to zero, which
    would hide the hidden layer)."""
    from guassianhand_amd.pool import LocalPoolPointnet
    torch.manual_seed(seed)
    m = LocalPoolPointnet(cfg, **kw)
    gen = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for b in m.blocks:
            b.fc_1.weight.copy_(torch.randn(b.fc_1.weight.shape, generator=gen) * b.fc_1.weight.shape[1] ** -0.5)
    return m.to(device=device, dtype=dtype)


if __name__ == "__main__":                                   # the seed search: prints, per case, the margins of its seed
    for case in ROW_CASES:
        mh, mx = relu_margin(make_rows(case))
        print(f"{case_id(case)}: min|h|/max|h| = {mh:.3e}, min|x|/max|x| = {mx:.3e} {'ok' if min(mh, mx) > GUARD else 'TOO CLOSE'}")
