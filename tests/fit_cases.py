"""Shared by tests/test_fit_edges_cpu.py and tests/test_gpu_fit_edges.py: the edge cases of the one-shot fit step's kernels
(gh_adam_reg_step / _group, gh_reg_total, gh_uv_gather_* / gh_uv_scatter_sorted*, gh_l1_loss, gh_fit_loss), their references written
from the formulas (not from uvmap.py / loss.py), and the three comparison rules the GPU file uses:

    bit equality     wherever two paths perform the same float32 operations in the same order
    three-way rule   max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64| per field, no element excluded (tests/test_gpu_vert_mlp.py)
    sum bound        a float32 sum of n terms lies within n U sum|terms| + U |result| of the exact one, U = 2^-24 (tests/pool_helpers.py)

Every case is drawn on the CPU from a seeded generator, so the CPU file pins the references on the very tensors the GPU file uses.
Inputs are finite throughout. Treat what the cached builders return as read-only."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests.pool_helpers import U, assert_within

I32 = torch.int32
WORST = {}                      # kernel name -> field -> worst err / bound seen so far (printed by report())


def f32(x) -> float:
    """The float32 value of a coefficient, as a Python float: what the C-ABI's `float` arguments hold."""
    return float(np.float32(x))


def _record(kernel, field, ratio):
    w = WORST.setdefault(kernel, {})
    w[field] = max(w.get(field, 0.0), ratio)


def report(kernel):
    print(f"[{kernel}] worst err / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.get(kernel, {}).items())))


def three_way(kernel, torch32, f64, fields, tag="", name=None):
    """max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64| per field; prints the three errors on one line, then asserts."""
    bad, line = [], []
    for k in fields:
        ref = f64[k].double()
        assert kernel[k].shape == ref.shape and kernel[k].dtype == torch.float32, (tag, k, kernel[k].shape, kernel[k].dtype)
        if ref.numel() == 0:
            continue
        e_k, e_t, m = float((kernel[k].double() - ref).abs().max()), float((torch32[k].double() - ref).abs().max()), float(ref.abs().max())
        line.append(f"{k}: kernel-f64 {e_k:.3e} torch32-f64 {e_t:.3e} max|f64| {m:.3e}")
        bound = 4 * e_t + 2.0 ** -20 * m
        if name is not None:
            _record(name, k, e_k / bound if bound > 0 else (0.0 if e_k == 0 else math.inf))
        if not e_k <= bound:
            bad.append((k, e_k, e_t, m))
    print(f"{tag} | " + " | ".join(line))
    assert not bad, (tag, bad)


def sum_within(got, exact, abs_sum, n, what, name=None, field="sum"):
    """The sum bound on a float32 sum of n terms: |got - exact| <= n U sum|terms| + U |exact| (elementwise over small tensors)."""
    exact, abs_sum = torch.as_tensor(exact, dtype=torch.float64).cpu(), torch.as_tensor(abs_sum, dtype=torch.float64).cpu()
    bound = n * U * abs_sum + U * exact.abs()
    got = got.detach().double().cpu().reshape(exact.shape)
    if name is not None:
        err = (got - exact).abs()
        _record(name, field, float((err / bound.clamp(min=1e-300)).max()) if float(err.max()) > 0 else 0.0)
    assert_within(got, exact, bound, what)


def bits(t):
    return t.contiguous().view(I32)


def misaligned(t):
    """A contiguous copy of t that starts 4 bytes past a 16-byte boundary: a view into a buffer one element longer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (t.numel() == 0 or v.data_ptr() % 16 == 4)
    return v


# ---- Adam with the regulariser folded in ---------------------------------------------------------------------------------------------
ADAM_N = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 1_048_581)   # the last: a second grid-stride trip of the float4 loop at 1024 blocks
ADAM_T = (1, 2, 1000, 20000)
ADAM_REG = ((0.0, 0.0), (3e-4, 0.0), (0.0, 2e-3), (3e-4, 2e-3))
ADAM_ALIGN = ("aligned", "param+4", "grad+4")
ADAM_LR, ADAM_BETAS, ADAM_EPS = 0.01, (0.9, 0.999), 1e-8
_ADAM_CACHE = {}


def adam_state(n):
    """(p, g, m, v) float32 on the CPU for n elements; m and v are the moments of a state with t > 1 (a first step starts from zeros).
    Populations: i % 7 == 3: p = +0.0, i % 7 == 5: p = -0.0, both with g = m = v = 0 (such an element must stay exactly as it is);
    i % 7 == 6: g exactly 0 on an ordinary parameter; elsewhere |g| >= 1e-6. v = m^2 (1 + rand) keeps the step bounded."""
    if n not in _ADAM_CACHE:
        gen = torch.Generator().manual_seed(5000 + n)
        i = torch.arange(n)
        p = 0.1 * torch.randn(n, generator=gen)
        g = 0.01 * torch.randn(n, generator=gen)
        g = torch.where(g.abs() < 1e-6, torch.full_like(g, 1e-6), g)
        m = 0.01 * torch.randn(n, generator=gen)
        v = m * m * (1.0 + torch.rand(n, generator=gen))
        pz, nz = i % 7 == 3, i % 7 == 5
        p[pz], p[nz] = 0.0, -0.0
        zero = pz | nz
        g[zero | (i % 7 == 6)] = 0.0
        m[zero], v[zero] = 0.0, 0.0
        _ADAM_CACHE[n] = SimpleNamespace(p=p, g=g, m=m, v=v, zero=zero)
    return _ADAM_CACHE[n]


def adam_ref(p, g, m, v, t, lr, betas, eps, l1, l2, dtype, coeffs="float32"):
    """One Adam step with the gradient of l1 sum|p| + l2 sum p^2 folded in, from the formulas, in `dtype`:
         gv = g + l1 sign(p) + 2 l2 p;  m' = b1 m + (1 - b1) gv;  v' = b2 v + (1 - b2) gv^2
         p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    and (sum|p|, sum p^2) of the pre-update values. coeffs="float32": the contract of the entry point is Adam with the coefficients
    as it receives them, so lr, betas, eps, l1, l2 are taken at their float32 values and 1 - b is formed from those (exact in
    both precisions: b >= 0.5). coeffs="decimal": the Python doubles, which is what torch.optim.Adam multiplies by. The bias
    corrections are Python doubles either way, as in torch.optim.Adam and in the kernel."""
    c = f32 if coeffs == "float32" else float
    lr, b1, b2, eps, l1, l2 = c(lr), c(betas[0]), c(betas[1]), c(eps), c(l1), c(l2)
    P, G, M, V = (x.detach().to(dtype) for x in (p, g, m, v))
    gv = G + l1 * torch.sign(P) + (2.0 * l2) * P
    m1 = b1 * M + (1.0 - b1) * gv
    v1 = b2 * V + (1.0 - b2) * (gv * gv)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p1 = P - (lr / bc1) * (m1 / (v1.sqrt() / math.sqrt(bc2) + eps))
    return dict(param=p1, exp_avg=m1, exp_avg_sq=v1, sums=torch.stack([P.abs().sum(), (P * P).sum()]))


# ---- bilinear gather over the active texels and its transpose ------------------------------------------------------------------------
# (P, Hm, Wm, C of the single-map kernels, (Ca, Cb) of the two-map kernels, UVs). Not the product of the axes: every P of
# 0, 1, 63, 64, 65, 257, 4099, every C of 1, 3, 48, 65, every pair of (48, 1), (1, 48), (3, 1), (65, 2) and every map of 1 x 1, 2 x 3,
# 64 x 128, 1024 x 2048 (the reference's own; only U <= 4P texels exist there) appears, the fit's (48, 1) at the reference's map size among
# them. "edge": test_plane_cpu.edge_uvs, uniform in +-1.1 with rows at exactly +-1; "one_uv": all 4096 points at one UV; "outside":
# every corner of every UV outside the map (U == 0).
GATHER_CASES = (
    (0, 2, 3, 3, (3, 1), "edge"),
    (0, 1024, 2048, 48, (48, 1), "edge"),
    (1, 1, 1, 1, (1, 48), "edge"),
    (1, 1024, 2048, 48, (48, 1), "edge"),
    (63, 2, 3, 65, (65, 2), "edge"),
    (64, 64, 128, 1, (1, 48), "edge"),
    (65, 1, 1, 48, (48, 1), "edge"),
    (257, 2, 3, 3, (3, 1), "edge"),
    (257, 64, 128, 48, (48, 1), "edge"),
    (4099, 64, 128, 65, (65, 2), "edge"),
    (4099, 1024, 2048, 48, (48, 1), "edge"),
    (4099, 1024, 2048, 3, (3, 1), "edge"),
    (4096, 2, 3, 1, (1, 48), "one_uv"),
    (4096, 64, 128, 48, (48, 1), "one_uv"),
    (4096, 1024, 2048, 3, (3, 1), "one_uv"),
    (65, 2, 3, 3, (3, 1), "outside"),
    (257, 64, 128, 48, (48, 1), "outside"),
    (4099, 1024, 2048, 65, (65, 2), "outside"),
)
ONE_UV = (0.3137, -0.4219)


def gather_id(case):
    P, Hm, Wm, C, (Ca, Cb), kind = case
    return f"P{P}-{Hm}x{Wm}-C{C}-{Ca}+{Cb}-{kind}"


def gather_uvs(case):
    """uv (P,2) float32 on the CPU."""
    P, Hm, Wm, _C, _pair, kind = case
    if kind == "edge":
        from tests.test_plane_cpu import edge_uvs
        return edge_uvs(P, seed=P + Hm)
    if kind == "one_uv":
        return torch.tensor(ONE_UV).repeat(P, 1)
    # outside: ix = (u + 1) / 2 * (Wm - 1) must be < -1 or >= Wm, i.e. |u| > 1 + 2 Wm / (Wm - 1) at the most 5 for Wm = 2; a map one
    # texel wide or high has no outside (ix is 0 whatever u is), so these cases use maps of at least 2 x 2
    assert Hm > 1 and Wm > 1
    gen = torch.Generator().manual_seed(6000 + P)
    mag = 5.5 + torch.rand(P, 2, generator=gen)
    return mag * (torch.randint(0, 2, (P, 2), generator=gen).float() * 2 - 1)


def gather_tensors(case, U_):
    """Texels (U,C), (U,Ca), (U,Cb) and cotangents (P,C), (P,Ca), (P,Cb), float32 on the CPU, for an index of U_ active texels."""
    P, Hm, Wm, C, (Ca, Cb), _kind = case
    gen = torch.Generator().manual_seed(7000 + P + Hm + C)
    r = lambda *s: torch.randn(*s, generator=gen)
    return SimpleNamespace(tex=r(U_, C), tex_a=r(U_, Ca), tex_b=r(U_, Cb), dout=r(P, C), dout_a=r(P, Ca), dout_b=r(P, Cb))


def gather_ref(tex, at, uv, dout, dtype):
    """F.grid_sample(bilinear, align_corners=True, zeros padding) in `dtype` on the dense map at.dense(tex), and its autograd gradient
    for the cotangent dout, compacted: dict(out (P,C), grad (U,C)). tex, uv, dout: float32, on one device."""
    P, Cc = uv.shape[0], tex.shape[1]
    if P == 0:                                                     # grid_sample has nothing to sample: the shapes alone
        return dict(out=torch.zeros(0, Cc, dtype=dtype, device=tex.device), grad=torch.zeros(at.U, Cc, dtype=dtype, device=tex.device))
    dense = at.dense(tex.to(dtype)).requires_grad_(True)
    out = F.grid_sample(dense.permute(2, 0, 1)[None], uv.to(dtype)[None, :, None, :], mode="bilinear", padding_mode="zeros",
                        align_corners=True)[0, :, :, 0].transpose(0, 1)
    (out * dout.to(dtype)).sum().backward()
    return dict(out=out.detach(), grad=at.compact(dense.grad))


def loop_gather(dense, uv, dout):
    """The same lookup as a per-point loop over the four corners in numpy float64, sharing nothing with torch's grid_sample:
    (out (P,C), gradient w.r.t. the dense map (Hm,Wm,C), the same gradient accumulated over |dout| for the bound)."""
    dense, uv, dout = (np.asarray(x, dtype=np.float64) for x in (dense, uv, dout))
    Hm, Wm, Cc = dense.shape
    out, grad, agrad = np.zeros((uv.shape[0], Cc)), np.zeros_like(dense), np.zeros_like(dense)
    for i in range(uv.shape[0]):
        ix, iy = (uv[i, 0] + 1.0) / 2.0 * (Wm - 1), (uv[i, 1] + 1.0) / 2.0 * (Hm - 1)
        x0, y0 = int(np.floor(ix)), int(np.floor(iy))
        for dy, wy in ((0, 1.0 - (iy - y0)), (1, iy - y0)):
            for dx, wx in ((0, 1.0 - (ix - x0)), (1, ix - x0)):
                x, y = x0 + dx, y0 + dy
                if 0 <= x < Wm and 0 <= y < Hm:
                    out[i] += dense[y, x] * (wx * wy)
                    grad[y, x] += dout[i] * (wx * wy)
                    agrad[y, x] += np.abs(dout[i]) * (wx * wy)
    return out, grad, agrad


# ---- gh_l1_loss ----------------------------------------------------------------------------------------------------------------------
L1_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1_048_583)
L1_ALIGN = ("aligned", "image+4", "target+4", "both+4")
_L1_CACHE = {}


def l1_case(n):
    """(image, target) float32 (n,) on the CPU. Every seventh element is an exact tie; of those, i % 21 == 0 is +0.0 against -0.0 and
    i % 21 == 7 is -0.0 against +0.0."""
    if n not in _L1_CACHE:
        gen = torch.Generator().manual_seed(8000 + n)
        a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        i = torch.arange(n)
        a[::7] = b[::7]
        a[i % 21 == 0], b[i % 21 == 0] = 0.0, -0.0
        a[i % 21 == 7], b[i % 21 == 7] = -0.0, 0.0
        _L1_CACHE[n] = (a, b)
    return _L1_CACHE[n]


def l1_ref(a, b):
    """The float64 mean of |a - b|, and the gradient to the bit: sign(a - b) * float32(1.0 / n) with sign(0) = +0."""
    d = a.detach().double() - b.detach().double()
    n = d.numel()
    s = torch.full((), 1.0 / n, dtype=torch.float64).to(torch.float32).to(d.device)
    grad = torch.where(d > 0, s, torch.where(d < 0, -s, torch.zeros_like(s))).reshape(a.shape)
    return d.abs().mean(), grad


# ---- gh_fit_loss ---------------------------------------------------------------------------------------------------------------------
FIT_SHAPES = ((1, 1, 1), (1, 1, 3), (2, 16, 16), (5, 7, 9), (257, 256, 256))     # the last: 16 842 752 pixels > 2^24, the 64-bit division
LO, HI = np.float32(-0.001), np.float32(1.0)
# alpha exactly at either clip bound and one float32 step to either side; the bounds are float32 values (float32(-0.001) =
# -0.0010000000475 lies BELOW the double -0.001): torch.clamp on a float32 tensor and the kernel both compare against those
SPECIAL = np.array([LO, np.nextafter(LO, np.float32(-2)), np.nextafter(LO, np.float32(2)),
                    HI, np.nextafter(HI, np.float32(2)), np.nextafter(HI, np.float32(-2))], dtype=np.float32)
SPECIAL_PASSES = (True, False, True, True, False, True)          # does dL/dalpha pass the clip there?


def fit_case(NV, H, W, bbox):
    """image (NV,3,H,W) in [0,1], alpha (NV,H,W) in [-0.1, 1.2], gt_rgb (NV,H,W,3), gt_mask (NV,H,W) 0/1, bbox (NV,H,W) 0/1 or None,
    float32 on the CPU, plus `special` (flat pixel indices) and `which` (their index into SPECIAL): up to six pixels when there are
    no more, else every fifth pixel holds a SPECIAL alpha in turn, with the mask on the far side (1 at the lower bound, 0 at the
    upper), so that a gradient which passes the clip is not zero. Every eleventh image element ties its target."""
    gen = torch.Generator().manual_seed(9000 + NV * H * W)
    npix = NV * H * W
    image = torch.rand(NV, 3, H, W, generator=gen)
    alpha = torch.rand(NV, H, W, generator=gen) * 1.3 - 0.1
    gt_rgb = torch.rand(NV, H, W, 3, generator=gen)
    gt_mask = (torch.rand(NV, H, W, generator=gen) > 0.5).float()
    bb = (torch.rand(NV, H, W, generator=gen) > 0.3).float() if bbox else None
    image.view(-1)[::11] = gt_rgb.permute(0, 3, 1, 2).reshape(-1)[::11]
    step = 1 if npix <= 6 else 5
    special = torch.arange(0, npix, step)
    which = (special // step) % 6
    alpha.view(-1)[special] = torch.from_numpy(SPECIAL)[which]
    gt_mask.view(-1)[special] = (which < 3).float()
    return SimpleNamespace(image=image, alpha=alpha, gt_rgb=gt_rgb, gt_mask=gt_mask, bbox=bb, special=special, which=which)


def fit_ref(c, scale, upstream, dtype, device="cpu"):
    """fit.fit_loss in `dtype` on the case's tensors: dict(loss, dimage, dalpha) of upstream * scale * fit_loss. The mask arrives with
    ONE channel, so fit_loss's `.float().mean(-1)` hands alpha on unchanged and its clip compares float32 against float32 bounds in
    either precision; everything behind the clip, and all of the colour term, runs in `dtype`. The reference's own error: in float64
    the loss and dimage are float64 throughout, but autograd casts dalpha to float32 where it re-enters the float32 clip, so dalpha
    carries ONE float32 rounding (2^-24 relative) — a sixteenth of the 2^-20 max|f64| the three-way rule allows."""
    from guassianhand_amd import fit
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)
    im, al = to(c.image).requires_grad_(True), to(c.alpha).requires_grad_(True)
    loss = fit.fit_loss(im.permute(0, 2, 3, 1), al.unsqueeze(-1), to(c.gt_rgb), to(c.gt_mask), to(c.bbox)) * f32(scale)
    (upstream * loss).backward()
    return dict(loss=loss.detach().reshape(1), dimage=im.grad, dalpha=al.grad)
