"""The one-shot fit step's kernels (csrc/gh_uv.hip, csrc/gh_loss.hip through uvmap.py and loss.py) at their edge shapes, against the
float64 references of tests/fit_cases.py computed on the device. Three rules only (fit_cases' docstring): bit equality, the
three-way rule, the sum bound. tests/test_fit_edges_cpu.py pins the references and the case generators on the CPU."""
import ctypes as C
import itertools

import pytest
import torch

from tests import fit_cases as fc

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def guards(dev):
    """(clear, set): device GhCounters whose overflow word is 0 / 1, as tests/test_gpu_fit.py builds them."""
    return torch.zeros(4, dtype=torch.int32, device=dev), torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)


# ---- gh_adam_reg_step ------------------------------------------------------------------------------------------------------------------
def make_adam(s, t, l1, l2, align):
    """An AdamReg over the device state s at device step count t - 1, and the `grad=` argument of its step (None: its own buffer)."""
    from guassianhand_amd.uvmap import AdamReg
    param = fc.misaligned(s.p) if align == "param+4" else s.p.clone()
    a = AdamReg(param, fc.ADAM_LR, fc.ADAM_BETAS, fc.ADAM_EPS, reg_l1=l1, reg_l2=l2)
    if t > 1:
        a.exp_avg.copy_(s.m); a.exp_avg_sq.copy_(s.v)
    a.step_state[0] = t - 1
    a.t = t - 1
    ext = None
    if align == "grad+4":
        ext = fc.misaligned(s.g)
    else:
        a.grad.copy_(s.g)
    wide = all(x.data_ptr() % 16 == 0 for x in (a.param, a.grad if ext is None else ext, a.exp_avg, a.exp_avg_sq))
    assert wide == (align == "aligned")              # the kernel takes its float4 loop exactly when all four arrays are aligned
    return a, ext


@pytest.mark.parametrize("n", fc.ADAM_N)
def test_adam_single_steps(dev, n):
    """Every t, regulariser and alignment at n elements: one step from a given state (never a trajectory: with the l1 term a parameter
    that crosses zero takes another sign in float32 than in float64, which measures the inputs). param / exp_avg / exp_avg_sq under the
    three-way rule, torch32 being the same statements in float32 torch; grad zeroed; the block partials' sums under the sum bound;
    the device step count. The distance from float64 Adam with the DECIMAL betas (torch.optim.Adam's) is printed, not asserted."""
    cpu = fc.adam_state(n)
    s = fc.SimpleNamespace(**{k: getattr(cpu, k).to(dev) for k in ("p", "g", "m", "v", "zero")})
    zeros = torch.zeros_like(s.p)
    hyper = (fc.ADAM_LR, fc.ADAM_BETAS, fc.ADAM_EPS)
    fields = ("param", "exp_avg", "exp_avg_sq")
    dec = {k: 0.0 for k in fields}
    tdec = {k: 0.0 for k in fields}
    for t, (l1, l2), align in itertools.product(fc.ADAM_T, fc.ADAM_REG, fc.ADAM_ALIGN):
        m, v = (s.m, s.v) if t > 1 else (zeros, zeros)
        f64 = fc.adam_ref(s.p, s.g, m, v, t, *hyper, l1, l2, F64)
        t32 = fc.adam_ref(s.p, s.g, m, v, t, *hyper, l1, l2, F32)
        a, ext = make_adam(s, t, l1, l2, align)
        sums = a.step(None, grad=ext)
        ker = dict(param=a.param, exp_avg=a.exp_avg, exp_avg_sq=a.exp_avg_sq)
        tag = f"adam n={n} t={t} l1={l1} l2={l2} {align}"
        fc.three_way(ker, t32, f64, fields, tag=tag, name="gh_adam_reg_step")
        assert float((a.grad if ext is None else ext).abs().max()) == 0.0, tag
        fc.sum_within(sums, f64["sums"], f64["sums"], n, tag + " sums", name="gh_adam_reg_step")
        assert a.step_state.tolist() == [t, 0], tag
        # an exactly zero parameter with a zero gradient stays what it is, sign included, and its moments stay 0
        assert torch.equal(fc.bits(a.param)[s.zero], fc.bits(s.p)[s.zero]), tag
        assert float(a.exp_avg[s.zero].abs().sum()) == 0.0 and float(a.exp_avg_sq[s.zero].abs().sum()) == 0.0, tag
        d64 = fc.adam_ref(s.p, s.g, m, v, t, *hyper, l1, l2, F64, coeffs="decimal")
        d32 = fc.adam_ref(s.p, s.g, m, v, t, *hyper, l1, l2, F32, coeffs="decimal")
        for k in fields:
            dec[k] = max(dec[k], float((ker[k].double() - d64[k]).abs().max()))
            tdec[k] = max(tdec[k], float((d32[k].double() - d64[k]).abs().max()))
    print(f"adam n={n}: max distance from float64 Adam with decimal betas, over every t / regulariser / alignment: kernel " +
          ", ".join(f"{k} {dec[k]:.3e}" for k in fields) + " | float32 torch statements with decimal betas " +
          ", ".join(f"{k} {tdec[k]:.3e}" for k in fields) + f" | max|v| {float(s.v.max()):.3e}")
    fc.report("gh_adam_reg_step")


@pytest.mark.parametrize("n", fc.ADAM_N)
def test_adam_guarded_step_is_a_no_op_that_still_sums(dev, n):
    """With the overflow word set: param and both moments bitwise unchanged, grad zeroed, the partials hold the sums, and the step is
    not counted — on the float4 path and on both scalar paths."""
    cpu = fc.adam_state(n)
    s = fc.SimpleNamespace(**{k: getattr(cpu, k).to(dev) for k in ("p", "g", "m", "v", "zero")})
    _, bad = guards(dev)
    for t, align in itertools.product((1, 1000), fc.ADAM_ALIGN):
        a, ext = make_adam(s, t, 3e-4, 2e-3, align)
        before = [fc.bits(x).clone() for x in (a.param, a.exp_avg, a.exp_avg_sq)]
        sums = a.step(bad, grad=ext)
        tag = f"adam guarded n={n} t={t} {align}"
        for x, b in zip((a.param, a.exp_avg, a.exp_avg_sq), before):
            assert torch.equal(fc.bits(x), b), tag
        assert float((a.grad if ext is None else ext).abs().max()) == 0.0, tag
        want = torch.stack([s.p.double().abs().sum(), (s.p.double() ** 2).sum()])
        fc.sum_within(sums, want, want, n, tag + " sums", name="gh_adam_reg_step (guarded)")
        assert a.step_state.tolist() == [t - 1, 0], tag
    fc.report("gh_adam_reg_step (guarded)")


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("sizes", [(0, 5, 1025), (1025, 0, 257, 5), (5,), (0,), (1_048_581, 0, 3)])
def test_adam_group_is_bitwise_the_single_calls(dev, sizes, guarded):
    """gh_adam_reg_step_group on tensors of different sizes, an empty one among them, one misaligned and one with a caller-supplied
    misaligned gradient: every array, the partials and the step counts equal those of the single calls on the same states."""
    from guassianhand_amd.uvmap import AdamReg, adam_group_step
    guard = guards(dev)[1 if guarded else 0]
    t = 1000
    aligns = ("aligned", "param+4", "grad+4", "aligned")

    def build():
        out = []
        for i, n in enumerate(sizes):
            cpu = fc.adam_state(n)
            s = fc.SimpleNamespace(**{k: getattr(cpu, k).to(dev) for k in ("p", "g", "m", "v")})
            if n == 0:
                a = AdamReg(s.p.clone(), fc.ADAM_LR, fc.ADAM_BETAS, fc.ADAM_EPS, reg_l1=3e-4)
                a.t, ext = t - 1, None
                a.step_state[0] = t - 1
            else:
                a, ext = make_adam(s, t, 3e-4 * (i % 2), 2e-3 * (i % 3 != 0), aligns[i])
            out.append((a, ext))
        return out

    one, grp = build(), build()
    for a, ext in one:
        a.step(guard, grad=ext, sums=False)
    adam_group_step([a for a, _ in grp], guard, [ext for _, ext in grp])
    for (a, ea), (b, eb), n in zip(one, grp, sizes):
        for x, y in ((a.param, b.param), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.partials, b.partials), (a.grad, b.grad)):
            assert torch.equal(fc.bits(x), fc.bits(y)), (sizes, n)
        if ea is not None:
            assert torch.equal(fc.bits(ea), fc.bits(eb)) and float(eb.abs().max()) == 0.0
        assert a.step_state.tolist() == b.step_state.tolist() == ([t - 1, 0] if (guarded or n == 0) else [t, 0]), (sizes, n)
        if n and not guarded:
            assert not torch.equal(b.param, fc.adam_state(n).p.to(dev))            # (the step did move the parameters)


# ---- gh_reg_total ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a,n_b", [(1, 1), (255, 1024), (256, 257), (257, 255), (1024, 256), (1, 1024)])
def test_reg_total_sums_hand_filled_partials(dev, n_a, n_b):
    """out[1] = k_a sum_i pa[i, col_a] + k_b sum_i pb[i, col_b] and out[0] = base + out[1], both columns of both arrays, base absent
    and present. The sum bound: out[1] is a float32 sum of the n_a + n_b terms k * p — n_a - 1 and n_b - 1 additions, the two
    scalings and the addition of the halves are n_a + n_b + 1 roundings, the last relative to the result — and out[0] is one term
    (base) and one rounding more. The columns hold values of different signs and sizes, so that a wrong column shows."""
    from guassianhand_amd.uvmap import AdamReg, reg_total
    gen = torch.Generator().manual_seed(n_a * 4099 + n_b)
    mk = lambda n: AdamReg(torch.zeros(256 * n, device=dev), 0.01)
    a, b = mk(n_a), mk(n_b)
    assert (a.n_partials, b.n_partials) == (n_a, n_b)
    a.partials.copy_((torch.randn(n_a, 2, generator=gen) * torch.tensor([1.0, 30.0])).to(dev))
    b.partials.copy_((torch.randn(n_b, 2, generator=gen) * torch.tensor([-7.0, 0.2]) + torch.tensor([2.0, -1.0])).to(dev))
    k_a, k_b = fc.f32(0.993), fc.f32(0.3)                                              # float32 values: what the entry point receives
    for col_a, col_b, base in itertools.product((0, 1), (0, 1), (None, torch.tensor(3.25, device=dev))):
        out = reg_total(a, col_a, k_a, b, col_b, k_b, base)
        ta, tb = k_a * a.partials[:, col_a].double(), k_b * b.partials[:, col_b].double()
        reg, areg = ta.sum() + tb.sum(), ta.abs().sum() + tb.abs().sum()
        b0 = 0.0 if base is None else float(base)
        tag = f"reg_total n=({n_a},{n_b}) cols=({col_a},{col_b}) base={'yes' if base is not None else 'no'}"
        fc.sum_within(out[1], reg, areg, n_a + n_b, tag + " reg", name="gh_reg_total", field="reg")
        fc.sum_within(out[0], reg + b0, areg + abs(b0), n_a + n_b + 1, tag + " total", name="gh_reg_total", field="total")
    fc.report("gh_reg_total")


# ---- gh_uv_gather_forward / _forward2 / gh_uv_scatter_sorted / _sorted2 / gh_uv_gather_backward ---------------------------------------
def atomic_scatter(at, dout, C_):
    """The C-ABI's atomic transpose (kept for callers without a texel list), into zeros."""
    from guassianhand_amd import _lib
    out = torch.zeros(at.U, C_, dtype=F32, device=dout.device)
    rc = _lib.lib().gh_uv_gather_backward(C.c_void_p(at.slot.data_ptr()), C.c_void_p(at.w.data_ptr()), C.c_void_p(dout.data_ptr()),
                                          C.c_void_p(out.data_ptr()), at.P, C_, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return out


@pytest.mark.parametrize("case", fc.GATHER_CASES, ids=fc.gather_id)
def test_gather_and_scatter(dev, case):
    from guassianhand_amd.uvmap import ActiveTexels, uv_gather, uv_gather2, uv_gather_backward, uv_gather_backward2, uv_sample
    P, Hm, Wm, C_, (Ca, Cb), kind = case
    uv = fc.gather_uvs(case).to(dev)
    at = ActiveTexels(uv, Hm, Wm)
    cpu_at = ActiveTexels(uv.cpu(), Hm, Wm)
    assert at.U == cpu_at.U and torch.equal(at.slot.cpu(), cpu_at.slot) and at.U <= 4 * P and (kind != "outside" or at.U == 0)
    t = fc.gather_tensors(case, at.U)
    t = fc.SimpleNamespace(**{k: v.to(dev) for k, v in vars(t).items()})
    tag = fc.gather_id(case)

    def scatter(dout, C__):
        g = torch.zeros(at.U, C__, device=dev)
        uv_gather_backward(dout, at, g)
        return g

    # one map: the compacted gather is the dense lookup, bit for bit; outputs and gradients against float64 grid_sample
    out = uv_gather(t.tex, at)
    dense = at.dense(t.tex)
    assert torch.equal(at.compact(dense), t.tex)
    assert out.shape == (P, C_) and torch.equal(fc.bits(uv_gather(at.compact(dense), at)), fc.bits(uv_sample(dense, uv))), tag
    del dense
    g = scatter(t.dout, C_)
    assert torch.equal(fc.bits(scatter(t.dout, C_)), fc.bits(g)), tag                   # the sorted scatter repeats itself
    twice = g.clone()
    uv_gather_backward(t.dout, at, twice)                                              # ... and ACCUMULATES into what it is given
    assert torch.equal(twice, g + g), tag
    f64, t32 = fc.gather_ref(t.tex, at, uv, t.dout, F64), fc.gather_ref(t.tex, at, uv, t.dout, F32)
    fc.three_way(dict(out=out, grad=g), t32, f64, ("out", "grad"), tag=f"gather {tag}", name="gh_uv_gather_forward / gh_uv_scatter_sorted")
    if P > 0 and at.U > 0:
        fc.three_way(dict(grad=atomic_scatter(at, t.dout, C_)), t32, f64, ("grad",), tag=f"atomic scatter {tag}", name="gh_uv_gather_backward")
    del f64, t32

    # two maps in one launch: bitwise the single-map kernels; and held to float64 themselves
    oa, ob = uv_gather2(t.tex_a, t.tex_b, at)
    assert oa.shape == (P, Ca) and ob.shape == (P, Cb)
    assert torch.equal(fc.bits(oa), fc.bits(uv_gather(t.tex_a, at))) and torch.equal(fc.bits(ob), fc.bits(uv_gather(t.tex_b, at))), tag
    ga, gb = torch.zeros(at.U, Ca, device=dev), torch.zeros(at.U, Cb, device=dev)
    uv_gather_backward2(t.dout_a, t.dout_b, at, ga, gb)
    assert torch.equal(fc.bits(ga), fc.bits(scatter(t.dout_a, Ca))) and torch.equal(fc.bits(gb), fc.bits(scatter(t.dout_b, Cb))), tag
    ga2, gb2 = torch.zeros_like(ga), torch.zeros_like(gb)
    uv_gather_backward2(t.dout_a, t.dout_b, at, ga2, gb2)
    assert torch.equal(fc.bits(ga2), fc.bits(ga)) and torch.equal(fc.bits(gb2), fc.bits(gb)), tag
    for name, tex, dout, o, gg in (("a", t.tex_a, t.dout_a, oa, ga), ("b", t.tex_b, t.dout_b, ob, gb)):
        f64, t32 = fc.gather_ref(tex, at, uv, dout, F64), fc.gather_ref(tex, at, uv, dout, F32)
        fc.three_way(dict(out=o, grad=gg), t32, f64, ("out", "grad"), tag=f"gather2 map {name} {tag}",
                     name="gh_uv_gather_forward2 / gh_uv_scatter_sorted2")
        del f64, t32

    if P == 0 or at.U == 0:
        # nothing to look up / nothing inside the map: right shapes, zeros, no error; a gradient buffer keeps what it held
        assert float(out.abs().sum()) == 0.0 and float(oa.abs().sum()) == 0.0 and float(ob.abs().sum()) == 0.0
        assert g.shape == (at.U, C_) and float(g.abs().sum()) == 0.0 and float(ga.abs().sum()) == 0.0 and float(gb.abs().sum()) == 0.0
    if P == 0 and at.U == 0:
        m = torch.randn(Hm, Wm, 3, device=dev).requires_grad_(True) if Hm * Wm <= 64 * 128 else None
        if m is not None:
            uv_sample(m, uv).sum().backward()
            assert m.grad.shape == m.shape and float(m.grad.abs().sum()) == 0.0
    if kind == "outside" and Hm * Wm <= 64 * 128:                                        # the dense lookup's autograd path, same case
        m = torch.randn(Hm, Wm, 3, device=dev).requires_grad_(True)
        o = uv_sample(m, uv)
        o.sum().backward()
        assert float(o.detach().abs().sum()) == 0.0 and float(m.grad.abs().sum()) == 0.0
    fc.report("gh_uv_gather_forward / gh_uv_scatter_sorted")
    fc.report("gh_uv_gather_forward2 / gh_uv_scatter_sorted2")
    fc.report("gh_uv_gather_backward")


# ---- gh_l1_loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fc.L1_N)
def test_l1_loss(dev, n):
    """The gradient to the bit (sign(a - b) float32(1 / n), +0 at ties, +0.0 against -0.0 among them) and the loss under the sum bound
    (n terms |a - b|, scaled by 1 / n), with image and target aligned and, separately and together, as contiguous views that start 4
    bytes past a 16-byte boundary; an upstream factor through l1_mean_loss; NaN and a zero gradient under the guard."""
    from guassianhand_amd.loss import _l1_kernel, l1_mean_loss
    a, b = (x.to(dev) for x in fc.l1_case(n))
    want_loss, want_grad = fc.l1_ref(a, b)
    for align in fc.L1_ALIGN:
        ia = fc.misaligned(a) if align in ("image+4", "both+4") else a
        ib = fc.misaligned(b) if align in ("target+4", "both+4") else b
        assert (ia.data_ptr() % 16, ib.data_ptr() % 16) == (4 * (ia is not a), 4 * (ib is not b))
        tag = f"l1 n={n} {align}"
        loss, grad = _l1_kernel(ia, ib)
        assert torch.equal(fc.bits(grad), fc.bits(want_grad)), tag
        fc.sum_within(loss, want_loss, want_loss, n, tag + " loss", name="gh_l1_loss", field="loss")
        x = ia.detach().requires_grad_(True)              # (detach keeps the storage offset: still misaligned)
        la = l1_mean_loss(x, ib)
        (2.5 * la).backward()
        assert torch.equal(fc.bits(la.detach()), fc.bits(loss)) and torch.equal(fc.bits(x.grad), fc.bits(want_grad * 2.5)), tag
        loss, grad = _l1_kernel(ia, ib, guards(dev)[1])
        assert bool(torch.isnan(loss)) and float(grad.abs().max()) == 0.0, tag
        loss, grad = _l1_kernel(ia, ib, guards(dev)[0])
        assert torch.equal(fc.bits(grad), fc.bits(want_grad)) and torch.equal(fc.bits(loss), fc.bits(la.detach())), tag
    fc.report("gh_l1_loss")


def test_l1_loss_of_a_slice_of_a_batch(dev):
    """The shape the defect was found at: torch.rand(3, 3, 7, 5)[1:] is contiguous and starts 4 bytes past a 16-byte boundary."""
    from guassianhand_amd.loss import l1_mean_loss
    gen = torch.Generator().manual_seed(2)
    img, gt = torch.rand(3, 3, 7, 5, generator=gen).to(dev), torch.rand(3, 3, 7, 5, generator=gen).to(dev)
    a, b = img[1:], gt[1:]
    assert a.is_contiguous() and a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4
    loss = l1_mean_loss(a, b)
    want, _ = fc.l1_ref(a, b)
    fc.sum_within(loss, want, want, a.numel(), "l1 of img[1:]", name="gh_l1_loss", field="loss")


# ---- gh_fit_loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bbox", [False, True])
@pytest.mark.parametrize("NV,H,W", fc.FIT_SHAPES)
def test_fit_loss(dev, NV, H, W, bbox):
    """Loss, dL/dimage and dL/dalpha of fit_image_loss under the three-way rule, fit.fit_loss in float32 on the device being the
    yardstick; at the alphas on and one float32 step either side of the clip bounds the kernel passes the gradient exactly where the
    float64 reference does; under the guard the loss is NaN and no gradient leaves."""
    from guassianhand_amd.loss import fit_image_loss
    c = fc.fit_case(NV, H, W, bbox)
    c = fc.SimpleNamespace(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in vars(c).items()})
    scale, upstream = (1.0 / 8, 3.0) if (NV * H * W) % 2 == 0 else (fc.f32(1.0 / 3), 0.7)
    im, al = c.image.clone().requires_grad_(True), c.alpha.clone().requires_grad_(True)
    loss = fit_image_loss(im, al, c.gt_rgb, c.gt_mask, c.bbox, scale=fc.f32(scale))
    (upstream * loss).backward()
    ker = dict(loss=loss.detach().reshape(1), dimage=im.grad, dalpha=al.grad)
    f64 = fc.fit_ref(c, scale, upstream, F64, dev)
    t32 = fc.fit_ref(c, scale, upstream, F32, dev)
    tag = f"fit_loss {NV}x{H}x{W} bbox={'yes' if bbox else 'no'}"
    fc.three_way(ker, t32, f64, ("loss", "dimage", "dalpha"), tag=tag, name="gh_fit_loss")
    passed_k, passed_r = ker["dalpha"].view(-1)[c.special] != 0, f64["dalpha"].view(-1)[c.special] != 0
    assert torch.equal(passed_k, passed_r), tag
    want = torch.tensor(fc.SPECIAL_PASSES, device=dev)[c.which]
    assert torch.equal(passed_r, want), tag
    del f64, t32
    loss = fit_image_loss(im, al, c.gt_rgb, c.gt_mask, c.bbox, scale=fc.f32(scale), guard=guards(dev)[1])
    gi, ga = torch.autograd.grad(upstream * loss, [im, al])
    assert bool(torch.isnan(loss)) and float(gi.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0, tag
    fc.report("gh_fit_loss")
