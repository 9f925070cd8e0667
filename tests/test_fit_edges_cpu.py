"""The references and case generators of tests/fit_cases.py, pinned on the CPU on the very cases tests/test_gpu_fit_edges.py draws:
the Adam reference against one torch.optim.Adam step in float64, the gather reference against a per-point loop in numpy float64,
the loss references' behaviour at the clip bounds and at ties, the populations the generators promise, and uvmap.ActiveTexels on an
empty and on an all-outside set of UVs. No GPU compute is launched here.

Two float64 evaluations of one formula differ by the rounding of their different operation orders only. They are compared under
k * 2^-53 * (the magnitude that enters the rounding), with k the number of roundings on the longer path, stated at each use."""
import numpy as np
import pytest
import torch

from guassianhand_amd.uvmap import ActiveTexels
from tests import fit_cases as fc

E64 = 2.0 ** -53


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in fc.ADAM_N if n <= 1025])
def test_adam_reference_is_one_torch_adam_step_in_float64(n):
    """fit_cases.adam_ref(float64) == torch.optim.Adam in float64 with the state injected, the float32-valued coefficients passed as
    Python floats and the regulariser's gradient added by autograd. At most 12 float64 roundings lie between the inputs and any
    output on either path (torch's lerp and addcdiv order them differently), each relative to a quantity no larger than the
    largest |value| of the field or, for the parameter, |p| + the step: 16 * 2^-53 * max is the bound."""
    s = fc.adam_state(n)
    lr, b1, b2, eps = fc.f32(fc.ADAM_LR), fc.f32(fc.ADAM_BETAS[0]), fc.f32(fc.ADAM_BETAS[1]), fc.f32(fc.ADAM_EPS)
    for t in fc.ADAM_T:
        m, v = (s.m, s.v) if t > 1 else (torch.zeros_like(s.m), torch.zeros_like(s.v))
        for l1, l2 in fc.ADAM_REG:
            want = fc.adam_ref(s.p, s.g, m, v, t, fc.ADAM_LR, fc.ADAM_BETAS, fc.ADAM_EPS, l1, l2, torch.float64)
            p = s.p.double().clone().requires_grad_(True)
            opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
            opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
            ((s.g.double() * p).sum() + fc.f32(l1) * p.abs().sum() + fc.f32(l2) * p.pow(2).sum()).backward()
            opt.step()
            got = dict(param=p.detach(), exp_avg=opt.state[p]["exp_avg"], exp_avg_sq=opt.state[p]["exp_avg_sq"])
            assert float(opt.state[p]["step"]) == t
            for k in ("param", "exp_avg", "exp_avg_sq"):
                err, mag = float((got[k] - want[k]).abs().max()), float(want[k].abs().max())
                assert err <= 16 * E64 * mag, (n, t, l1, l2, k, err, mag)
            # a zero parameter with a zero gradient stays exactly zero, with its sign, and so do its moments
            z = s.zero
            assert torch.equal(fc.bits(want["param"][z].float()), fc.bits(s.p[z]))
            assert float(want["exp_avg"][z].abs().sum()) == 0.0 and float(want["exp_avg_sq"][z].abs().sum()) == 0.0
            assert float(want["sums"][0]) == float(s.p.double().abs().sum()) and float(want["sums"][1]) == float((s.p.double() ** 2).sum())


def test_adam_reference_forms_one_minus_beta_from_the_float32_betas():
    """The decision of the issue: 1 - float32(0.999) = 0.00099998713, not 0.001; the decimal form is what torch multiplies by."""
    p, g, z = torch.tensor([0.25]), torch.tensor([0.5]), torch.zeros(1)
    a = fc.adam_ref(p, g, z, z, 1, 0.01, (0.9, 0.999), 1e-8, 0.0, 0.0, torch.float64)
    b = fc.adam_ref(p, g, z, z, 1, 0.01, (0.9, 0.999), 1e-8, 0.0, 0.0, torch.float64, coeffs="decimal")
    assert float(a["exp_avg_sq"]) == (1.0 - float(np.float32(0.999))) * 0.25 and float(b["exp_avg_sq"]) == (1.0 - 0.999) * 0.25
    assert float(np.float32(1.0) - np.float32(0.999)) == 1.0 - float(np.float32(0.999))       # exact in float32 too (Sterbenz)
    assert abs(float(a["exp_avg_sq"]) / float(b["exp_avg_sq"]) - 1.0) == pytest.approx(1.3e-5, rel=0.05)


def test_adam_states_hold_the_promised_populations():
    for n in fc.ADAM_N:
        s = fc.adam_state(n)
        i = torch.arange(n)
        assert all(x.dtype == torch.float32 and x.shape == (n,) and bool(torch.isfinite(x).all()) for x in (s.p, s.g, s.m, s.v))
        assert torch.equal(s.zero, (i % 7 == 3) | (i % 7 == 5)) and torch.equal(s.p == 0, s.zero)
        assert bool((fc.bits(s.p)[i % 7 == 3] == 0).all()) and bool((fc.bits(s.p)[i % 7 == 5] == -2 ** 31).all())      # +0.0 and -0.0
        assert float(s.g[s.zero].abs().sum()) == 0.0 and float(s.m[s.zero].abs().sum()) == 0.0 and float(s.v[s.zero].abs().sum()) == 0.0
        assert torch.equal(s.g == 0, s.zero | (i % 7 == 6)) and bool((s.g[s.g != 0].abs() >= 1e-6).all())
        assert bool((s.v >= s.m * s.m).all())
        if n >= 6:
            assert bool((i % 7 == 3).any()) and bool((i % 7 == 5).any())
    assert fc.adam_state(5) is fc.adam_state(5)


# ---- gather ----------------------------------------------------------------------------------------------------------------------------
CPU_GATHER = [c for c in fc.GATHER_CASES if c[1] * c[2] <= 64 * 128 and c[0] <= 257]


@pytest.mark.parametrize("case", CPU_GATHER, ids=fc.gather_id)
def test_gather_reference_is_the_per_point_loop(case):
    """grid_sample in float64 (fit_cases.gather_ref) against the four-corner loop in numpy float64, outputs and the transpose. Both
    round ix = (u + 1) / 2 * (Wm - 1) (three roundings at magnitude <= 1.1 Wm, so a weight is off by up to 4 Wm 2^-53), then a
    product and at most three additions per corner: 8 max(Hm, Wm) 2^-53 times the sum of |texel| (resp. |cotangent|) that entered."""
    P, Hm, Wm, C, (Ca, Cb), kind = case
    uv = fc.gather_uvs(case)
    at = ActiveTexels(uv, Hm, Wm)
    t = fc.gather_tensors(case, at.U)
    for tex, dout in ((t.tex, t.dout), (t.tex_a, t.dout_a), (t.tex_b, t.dout_b)):
        ref = fc.gather_ref(tex, at, uv, dout, torch.float64)
        dense = at.dense(tex.double())
        out, grad, agrad = fc.loop_gather(dense.numpy(), uv.numpy(), dout.numpy())
        assert ref["out"].shape == (P, tex.shape[1]) and ref["grad"].shape == (at.U, tex.shape[1])
        k = 8 * max(Hm, Wm) * E64
        if P:
            bound = k * float(tex.abs().max()) * 4 if at.U else 0.0
            assert float((ref["out"] - torch.from_numpy(out)).abs().max()) <= bound
        g, ag = at.compact(torch.from_numpy(grad)), at.compact(torch.from_numpy(agrad))
        assert bool(((ref["grad"] - g).abs() <= k * ag).all())
        # nothing lands outside the active set
        assert float((torch.from_numpy(grad) - at.dense(g)).abs().max()) == 0.0
    if kind == "outside":
        assert at.U == 0 and float(fc.gather_ref(t.tex, at, uv, t.dout, torch.float64)["out"].abs().max()) == 0.0


def test_gather_cases_hold_the_promised_populations():
    seen_P, seen_C, seen_pair, seen_map = set(), set(), set(), set()
    for case in fc.GATHER_CASES:
        P, Hm, Wm, C, pair, kind = case
        seen_P.add(P); seen_C.add(C); seen_pair.add(pair); seen_map.add((Hm, Wm))
        uv = fc.gather_uvs(case)
        assert uv.shape == (P, 2) and uv.dtype == torch.float32 and bool(torch.isfinite(uv).all())
        at = ActiveTexels(uv, Hm, Wm)
        if kind == "edge" and P >= 9:
            assert bool((uv.abs() == 1).any()) and bool((uv.abs() > 1).any()) and float(uv.abs().max()) <= 1.1
            if Hm > 1 and Wm > 1:
                assert bool((at.slot < 0).any()) and bool((at.slot >= 0).any())            # corners in and out of the map
        if kind == "one_uv":
            assert P == 4096 and bool((uv == uv[0]).all()) and at.U == 4 and bool((at.slot >= 0).all())
            assert at.row_ptr.tolist() == [0, P, 2 * P, 3 * P, 4 * P]                   # each of the four texels takes all P points
        if kind == "outside":
            assert at.U == 0 and bool((at.slot == -1).all())
    assert seen_P >= {0, 1, 63, 64, 65, 257, 4099} and seen_C == {1, 3, 48, 65}
    assert seen_pair == {(48, 1), (1, 48), (3, 1), (65, 2)} and seen_map == {(1, 1), (2, 3), (64, 128), (1024, 2048)}
    assert (4099, 1024, 2048, 48, (48, 1), "edge") in fc.GATHER_CASES                   # the fit's own configuration


@pytest.mark.parametrize("case", [c for c in fc.GATHER_CASES if c[0] == 0 or c[5] == "outside"], ids=fc.gather_id)
def test_texel_index_of_no_points_and_of_all_outside_uvs(case):
    P, Hm, Wm = case[:3]
    at = ActiveTexels(fc.gather_uvs(case), Hm, Wm)
    assert at.U == 0 and at.P == P and at.index.numel() == 0
    assert at.slot.shape == (P, 4) and at.slot.dtype == torch.int32 and bool((at.slot == -1).all())
    assert at.w.shape == (P, 4) and at.w.dtype == torch.float32
    assert at.row_ptr.tolist() == [0] and at.row_ptr.dtype == torch.int32
    assert at.pairs.numel() == 0 and at.pairs.dtype == torch.int32
    assert at.compact(torch.zeros(Hm, Wm, 3)).shape == (0, 3) and float(at.dense(torch.zeros(0, 3)).abs().sum()) == 0.0


# ---- losses ----------------------------------------------------------------------------------------------------------------------------
def test_l1_cases_and_reference():
    for n in fc.L1_N:
        a, b = fc.l1_case(n)
        i = torch.arange(n)
        tie = i % 7 == 0
        assert torch.equal(a == b, tie)
        assert bool((fc.bits(a)[i % 21 == 0] == 0).all()) and bool((fc.bits(b)[i % 21 == 0] == -2 ** 31).all())
        assert bool((fc.bits(a)[i % 21 == 7] == -2 ** 31).all()) and bool((fc.bits(b)[i % 21 == 7] == 0).all())
        loss, grad = fc.l1_ref(a, b)
        assert loss.dtype == torch.float64 and grad.dtype == torch.float32 and grad.shape == a.shape
        assert bool((fc.bits(grad)[tie] == 0).all())                                     # sign(0) = +0, also for +0 against -0
        s = np.float32(1.0 / n)
        assert torch.equal(grad[~tie], torch.where(a > b, torch.tensor(s), torch.tensor(-s))[~tie])
        # the float64 autograd gradient is the same decision, scaled by the double 1 / n
        x = a.double().requires_grad_(True)
        (x - b.double()).abs().mean().backward()
        assert torch.equal(torch.sign(x.grad), torch.sign(grad.double())) and float(loss) == float((a.double() - b.double()).abs().mean())


def test_fit_cases_hold_the_promised_populations():
    for NV, H, W in fc.FIT_SHAPES[:-1]:
        for bbox in (False, True):
            c = fc.fit_case(NV, H, W, bbox)
            npix = NV * H * W
            assert c.image.shape == (NV, 3, H, W) and c.alpha.shape == (NV, H, W) and c.gt_rgb.shape == (NV, H, W, 3)
            assert (c.bbox is None) == (not bbox) and (c.bbox is None or set(c.bbox.unique().tolist()) <= {0.0, 1.0})
            assert float(c.alpha.min()) >= -0.1 and float(c.alpha.max()) <= 1.2
            got = c.alpha.view(-1)[c.special].numpy()
            assert np.array_equal(got, fc.SPECIAL[c.which.numpy()]) and c.special.numel() == (npix if npix <= 6 else (npix + 4) // 5)
            if npix >= 30:
                assert set(c.which.tolist()) == set(range(6))
            assert bool((c.image.view(-1)[::11] == c.gt_rgb.permute(0, 3, 1, 2).reshape(-1)[::11]).all())
    assert float(fc.SPECIAL[0]) < -0.001 < float(fc.SPECIAL[2]) and fc.SPECIAL[1] < fc.SPECIAL[0]      # float32(-0.001) lies below -0.001
    assert fc.SPECIAL[5] < fc.SPECIAL[3] == 1.0 < fc.SPECIAL[4]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("bbox", [False, True])
def test_fit_reference_passes_the_gradient_on_the_closed_float32_interval(dtype, bbox):
    """A gradient at -0.001f and at 1.0f, none at nextafter beyond either, in float64 as in float32: a float64 restatement with the
    decimal bound -0.001 would deny it at -0.001f."""
    for NV, H, W in fc.FIT_SHAPES[:-1]:
        c = fc.fit_case(NV, H, W, bbox)
        r = fc.fit_ref(c, 1.0 / 8, 3.0, dtype)
        assert r["loss"].dtype == dtype and r["dalpha"].dtype == dtype and r["dimage"].shape == c.image.shape
        passed = r["dalpha"].view(-1)[c.special] != 0
        assert passed.tolist() == [fc.SPECIAL_PASSES[w] for w in c.which.tolist()]
        # where it passes, d/dalpha = upstream * scale * lambda_m * 2 (alpha - mask) / (H W). fit_loss's own `.float()` makes autograd
        # round this gradient to float32 ONCE on its way back (see fit_ref), also in float64: 2 * 2^-24 there; the float32 run has
        # the six roundings of its chain (sub, pow, mean, lambda, scale, upstream) on top
        al, gm = c.alpha.view(-1)[c.special].double(), c.gt_mask.view(-1)[c.special].double()
        want = torch.where(passed, 3.0 / 8 * 2.0 * (al - gm) / (H * W), torch.zeros_like(al))
        k = 8 if dtype == torch.float32 else 2
        assert bool(((r["dalpha"].view(-1)[c.special].double() - want).abs() <= k * 2.0 ** -24 * want.abs()).all())
        # ties and pixels outside the bbox carry no colour gradient
        tie = (c.image == c.gt_rgb.permute(0, 3, 1, 2))
        if c.bbox is None:
            assert float(r["dimage"][tie].abs().sum()) == 0.0
        else:
            assert float(r["dimage"][(c.bbox == 0)[:, None].expand_as(c.image)].abs().sum()) == 0.0
