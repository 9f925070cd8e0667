"""The HIP pooling kernels (include/gh_pool.h) at the shapes, populations and values where they can go wrong, against the float64
per-cell loop of tests/pool_helpers.py, which shares no code with guassianhand_amd.pool and was checked against the restatement on
the CPU (tests/test_pool_cpu.py) on the very same cases.

The sweep (pool_helpers.SWEEP) is no product of its axes; every listed size appears at least once and every case runs every kernel:
a second 64-channel slab with some lanes off (C = 65, 100, 130) and C = 1; a last partial group of 8 cells in the plane kernels
(n_cells = 1, 7, 9, 1023, 1025) and fewer than 8 cells; one to nine passes of the plan's 1024-bin scan up to GH_POOL_MAX_CELLS;
T = 1 and the plan's 256-point block boundary; cells of exactly 0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129 and 300 points spread over
the blocks, everything in one cell, every point its own cell, only the first / last cell occupied, no point in any cell; int32 and
int64 indices with out-of-range values either side of the block boundaries; ties (a quantised grid, constant columns, identical rows
either side of a quarter cut and of a 64-entry chunk), -inf / +inf, and NaN at every place of a cell's list.

Maxima, argmax and the plan are compared bit for bit. Sums are compared under the bound derived in tests/pool_helpers.py from the
loop's own sum|terms| / count; no other tolerance appears. Where the exact value is NaN or infinite (a mean over a cell that
holds one) the kernel must return the same NaN / infinity."""
import pytest
import torch

from guassianhand_amd import _abi, _call, pool
from guassianhand_amd.pool import LocalPoolPointnet, PoolPlan, plane_mean, pool_cat, pool_local, scatter_max, scatter_mean
from tests.pool_helpers import (NAN_VALUES, SWEEP, U, assert_within, assert_within_or_same_nonfinite, case_id, fixture_cfg,
                                fixture_weights, load_fixture, loop_pool, permute_within_cells, plane_bounds, pool_bounds, sweep_case)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KINDS = ("max", "mean")
sweep = pytest.mark.parametrize("case", SWEEP, ids=case_id)


def _on_device(case):
    s = sweep_case(case)
    return s, PoolPlan(s.index.to(DEV), s.n)


def _has_bad(s):
    return bool(((s.index.long() < 0) | (s.index.long() >= s.n)).any())


@sweep
def test_plan_is_the_loops_plan(case):
    s, plan = _on_device(case)
    assert torch.equal(plan.cell_start.cpu(), s.max.cell_start), "cell_start"
    assert torch.equal(plan.order.cpu(), s.max.order), "order"
    if _has_bad(s):
        with pytest.raises(IndexError):
            plan.check()
    else:
        plan.check()


def test_more_cells_than_the_limit_is_refused_before_any_launch():
    index = torch.zeros(300, dtype=torch.int64, device=DEV)
    PoolPlan(index, _abi.GH_POOL_MAX_CELLS)
    with pytest.raises(RuntimeError, match="GH_ERR_UNSUPPORTED"):
        PoolPlan(index, _abi.GH_POOL_MAX_CELLS + 1)
    torch.cuda.synchronize()


@sweep
def test_max_forward_and_argmax_are_the_loops(case):
    s, plan = _on_device(case)
    xd = s.x.to(DEV)
    out = pool_local(xd, plan, "max")
    assert torch.equal(out.cpu(), s.max.pooled.float())
    assert torch.equal(pool.pool_argmax(xd, plan).cpu(), s.max.argmax), "the lowest point index attaining the maximum"
    assert not torch.isnan(out).any()
    cat = pool_cat(xd, plan, "max")
    assert torch.equal(cat[:, s.C:], out)
    left, want = cat[:, :s.C].cpu(), s.x                                               # the input, NaNs included, bit for bit
    assert torch.equal(left.view(torch.int32), want.view(torch.int32))


@sweep
def test_max_backward_lands_on_the_argmax_rows_only(case):
    """Plain and through pool_cat's accumulate path: the whole cell gradient is on the loop's lowest-index row, within the bound of
    the float64 sum; every other element is exactly 0 (plain) or exactly the left half's cotangent (cat)."""
    s, plan = _on_device(case)
    _, bwd, cat_bound = pool_bounds(s.max, "max", s.left)
    xd = s.x.to(DEV).requires_grad_(True)
    pool_local(xd, plan, "max").backward(s.cot.to(DEV))
    got = xd.grad.cpu()
    assert_within(got, s.max.grad, bwd, f"{case_id(case)} max backward")
    assert (got[~s.max.lands] == 0).all()
    xc = s.x.to(DEV).requires_grad_(True)
    pool_cat(xc, plan, "max").backward(torch.cat([s.left, s.cot], dim=1).to(DEV))
    got = xc.grad.cpu()
    assert_within(got, s.left.double() + s.max.grad, cat_bound, f"{case_id(case)} max cat backward")
    assert torch.equal(got[~s.max.lands], s.left[~s.max.lands])


@sweep
def test_mean_forward_and_backward_are_within_the_bound(case):
    s, plan = _on_device(case)
    fwd, bwd, cat_bound = pool_bounds(s.mean, "mean", s.left)
    xd = s.x.to(DEV).requires_grad_(True)
    out = pool_local(xd, plan, "mean")
    assert_within_or_same_nonfinite(out, s.mean.pooled, fwd, f"{case_id(case)} mean forward")
    out.backward(s.cot.to(DEV))
    assert_within(xd.grad, s.mean.grad, bwd, f"{case_id(case)} mean backward")
    xc = s.x.to(DEV).requires_grad_(True)
    cat = pool_cat(xc, plan, "mean")
    assert torch.equal(cat[:, s.C:].view(torch.int32), out.detach().view(torch.int32))
    assert torch.equal(cat[:, :s.C].view(torch.int32), xd.detach().view(torch.int32))
    cat.backward(torch.cat([s.left, s.cot], dim=1).to(DEV))
    assert_within(xc.grad, s.left.double() + s.mean.grad, cat_bound, f"{case_id(case)} mean cat backward")
    no_cell = s.mean.count_pt == 0
    assert (out.detach().cpu()[no_cell] == 0).all() and (xd.grad.cpu()[no_cell] == 0).all()
    assert torch.equal(xc.grad.cpu()[no_cell], s.left[no_cell])


@sweep
def test_plane_mean_and_its_gradient_are_within_the_bound(case):
    s, plan = _on_device(case)
    pf, pb = plane_bounds(s.mean)
    cd = s.x.to(DEV).requires_grad_(True)
    plane = plane_mean(cd, plan)
    assert plane.shape == (s.C, s.n) and plane.is_contiguous()
    assert_within_or_same_nonfinite(plane, s.mean.plane, pf, f"{case_id(case)} plane forward")
    assert (plane.detach().cpu()[:, s.mean.counts == 0] == 0).all()
    plane.backward(s.plane_cot.to(DEV))
    assert_within(cd.grad, s.mean.plane_grad, pb, f"{case_id(case)} plane backward")
    assert (cd.grad.cpu()[s.mean.count_pt == 0] == 0).all()


@pytest.mark.parametrize("case", [c for c in SWEEP if c[3] == "all_bad"], ids=case_id)
def test_no_point_in_any_cell(case):
    s, plan = _on_device(case)
    with pytest.raises(IndexError):
        plan.check()
    assert (plan.cell_start == 0).all() and torch.equal(plan.order.cpu(), torch.arange(s.T, dtype=torch.int32))
    xd = s.x.to(DEV)
    assert (pool.pool_argmax(xd, plan) == s.T).all()
    for kind in KINDS:
        xr = s.x.to(DEV).requires_grad_(True)
        out = pool_local(xr, plan, kind)
        out.backward(s.cot.to(DEV))
        assert (out == 0).all() and (xr.grad == 0).all(), kind
    cr = s.x.to(DEV).requires_grad_(True)
    plane = plane_mean(cr, plan)
    plane.backward(s.plane_cot.to(DEV))
    assert (plane == 0).all() and (cr.grad == 0).all()


@pytest.mark.parametrize("case", [c for c in SWEEP if c[4] in NAN_VALUES], ids=case_id)
def test_the_maximum_does_not_depend_on_where_a_nan_sits_in_its_cell(case):
    s, plan = _on_device(case)
    out = pool_local(s.x.to(DEV), plan, "max")
    empty = pool.pool_argmax(s.x.to(DEV), plan) == s.T
    assert torch.equal(out.cpu(), s.max.pooled.float())
    for seed in (1, 2):
        y = permute_within_cells(s.index, s.x, s.n, seed)
        yd = y.to(DEV)
        arg = pool.pool_argmax(yd, plan)
        assert torch.equal(pool_local(yd, plan, "max"), out) and torch.equal(arg == s.T, empty)
        assert torch.equal(arg.cpu(), loop_pool(y, s.index, s.n, "max").argmax)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [c for c in SWEEP if c[:5] in ((3000, 130, 1025, "ladder", "dup_rows"), (3000, 1, 2500, "all_in_first", "grid"),
                                               (1, 65, 9, "all_in_last", "normal"), (257, 65, 1023, "random", "const_col"))]
assert len(LAYOUT_CASES) == 4


def _window(t, lead=3, tail=4, fill=9.0):
    """t (T,C) as the column window [lead, lead + C) of a wider buffer: row stride > C, start not 16-byte aligned."""
    buf = torch.full((t.shape[0], lead + t.shape[1] + tail), fill, device=DEV)
    buf[:, lead:lead + t.shape[1]] = t.to(DEV)
    return buf, buf[:, lead:lead + t.shape[1]]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=case_id)
def test_column_windows_of_wider_buffers_in_and_out(case):
    s, plan = _on_device(case)
    xd = s.x.to(DEV)
    buf, xw = _window(s.x)
    assert xw.data_ptr() % 16 != 0 and (s.T == 1 or xw.stride(0) > s.C)
    for kind in KINDS:
        want = pool_local(xd, plan, kind)
        xr = xw.detach().requires_grad_(True)
        assert xr.stride() == xw.stride() and xr.data_ptr() == xw.data_ptr()
        got = pool_local(xr, plan, kind)
        assert torch.equal(got.detach(), want), kind
        got.backward(s.cot.to(DEV))
        x0 = xd.clone().requires_grad_(True)
        pool_local(x0, plan, kind).backward(s.cot.to(DEV))
        assert torch.equal(xr.grad, x0.grad), kind
        assert torch.equal(pool_cat(xw, plan, kind)[:, s.C:], want), kind
        obuf, ow = _window(torch.zeros(s.T, s.C), lead=5, tail=2, fill=7.0)
        r = pool_local(xw, plan, kind, out=ow)
        assert r.data_ptr() == ow.data_ptr() and torch.equal(ow, want), kind
        assert (obuf[:, :5] == 7.0).all() and (obuf[:, 5 + s.C:] == 7.0).all(), kind
    assert torch.equal(pool.pool_argmax(xw, plan), pool.pool_argmax(xd, plan))
    assert torch.equal(plane_mean(xw, plan), plane_mean(xd, plan))
    assert (buf[:, :3] == 9.0).all() and (buf[:, 3 + s.C:] == 9.0).all() and torch.equal(xw, xd)
    assert torch.equal(pool_local(xd, plan, "max").cpu(), s.max.pooled.float())


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=case_id)
def test_cotangents_with_stride_zero_and_transposed(case):
    s, plan = _on_device(case)
    xd = s.x.to(DEV)
    g = torch.Generator().manual_seed(21)
    row, row2, col = torch.randn(1, s.C, generator=g).to(DEV), torch.randn(1, 2 * s.C, generator=g).to(DEV), torch.randn(s.C, 1, generator=g).to(DEV)
    tr, tr2, trp = torch.randn(s.C, s.T, generator=g).to(DEV).t(), torch.randn(2 * s.C, s.T, generator=g).to(DEV).t(), torch.randn(s.n, s.C, generator=g).to(DEV).t()

    def grad(fn, cot):
        xr = xd.clone().requires_grad_(True)
        fn(xr).backward(cot)
        return xr.grad

    for kind in KINDS:
        for cot in (row.expand(s.T, s.C), tr):
            assert s.T == 1 or s.C == 1 or not cot.is_contiguous()
            assert torch.equal(grad(lambda t: pool_local(t, plan, kind), cot), grad(lambda t: pool_local(t, plan, kind), cot.contiguous())), kind
        for cot in (row2.expand(s.T, 2 * s.C), tr2):
            assert torch.equal(grad(lambda t: pool_cat(t, plan, kind), cot), grad(lambda t: pool_cat(t, plan, kind), cot.contiguous())), kind
    for cot in (col.expand(s.C, s.n), trp):
        assert torch.equal(grad(lambda t: plane_mean(t, plan), cot), grad(lambda t: plane_mean(t, plan), cot.contiguous()))
    # and against the loop, for the stride-0 cotangent of the maximum
    lp = loop_pool(s.x, s.index, s.n, "max", row.expand(s.T, s.C))
    got = grad(lambda t: pool_local(t, plan, "max"), row.expand(s.T, s.C)).cpu()
    assert_within(got, lp.grad, pool_bounds(lp, "max")[1], f"{case_id(case)} max backward, stride-0 cotangent")
    assert (got[~lp.lands] == 0).all()


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=case_id)
def test_raw_entry_points_with_column_offsets_and_strided_gradients(case):
    """What the Python wrappers never pass: out_col > 0 on the base pointer of the (T, 2C) buffer, accumulate = 1 into a grad_x of
    row stride 2C, x_stride > C for the plane. Bit-equal to the view-pointer forms."""
    s, plan = _on_device(case)
    L, T, Cc, n = _call.lib(), s.T, s.C, s.n
    ptr, stream = _call.ptr, _call.stream(DEV)
    xd = s.x.to(DEV)
    G = torch.cat([s.left, s.cot], dim=1).to(DEV).contiguous()
    for kind in KINDS:
        red = pool._REDUCE[kind]
        xc = xd.clone().requires_grad_(True)
        want = pool_cat(xc, plan, kind)
        want.backward(G)
        buf = torch.full((T, 2 * Cc), 7.0, device=DEV)
        buf[:, :Cc] = xd
        argmax = torch.full((n, Cc), -5, dtype=torch.int32, device=DEV)
        rc = L.gh_pool_forward(ptr(buf), 2 * Cc, T, Cc, n, ptr(plan.cell_start), ptr(plan.order), red, ptr(buf), 2 * Cc, Cc, ptr(argmax),
                               stream)
        assert rc == 0, _abi.status_name(rc)
        assert torch.equal(buf.view(torch.int32), want.detach().view(torch.int32)), kind
        if kind == "max":
            assert torch.equal(argmax.long(), pool.pool_argmax(xd, plan))
        gx = torch.full((T, 2 * Cc), 3.0, device=DEV)                       # prefilled: the left half's gradient, then a sentinel
        gx[:, :Cc] = G[:, :Cc]
        rc = L.gh_pool_backward(ptr(G), 2 * Cc, Cc, T, Cc, n, ptr(plan.cell_start), ptr(plan.order), red, ptr(argmax), ptr(gx), 2 * Cc, 1,
                                stream)
        assert rc == 0, _abi.status_name(rc)
        assert torch.equal(gx[:, :Cc], xc.grad) and (gx[:, Cc:] == 3.0).all(), kind
    wide = torch.full((T, 2 * Cc), 7.0, device=DEV)
    wide[:, :Cc] = xd
    plane = torch.empty(Cc, n, device=DEV)
    rc = L.gh_plane_mean_forward(ptr(wide), 2 * Cc, T, Cc, n, ptr(plan.cell_start), ptr(plan.order), ptr(plane), stream)
    assert rc == 0, _abi.status_name(rc)
    want = plane_mean(xd, plan)
    assert torch.equal(plane.view(torch.int32), want.view(torch.int32))
    torch.cuda.synchronize()


# ---- torch_scatter's two functions on device tensors -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.int32, torch.int64), ids=("i32", "i64"))
def test_scatter_drop_ins_on_the_device(dtype):
    g = torch.Generator().manual_seed(31)
    B, Cc, T, n = 2, 65, 700, 9
    src = torch.randint(-3, 4, (B, Cc, T), generator=g).float() / 4        # ties everywhere
    src[1] = torch.randn(Cc, T, generator=g)
    index = torch.randint(0, n - 1, (B, 1, T), generator=g).to(dtype)       # cell n-1 stays empty
    index[1] = index[1].flip(-1) // 2
    sd, idd = src.to(DEV), index.to(DEV)
    out, arg = scatter_max(sd, idd, dim_size=n)
    out_c, arg_c = scatter_max(src, index, dim_size=n)
    assert out.shape == (B, Cc, n) and arg.dtype == torch.int64 and out.device.type == "cuda"
    assert torch.equal(out.cpu(), out_c) and torch.equal(arg.cpu(), arg_c)
    mean = scatter_mean(sd, idd, dim_size=n)
    mean_c = scatter_mean(src, index, dim_size=n)
    for b in range(B):
        lp = loop_pool(src[b].t(), index[b, 0], n, "max")
        assert torch.equal(arg[b].cpu(), lp.argmax.t())
        cells = torch.where(lp.argmax == T, torch.zeros(()), src[b].t().gather(0, lp.argmax.clamp(max=T - 1)))
        assert torch.equal(out[b].cpu(), cells.t())
        assert (lp.counts == 0).any() and (out[b].cpu()[:, lp.counts == 0] == 0).all() and (arg[b].cpu()[:, lp.counts == 0] == T).all()
        bound = lp.counts.double() * U * lp.abs_plane + U * lp.plane.abs()
        assert_within(mean[b], lp.plane, bound, f"scatter_mean[{b}] on the device vs the loop")
        assert_within(mean[b], mean_c[b], bound, f"scatter_mean[{b}] on the device vs on the CPU", slack=2.0)   # two float32 sums
    fea = torch.zeros(B, Cc, n, device=DEV)                                # generate_plane_features' form
    ret = scatter_mean(sd, idd, out=fea)
    assert ret is fea and torch.equal(fea, mean)
    scatter_mean(sd, idd, out=fea)                                         # accumulated into, not overwritten
    assert torch.equal(fea, mean + mean)
    with pytest.raises(NotImplementedError):
        scatter_max(sd, idd, out=fea)


# ---- the encoder on a batch ------------------------------------------------------------------------------------------------------------
def test_encoder_on_a_batch_of_two_clouds_fused_equals_plain_torch_ops_on_the_device():
    """As the B = 1 test of tests/test_gpu_pool.py: same module, same device, same GEMMs, so every pooled tensor is bit-equal; the
    planes are float32 means of the same rows, each within the bound of the float64 value."""
    fx = load_fixture()
    p = torch.cat([fx["p"], fx["p"].flip(1) * 0.7 + 0.05], dim=0)
    radius, ps = float(fx["radius"]), int(fx["dims"][4])
    index = pool.cell_index(p, radius, ps)
    assert not torch.equal(index[0], index[1])

    def run(ops):
        m = LocalPoolPointnet(fixture_cfg(fx, "max"), ops=ops)
        m.load_state_dict(fixture_weights(fx))
        m = m.to(DEV)
        m.pool_record, cs = [], []
        m.fc_c.register_forward_hook(lambda mod, a, o: cs.append(o.detach()))
        return m, m(p.to(DEV)).detach(), cs

    mf, plane_f, c_f = run("fused")
    mt, plane_t, c_t = run("torch")
    assert plane_f.shape == (2, int(fx["dims"][3]), ps, ps)
    assert len(mf.pool_record) == len(mt.pool_record) == 2 * 4 == 2 * (int(fx["dims"][5]) - 1) and len(c_f) == len(c_t) == 2
    for k, (a, b) in enumerate(zip(mf.pool_record, mt.pool_record)):
        assert torch.equal(a, b), f"cloud {k // 4}, pooled tensor of block {k % 4 + 1}"
    for b in range(2):
        assert torch.equal(c_f[b], c_t[b])
        lp = loop_pool(c_f[b].cpu(), index[b], ps * ps, "mean")
        bound = lp.counts.double() * U * lp.abs_plane + U * lp.plane.abs()
        assert_within(plane_f[b].reshape(lp.plane.shape), lp.plane, bound, f"cloud {b}: fused plane vs the loop")
        assert_within(plane_f[b].reshape(lp.plane.shape), plane_t[b].reshape(lp.plane.shape), bound, f"cloud {b}: fused vs plain-torch plane",
                      slack=2.0)
