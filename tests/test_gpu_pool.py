"""The HIP pooling kernels (include/gh_pool.h) against the plain-torch restatement of guassianhand_amd.pool: the fixture's sizes
and the real one — T = 98 562 points, C = 128 (pool) / 512 (plane), 1024 cells, the cell index derived the reference's way from the
two-hand scene's points, so that most cells are empty and the fullest hold over a thousand points.

Maxima are exact, so they are compared bit for bit. Sums are compared with the float64 restatement under the bound derived in
tests/pool_helpers.py: n * u * sum|terms| / count + u * |result|. Where one more term is added to a finished sum (the cat
buffer's backward: the left half's gradient plus the pooled half's) that is one more rounding, relative to at most
|left| + sum|terms| / count, hence (n + 1) * u * (|left| + sum|terms| / count)."""
import pytest
import torch

from guassianhand_amd import pool
from guassianhand_amd.pool import LocalPoolPointnet, PoolPlan, plane_mean, pool_cat, pool_local
from guassianhand_amd.scenes import make_scene
from tests.pool_helpers import U, assert_within, fixture_cfg, fixture_weights, load_fixture, rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T_REAL, N_CELLS, PLANE = 98562, 1024, 32
KINDS = ("max", "mean")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def real():
    """(index (T,) int64 on the CPU, per-cell counts): the two-hand scene's points through the reference's index formula with the
    shade encoder's radius (config_one_shot.yaml:164,178)."""
    sc = make_scene("two_hands", n_views=1, P=T_REAL)
    assert sc.xyz.shape[0] == T_REAL
    index = pool.cell_index(sc.xyz[None], 0.2, PLANE)[0]
    counts = torch.bincount(index, minlength=N_CELLS)
    assert (counts == 0).any(), "no empty cell"
    assert counts.max() > 256, f"the fullest cell holds {int(counts.max())} points"
    return index, counts


def _cases(fx, real, C):
    g = torch.Generator().manual_seed(C)
    yield "fixture", fx["max_index"], fx["max_op_pool_in"], int(fx["dims"][4]) ** 2
    yield "real", real[0], torch.randn(T_REAL, C, generator=g), N_CELLS


def test_plan_equals_the_cpu_plan(fx, real):
    for name, index, _, n in _cases(fx, real, 1):
        for idx in (index, index.to(torch.int32)):
            cpu, gpu = PoolPlan(idx, n), PoolPlan(idx.to(DEV), n)
            assert torch.equal(gpu.cell_start.cpu(), cpu.cell_start) and torch.equal(gpu.order.cpu(), cpu.order), name
            gpu.check()


def test_max_forward_and_argmax_are_bit_equal(fx, real):
    for name, index, x, n in _cases(fx, real, 128):
        cpu = PoolPlan(index, n)
        gpu = PoolPlan(index.to(DEV), n)
        want = pool_local(x, cpu, "max")
        xd = x.to(DEV)
        assert torch.equal(pool_local(xd, gpu, "max").cpu(), want), name
        assert torch.equal(pool.pool_argmax(xd, gpu).cpu(), pool.pool_argmax(x, cpu)), name
        # the strided form: the right half of a (T, 2C) buffer whose left half is the input
        C = x.shape[1]
        buf = torch.full((x.shape[0], 2 * C), 7.0, device=DEV)
        buf[:, :C] = xd
        r = pool_local(buf[:, :C], gpu, "max", out=buf[:, C:])
        assert r.data_ptr() == buf[:, C:].data_ptr()
        assert torch.equal(buf[:, :C], xd) and torch.equal(buf[:, C:].cpu(), want), name
        cat = pool_cat(xd, gpu, "max")
        assert torch.equal(cat, buf), name


@pytest.mark.parametrize("kind", KINDS)
def test_pool_values_and_gradients_are_within_the_bound(fx, real, kind):
    for name, index, x, n in _cases(fx, real, 128):
        cpu, gpu = PoolPlan(index, n), PoolPlan(index.to(DEV), n)
        cnt = cpu.counts().double()[index].unsqueeze(1)
        g = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
        gl = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
        xd = x.to(DEV).requires_grad_(True)
        out = pool_local(xd, gpu, kind)
        out.backward(g.to(DEV))
        x64 = x.double().requires_grad_(True)
        ref = pool._pool_local_ref(x64, cpu, kind)
        ref.backward(g.double())
        xa = x.double().requires_grad_(True)
        pool._pool_local_ref(xa, cpu, kind).backward(g.double().abs())            # sum|g| (/ count) where the sum lands
        if kind == "mean":
            absx = pool._pool_local_ref(x.abs(), cpu, "mean", acc=torch.float64)
            assert_within(out, ref, cnt * U * absx + U * ref.detach().abs(), f"{name} mean forward")
            assert_within(xd.grad, x64.grad, cnt * U * xa.grad + U * x64.grad.abs(), f"{name} mean backward")
        else:
            assert torch.equal(out.detach().cpu(), ref.detach().float())
            assert_within(xd.grad, x64.grad, cnt * U * xa.grad, f"{name} max backward")
            assert (xd.grad.cpu()[x64.grad == 0] == 0).all()                          # nothing lands beside the argmax rows
        # the cat buffer: left half's gradient + the pooled half's, in one pass
        xc = x.to(DEV).requires_grad_(True)
        cat = pool_cat(xc, gpu, kind)
        assert torch.equal(cat[:, x.shape[1]:], out.detach()) and torch.equal(cat[:, :x.shape[1]], xc.detach())
        cat.backward(torch.cat([gl, g], dim=1).to(DEV))
        assert_within(xc.grad, gl.double() + x64.grad, (cnt + 1) * U * (gl.double().abs() + xa.grad), f"{name} {kind} cat backward")


def test_plane_mean_and_its_gradient_are_within_the_bound(fx, real):
    for name, index, c, n in _cases(fx, real, 512):
        cpu, gpu = PoolPlan(index, n), PoolPlan(index.to(DEV), n)
        cd = c.to(DEV).requires_grad_(True)
        plane = plane_mean(cd, gpu)
        assert plane.shape == (c.shape[1], n) and plane.is_contiguous()
        cot = torch.randn(plane.shape, generator=torch.Generator().manual_seed(8))
        plane.backward(cot.to(DEV))
        c64 = c.double().requires_grad_(True)
        ref = pool._plane_mean_ref(c64, cpu)
        ref.backward(cot.double())
        bound = cpu.counts().double() * U * pool._plane_mean_ref(c.abs(), cpu, acc=torch.float64) + U * ref.detach().abs()
        assert_within(plane, ref, bound, f"{name} plane forward")
        assert (plane[:, (cpu.counts() == 0).to(DEV)] == 0).all()
        assert_within(cd.grad, c64.grad, 2 * U * c64.grad.abs(), f"{name} plane backward")      # one term, one division


def test_two_runs_of_every_kernel_are_bitwise_identical(real):
    index = real[0].to(DEV)
    g = torch.Generator().manual_seed(9)
    x, c = torch.randn(T_REAL, 128, generator=g).to(DEV), torch.randn(T_REAL, 512, generator=g).to(DEV)
    cot_x, cot_p = torch.randn(T_REAL, 256, generator=g).to(DEV), torch.randn(512, N_CELLS, generator=g).to(DEV)

    def run():
        plan = PoolPlan(index, N_CELLS)
        outs = [plan.cell_start, plan.order]
        for kind in KINDS:
            xr = x.clone().requires_grad_(True)
            cat = pool_cat(xr, plan, kind)
            cat.backward(cot_x)
            xs = x.clone().requires_grad_(True)
            o = pool_local(xs, plan, kind)
            o.backward(cot_x[:, :128])
            outs += [cat.detach(), xr.grad, o.detach(), xs.grad]
        cr = c.clone().requires_grad_(True)
        pl = plane_mean(cr, plan)
        pl.backward(cot_p)
        return outs + [pl.detach(), cr.grad, pool.pool_argmax(x, plan)]

    a, b = run(), run()
    torch.cuda.synchronize()
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(s, t), i


def test_out_of_range_indices_are_skipped_and_reported(real):
    """The kernels give such points a bin of their own after the last cell: they are written zeros and read by no reduction."""
    index = real[0]
    bad_at = torch.tensor([0, 4097, 50000, T_REAL - 1])
    bad_index = index.clone()
    bad_index[bad_at] = torch.tensor([N_CELLS, -1, 1 << 40, N_CELLS + 7])
    keep = torch.ones(T_REAL, dtype=torch.bool)
    keep[bad_at] = False
    g = torch.Generator().manual_seed(10)
    x = torch.randn(T_REAL, 128, generator=g).to(DEV)
    plan, sub = PoolPlan(bad_index.to(DEV), N_CELLS), PoolPlan(index[keep].to(DEV), N_CELLS)
    with pytest.raises(IndexError):
        plan.check()
    sub.check()
    assert torch.equal(plan.cell_start, sub.cell_start)
    keep_d = keep.to(DEV)
    for kind in KINDS:
        xr, xs = x.clone().requires_grad_(True), x[keep_d].clone().requires_grad_(True)
        out, want = pool_local(xr, plan, kind), pool_local(xs, sub, kind)
        assert (out[bad_at.to(DEV)] == 0).all() and torch.equal(out[keep_d], want), kind
        cot = torch.randn(T_REAL, 128, generator=g).to(DEV)
        out.backward(cot)
        want.backward(cot[keep_d])
        assert (xr.grad[bad_at.to(DEV)] == 0).all() and torch.equal(xr.grad[keep_d], xs.grad), kind
    cr, cs = x.clone().requires_grad_(True), x[keep_d].clone().requires_grad_(True)
    pl, pw = plane_mean(cr, plan), plane_mean(cs, sub)
    assert torch.equal(pl, pw)
    cot = torch.randn(128, N_CELLS, generator=g).to(DEV)
    pl.backward(cot)
    pw.backward(cot)
    assert (cr.grad[bad_at.to(DEV)] == 0).all() and torch.equal(cr.grad[keep_d], cs.grad)


def test_a_whole_forward_and_backward_replays_from_a_graph(real):
    index = real[0].to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T_REAL, 128, generator=g).to(DEV).requires_grad_(True)
    cot = torch.randn(128, N_CELLS, generator=g).to(DEV)

    def step():
        plan = PoolPlan(index, N_CELLS)
        h = x
        for _ in range(4):
            cat = pool_cat(h, plan, "max")
            h = cat[:, 128:] + 0.5 * cat[:, :128]
        plane = plane_mean(h, plan)
        (gx,) = torch.autograd.grad(plane, x, cot)
        return plane, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for a, b in zip(cap, eager):
        assert torch.equal(a, b)
    with torch.no_grad():                                                   # new inputs in the same buffers: the replay follows them
        x.mul_(-1.0)
        index.copy_(index.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    eager2 = step()
    for a, b, c in zip(cap, eager2, eager):
        assert torch.equal(a, b) and not torch.equal(b, c)


def _encoder(fx, kind, ops, dev):
    m = LocalPoolPointnet(fixture_cfg(fx, kind), ops=ops)
    m.load_state_dict(fixture_weights(fx))
    m = m.to(dev)
    m.pool_record, cs = [], []
    m.fc_c.register_forward_hook(lambda mod, a, o: cs.append(o.detach()))
    p = fx["p"].to(dev).requires_grad_(True)
    plane = m(p)
    plane.backward(fx["cot"].to(dev))
    return m, p, plane.detach(), cs[0]


def test_encoder_with_fused_ops_equals_the_plain_torch_ops_on_the_device(fx):
    """Same module, same device, same rocBLAS GEMMs: every pooled tensor is bit-equal; the two planes are float32 means of the
    same rows, each within the bound of the float64 value, so within twice the bound of each other."""
    mf, pf, plane_f, c_f = _encoder(fx, "max", "fused", DEV)
    mt, pt, plane_t, c_t = _encoder(fx, "max", "torch", DEV)
    assert len(mf.pool_record) == len(mt.pool_record) == 4
    for k, (a, b) in enumerate(zip(mf.pool_record, mt.pool_record), 1):
        assert torch.equal(a, b), f"pooled tensor of block {k}"
    assert torch.equal(c_f, c_t)
    plan = PoolPlan(fx["max_index"].to(DEV), 64)
    exact = pool._plane_mean_ref(c_f, plan, acc=torch.float64)
    bound = plan.counts().double() * U * pool._plane_mean_ref(c_f.abs(), plan, acc=torch.float64) + U * exact.abs()
    assert_within(plane_f.reshape(exact.shape), exact, bound, "fused plane vs float64")
    assert_within(plane_f.reshape(exact.shape), plane_t.reshape(exact.shape), bound, "fused plane vs plain-torch plane", slack=2.0)


@pytest.mark.parametrize("kind", KINDS)
def test_encoder_is_as_close_to_the_cpu_fixture_as_plain_torch_on_the_device(fx, kind):
    """CPU and GPU GEMMs round differently by an amount nobody fixed; the fused path must be no further from the CPU-recorded
    fixture than twice the plain-torch path on the same device (they share every GEMM and may differ only in which of two
    near-equal rows wins a maximum, and in the order of the sums)."""
    mf, pf, plane_f, _ = _encoder(fx, kind, "fused", DEV)
    mt, pt, plane_t, _ = _encoder(fx, kind, "torch", DEV)
    want = fx[f"{kind}_plane"]
    d_f, d_t = (plane_f.cpu() - want).abs().max().item(), (plane_t.cpu() - want).abs().max().item()
    print(f"{kind} plane max |diff| to the fixture: fused {d_f:.3e}, plain torch {d_t:.3e}")
    assert d_f <= 2 * d_t, (kind, d_f, d_t)
    for name, a, b in (("grad_p", pf.grad, pt.grad), ("grad_fc_pos_w", mf.fc_pos.weight.grad, mt.fc_pos.weight.grad)):
        r_f, r_t = rel_l2(a, fx[f"{kind}_{name}"]), rel_l2(b, fx[f"{kind}_{name}"])
        print(f"{kind} {name} rel-L2 to the fixture: fused {r_f:.3e}, plain torch {r_t:.3e}")
        assert r_f <= 2 * r_t, (kind, name, r_f, r_t)
