"""The kernels of include/gh_res.h on the device, under the three-way rule of tests/test_gpu_vert_mlp.py: on the same inputs the float64
restatement, the float32 torch statements (the unfolded ResnetBlockFC over the materialised concatenation) and the kernel are computed
on the device, and per field

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

The three errors are printed per field. Cases and yardsticks: tests/res_block_cases.py."""
import pytest
import torch

from tests import res_block_cases as rc
from tests.pool_helpers import NAN_VALUES, TIE_VALUES, U, fixture_cfg, fixture_weights, load_fixture, make_index, make_values, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _raw(c, u=None, s=None, x=None, g=None, want_dh=True):
    """out, mask, dx, dh of the two row kernels on a case's tensors."""
    from guassianhand_amd import res_block as R
    from guassianhand_amd._call import rows
    tu, ts = rc.tables(c)
    u, s = (tu if u is None else u).contiguous(), (ts if s is None else s).contiguous()
    x, g = rows(c.x if x is None else x), rows(c.g if g is None else g)
    W0, Ws = c.W0[:, :c.Cin], c.Ws[:, :c.Cin]
    out, mask = R._launch_forward(x, u, s, c.row_of, W0, Ws, c.W1)
    dx, dh = R._launch_backward(g, x, mask, W0, Ws, c.W1, want_dh)
    return dict(out=out, mask=mask, dx=dx, dh=dh)


def _bits(mask, H):
    """(T,H) bool from the (T,H/32) mask words."""
    sh = torch.arange(32, device=mask.device)
    return ((mask.unsqueeze(2) >> sh) & 1).bool().reshape(mask.shape[0], H)


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.ROW_CASES, ids=rc.case_id)
def test_row_kernels_against_float64_and_the_unfolded_block(dev, case):
    c = rc.make_rows(case, dev)
    mh, mx = rc.relu_margin(c)
    assert mh > rc.GUARD and mx > rc.GUARD, (mh, mx)            # no ReLU argument near its kink: a flip is not rounding
    from guassianhand_amd import res_block as R
    u, s = rc.tables(c)
    assert R._kernel_ok(c.x, u, s, c.row_of, c.W0[:, :c.Cin], c.Ws[:, :c.Cin], c.W1)
    f64, t32, ker = rc.run_rows(c, "f64"), rc.run_rows(c, "torch32"), rc.run_rows(c, "fused")
    rc.three_way(ker, t32, f64, tag=rc.case_id(case))
    # the mask is the sign of the float64 h (the margin above is far beyond float32 rounding)
    h64 = rc.tables(c, torch.float64)[0].index_select(0, rc._rows_index(c)) + torch.relu(c.x.double()) @ c.W0.double()[:, :c.Cin].t()
    assert torch.equal(_bits(_raw(c)["mask"], c.H), h64 > 0)


def test_zero_w1_ignores_u_and_a_zero_cotangent_gives_zero_gradients(dev):
    case = (129, 128, 1, "plan", True, 64)
    c = rc.make_rows(case, dev, w1_scale=0.0)
    assert not c.W1.any()
    u, s = rc.tables(c)
    a, b = _raw(c), _raw(c, u=torch.randn_like(u))
    assert torch.equal(a["out"], b["out"]) and not torch.equal(a["mask"], b["mask"])
    assert not a["dh"].any() and torch.equal(a["dx"], b["dx"])
    want = c.g.double() @ c.Ws.double()[:, :c.Cin]                # dx = Ws^T g
    t32 = c.g @ c.Ws[:, :c.Cin]
    rc.three_way(dict(dx=a["dx"]), dict(dx=t32), dict(dx=want), fields=("dx",), tag="W1 = 0")
    c = rc.make_rows(case, dev)
    c.g = torch.zeros_like(c.g)
    z = rc.run_rows(c, "fused")
    assert all(not z[k].any() for k in ("dx", "du", "ds"))


@pytest.mark.parametrize("H", [32, 128])
def test_negative_rows_leave_h_at_the_table_row(dev, H):
    c = rc.make_rows((130, H, 1, "plan", False, 0), dev)
    c.x = -c.x.abs()
    u, s = rc.tables(c)
    r = _raw(c)
    assert torch.equal(_bits(r["mask"], H), u.index_select(0, c.row_of.long()) > 0)     # h = u[r] bit for bit
    assert torch.equal(r["dx"], rc.run_rows(c, "fused")["dx"])
    want = c.g.double() @ c.Ws.double()[:, :c.Cin]                                       # x < 0 everywhere: dx = Ws^T g
    rc.three_way(dict(dx=r["dx"]), dict(dx=c.g @ c.Ws[:, :c.Cin]), dict(dx=want), fields=("dx",), tag=f"negative x, H={H}")


@pytest.mark.parametrize("case", [(257, 128, 1, "plan", False, 8), (257, 32, 2, "plan", True, 0)], ids=rc.case_id)
def test_a_row_does_not_depend_on_its_neighbours_or_its_stride(dev, case):
    c = rc.make_rows(case, dev)
    full = _raw(c)
    p = 70
    one = rc.make_rows(case, dev)
    wide = torch.zeros(1, c.Cin + 13, device=dev)
    wide[:, 5:5 + c.Cin] = c.x[p]
    gw = torch.zeros(1, c.H + 4, device=dev)
    gw[:, 4:] = c.g[p]
    one.T, one.x, one.g, one.row_of = 1, wide[:, 5:5 + c.Cin], gw[:, 4:], c.row_of[p:p + 1].contiguous()
    alone = _raw(one)
    for k in ("out", "mask", "dx", "dh"):
        assert torch.equal(alone[k][0], full[k][p]), k
    tail = rc.make_rows(case, dev)                                # the same row as the last of a 33-row call: a tail tile
    tail.T, tail.x, tail.g, tail.row_of = 33, c.x[p - 32:p + 1], c.g[p - 32:p + 1], c.row_of[p - 32:p + 1].contiguous()
    last = _raw(tail)
    for k in ("out", "mask", "dx", "dh"):
        assert torch.equal(last[k][32], full[k][p]), k


def test_every_kernel_is_bitwise_repeatable(dev):
    from guassianhand_amd import res_block as R
    from guassianhand_amd.pool import PoolPlan
    c = rc.make_rows((257, 128, 2, "plan", True, 297), dev)
    a, b = _raw(c), _raw(c)
    assert all(torch.equal(a[k], b[k]) for k in a)
    ra, rb = rc.run_rows(c, "fused"), rc.run_rows(c, "fused")
    assert all(torch.equal(ra[k], rb[k]) for k in ra)
    index = make_index("ladder", 1000, 20, torch.int32, True)      # cell 12 holds 300 points
    x = make_values("normal", index, 20, 128).to(dev)
    plan = PoolPlan(index.to(dev), 20)
    assert int(plan.counts()[12]) == 300
    assert torch.equal(R._cell_sum(x, plan, True), R._cell_sum(x, plan, True))
    (m1, a1), (m2, a2) = R._launch_cell_max(x, plan), R._launch_cell_max(x, plan)
    assert torch.equal(m1, m2) and torch.equal(a1, a2)


# ---- the cell kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("values", TIE_VALUES + ("inf",) + NAN_VALUES)
def test_cell_max_is_bit_equal_to_the_restatement(dev, values, C):
    from guassianhand_amd import pool, res_block as R
    index = make_index("ladder", 1000, 20, torch.int64 if C == 32 else torch.int32, True)        # cell 0 is empty
    x = make_values(values, index, 20, C)
    want, arg = pool._cell_max(x, pool.PoolPlan(index, 20))
    plan = pool.PoolPlan(index.to(dev), 20)
    m, argmax = R._launch_cell_max(x.to(dev), plan)
    assert torch.equal(m[:20].cpu(), want) and torch.equal(argmax.cpu().long(), arg) and not m[20].any()
    assert torch.equal(m.cpu().view(torch.int32)[:20], want.view(torch.int32))                   # the sign of a zero included
    assert (arg[0] == 1000).all() and not want[0].any()
    # backward against index_put in float64
    xg = x.to(dev).nan_to_num(0.0, 0.0, 0.0).requires_grad_(True)
    gm = torch.randn(21, C, device=dev)
    mg = R.cell_max(xg, plan)
    mg.backward(gm)
    a = R._launch_cell_max(xg.detach(), plan)[1].long()
    hit = a < 1000
    exp = torch.zeros(1000, C, dtype=torch.float64, device=dev)
    exp.index_put_((a[hit], torch.arange(C, device=dev).expand(20, C)[hit]), gm[:20][hit].double())
    assert torch.equal(xg.grad.double(), exp)


@pytest.mark.parametrize("tail", [False, True])
def test_cell_sum_is_within_the_bound_of_a_float32_sum(dev, tail):
    from guassianhand_amd import res_block as R
    from guassianhand_amd.pool import PoolPlan
    index = make_index("ladder", 1000, 20, torch.int32, True)
    x = make_values("normal", index, 20, 96)
    wide = torch.zeros(1000, 101, device=dev)
    wide[:, 2:98] = x.to(dev)
    plan = PoolPlan(index.to(dev), 20)
    got = R._cell_sum(wide[:, 2:98], plan, tail).cpu().double()
    key = torch.where((index >= 0) & (index < 20), index, torch.full_like(index, 20)).long()
    exact = torch.zeros(21, 96, dtype=torch.float64).index_add_(0, key, x.double())[:20 + tail]
    absum = torch.zeros(21, 96, dtype=torch.float64).index_add_(0, key, x.double().abs())[:20 + tail]
    n = torch.bincount(key, minlength=21)[:20 + tail].double().unsqueeze(1)
    bound = n * U * absum + U * exact.abs()                        # tests/pool_helpers.py
    err = (got - exact).abs()
    print(f"cell_sum tail={tail}: max err {float(err.max()):.3e}, worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert got.shape == exact.shape and (err <= bound).all() and not got[0].any()


# ---- the encoder -------------------------------------------------------------------------------------------------------------------
# The input gradients of two float32 paths agree to rounding only while both take float64's branch at every ReLU and every cell
# maximum. Among some 2.5 million such decisions per forward, one falls within float32 rounding of its kink at roughly one seed in
# eight, in either path (measured on an MI355X over the seeds 11 .. 18 and the eight configurations below: the torch path left
# float64's branches at the seeds 11, 12, 13 and 15, the folded path at 12, 14, 16 and 18, each time in one configuration, with a
# rel-L2 of 8e-5 .. 6e-3 where it is 3e-7 .. 8e-7 otherwise). Such an event measures the inputs, not a path, so the inputs are drawn
# from a seed at which neither path meets one, and the test asserts that of the yardstick too (torch against float64).
ENCODER_SEED = 17


def _encoder_inputs(dev, rows_input, T=2000, seed=None):
    gen = torch.Generator().manual_seed(ENCODER_SEED if seed is None else seed)
    uv = 2.2 * torch.rand(1, T, 2, generator=gen) - 1.1                  # both clamp edges; 64 cells, some crowded
    uv[0, :150] = 0.3 + 0.01 * torch.rand(150, 2, generator=gen)
    code = 2 * torch.rand(1, T, 33, generator=gen) - 1
    if rows_input:
        return uv.to(dev), code.to(dev)
    return torch.cat([uv, code], dim=2).to(dev), None


@pytest.mark.parametrize("rows_input", [False, True], ids=["tensor", "PointRows"])
@pytest.mark.parametrize("H", [32, 128])
@pytest.mark.parametrize("kind", ["max", "mean"])
def test_folded_encoder_against_the_torch_blocks(dev, kind, H, rows_input):
    from guassianhand_amd import pool
    from guassianhand_amd.cond import PointRows
    cin = 2 * (2 + 2 * 4) + 33 if rows_input else 35
    cfg = dict(input_channels=cin, c_dim=H, hidden_dim=H, scatter_type=kind, plane_size=8, n_blocks=5, radius=1.0)
    ref = rc.encoder(cfg, seed=1, device=dev)
    for q in ref.parameters():
        q.requires_grad_(False)
    a, code = _encoder_inputs(dev, rows_input)
    cot = torch.randn(1, H, 8, 8, generator=torch.Generator().manual_seed(0)).to(dev)

    def run(model, blocks, dtype=torch.float32, ops=None):
        if rows_input:
            leaf = code.to(dtype).clone().requires_grad_(True)
            p = PointRows(uv=a.to(dtype), code=leaf)
        else:
            leaf = a.to(dtype).clone().requires_grad_(True)
            p = leaf
        plane = pool.pointnet_forward(model, p, ops=ops, blocks=blocks)
        plane.backward(cot.to(dtype))
        return plane.detach(), leaf.grad

    uvs = a if rows_input else a[..., :2]
    plan = pool.PoolPlan(pool.cell_index(uvs, 1.0, 8)[0], 64)
    n_max = int(plan.counts().max())
    assert n_max >= 150
    import copy
    pf, gf = run(ref, "folded")
    pt, gt = run(ref, "torch")
    p64, g64 = run(copy.deepcopy(ref).double(), "torch", torch.float64, ops="torch")
    rc.three_way(dict(plane=pf), dict(plane=pt), dict(plane=p64), fields=("plane",), tag=f"{kind} H={H}")
    tol = 2 * 5 * n_max * U
    d, d_t = rel_l2(gf, gt), rel_l2(gt, g64)
    print(f"{kind} H={H} input gradient: folded vs torch rel-L2 {d:.3e} (bound {tol:.3e}); torch vs float64 {d_t:.3e}")
    assert d_t <= tol, "the float32 yardstick left float64's branches at these inputs: they test nothing"
    assert d <= tol


def test_the_fixture_runs_through_the_fallback(dev):
    from guassianhand_amd.pool import LocalPoolPointnet
    fx = load_fixture()
    m = LocalPoolPointnet(fixture_cfg(fx, "max"), blocks="folded")                   # H = 16: out of the kernels' domain
    m.load_state_dict(fixture_weights(fx))
    p = fx["p"].to(dev).requires_grad_(True)
    plane = m.to(dev)(p)
    plane.backward(fx["cot"].to(dev))
    d = float((plane.detach().cpu() - fx["max_plane"]).abs().max())
    print(f"fixture through the fallback: max |plane - fixture| {d:.3e}, grad_p rel-L2 {rel_l2(p.grad, fx['max_grad_p']):.3e}")
    assert d <= 64 * U * float(fx["max_plane"].abs().max()) and m.fc_pos.weight.grad is not None


# ---- fallbacks and refusal ---------------------------------------------------------------------------------------------------------
def test_fallbacks_do_not_raise_and_trainable_blocks_get_their_gradients(dev):
    from guassianhand_amd import pool, res_block as R
    gen = torch.Generator().manual_seed(4)
    block = pool.ResnetBlockFC(64, 32).to(dev)
    torch.nn.init.normal_(block.fc_1.weight, std=0.2)
    idx = torch.randint(0, 5, (100,), generator=gen).to(dev)
    plan = pool.PoolPlan(idx, 5)
    net = torch.randn(100, 32, generator=gen).to(dev).requires_grad_(True)
    m = R.cell_max(net, plan)
    out = R.folded_block(block, net, m, R.row_index(plan), plan=plan)               # parameters require a gradient: the restatement
    assert "ResRows" not in type(out.grad_fn).__name__
    out.sum().backward()
    assert all(q.grad is not None and bool(q.grad.any()) for q in block.parameters()) and net.grad is not None
    want = block(pool.pool_cat(net.detach(), plan, "max"))
    assert torch.allclose(out.detach(), want.detach(), rtol=0, atol=64 * U * float(want.detach().abs().max()))
    for q in block.parameters():
        q.requires_grad_(False)
    out = R.folded_block(block, net, R.cell_max(net, plan), R.row_index(plan), plan=plan)
    assert "ResRows" in type(out.grad_fn).__name__
    assert torch.allclose(out.detach(), want.detach(), rtol=0, atol=64 * U * float(want.detach().abs().max()))
    b64 = pool.ResnetBlockFC(64, 32).to(dev).double()
    R.folded_block(b64, net.detach().double(), R.cell_max(net.detach().double(), plan), R.row_index(plan), plan=plan)
    b48 = pool.ResnetBlockFC(96, 48).to(dev)
    n48 = torch.randn(100, 48, device=dev)
    got = R.folded_block(b48, n48, R.cell_max(n48, plan), R.row_index(plan), plan=plan)
    assert got.shape == (100, 48)


def test_the_entry_point_refuses_what_is_outside_its_domain(dev):
    from guassianhand_amd import _abi
    from guassianhand_amd._call import lib, ptr, stream
    L = lib()
    t = torch.zeros(64, 512, device=dev)
    i32 = torch.zeros(64, dtype=torch.int32, device=dev)

    def fwd(Cin, H, R):
        return L.gh_res_forward(ptr(t), 512, 64, Cin, H, ptr(t), ptr(t), R, ptr(i32), ptr(t), 512, ptr(t), 512, ptr(t), ptr(t), 512, None, stream(dev))
    assert fwd(48, 48, 1) == _abi.GH_ERR_INVALID_ARG and fwd(96, 32, 1) == _abi.GH_ERR_INVALID_ARG and fwd(32, 32, 0) == _abi.GH_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not t.any()                                            # refused before any launch: nothing was written


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_are_graph_capturable(dev):
    c = rc.make_rows((257, 128, 1, "plan", False, 8), dev)
    eager = rc.run_rows(c, "fused")
    from guassianhand_amd import res_block as R
    u, s = (t.detach().requires_grad_(True) for t in rc.tables(c))
    x = c.x.detach().clone().requires_grad_(True)

    def step():
        out = R.res_rows(x, u, s, c.row_of, c.W0[:, :c.Cin], c.Ws[:, :c.Cin], c.W1, plan=c.plan)
        return [out] + list(torch.autograd.grad(out, (x, u, s), c.g))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, o in zip(rc.FIELDS, outs):
            assert torch.equal(o, eager[k]), k
