"""guassianhand_amd.pool on CPU tensors — the plain-torch restatement the GPU tests compare against — checked against
tests/golden/pointnet_fixture.npz (the reference's LocalPoolPointnet run on the CPU, tests/golden/make_pointnet_fixture.py), the
torch_scatter drop-ins, the encoder's state-dict keys, and the C-ABI surface of include/gh_pool.h (argument checks only, nothing
is launched). The rounding bound is derived in tests/pool_helpers.py; where two float32 results are compared with each other
(restatement against fixture) each is within the bound of the exact value, so their distance is within twice the bound."""
import ctypes as C
import os
import re

import pytest
import torch

from guassianhand_amd import _abi, pool
from guassianhand_amd.pool import LocalPoolPointnet, PoolPlan, plane_mean, pool_cat, pool_local, scatter_max, scatter_mean
from tests.helpers import header_symbols
from tests.pool_helpers import U, assert_within, fixture_cfg, fixture_weights, load_fixture, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("max", "mean")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture()
def one_thread():
    """The fixture's GEMMs ran on one thread (tests/cpu_numerics.py: other thread counts split some sums differently)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _plan(fx, kind="max"):
    return PoolPlan(fx[f"{kind}_index"], int(fx["dims"][4]) ** 2)


def test_plan_groups_points_by_cell_in_ascending_order(fx):
    plan = _plan(fx)
    idx = fx["max_index"]
    cs, order = plan.cell_start.long(), plan.order.long()
    assert cs[0] == 0 and cs[-1] == idx.numel() and sorted(order.tolist()) == list(range(idx.numel()))
    for c in range(plan.n_cells):
        pts = order[cs[c]:cs[c + 1]]
        assert (idx[pts] == c).all() and (pts[1:] > pts[:-1]).all()
    plan.check()
    counts = plan.counts()
    assert (counts == 0).any() and (counts == 1).any() and counts.max() >= 200        # what the fixture was built to contain


def test_cell_index_is_the_reference_index(fx):
    for kind in KINDS:
        got = pool.cell_index(fx["p"], float(fx["radius"]), int(fx["dims"][4]))
        assert torch.equal(got[0], fx[f"{kind}_index"])
    uv = fx["p"][0, :, :2]
    assert (uv[:, 0] >= 1).any() and (uv[:, 0] <= -1).any() and (uv[:, 1] >= 1).any() and (uv[:, 1] <= -1).any()   # both clamp edges


@pytest.mark.parametrize("kind", KINDS)
def test_encoder_reproduces_every_pooled_tensor_and_the_plane(fx, kind, one_thread):
    m = LocalPoolPointnet(fixture_cfg(fx, kind))
    m.load_state_dict(fixture_weights(fx))
    m.pool_record = []
    p = fx["p"].clone().requires_grad_(True)
    plane = m(p)
    idx = fx[f"{kind}_index"]
    assert len(m.pool_record) == int(fx["dims"][5]) - 1
    for k, got in enumerate(m.pool_record, 1):
        assert torch.equal(got, fx[f"{kind}_pooled{k}_cells"][idx]), f"pooled tensor of block {k}"
    # the plane: a float32 mean per cell on both sides -> twice the bound of one float32 sum around the float64 value
    plan = _plan(fx, kind)
    c = fx[f"{kind}_op_plane_in"]
    exact = pool._plane_mean_ref(c, plan, acc=torch.float64)
    bound = plan.counts().double() * U * pool._plane_mean_ref(c.abs(), plan, acc=torch.float64) + U * exact.abs()
    assert_within(pool._plane_mean_ref(c, plan), exact, bound, f"{kind} plane restatement vs float64")
    assert_within(fx[f"{kind}_plane"].reshape(exact.shape), exact, bound, f"{kind} fixture plane vs float64")
    assert_within(plane.reshape(exact.shape), fx[f"{kind}_plane"].reshape(exact.shape), bound, f"{kind} encoder plane vs fixture", slack=2.0)
    # end to end gradients. Both sides run the same GEMMs on the same values; they can differ only in the order of the float32
    # sums of the five pooling calls' backwards, each within n * u of its sum of |terms|. To first order, and without the
    # amplification a cancelling sum could add, that is 5 ops * n_max * u per side; two sides.
    plane.backward(fx["cot"])
    tol = 2 * 5 * int(plan.counts().max()) * U
    for name, got in (("grad_p", p.grad), ("grad_fc_pos_w", m.fc_pos.weight.grad)):
        d = rel_l2(got, fx[f"{kind}_{name}"])
        print(f"{kind} {name}: rel-L2 to the fixture {d:.3e} (bound {tol:.3e})")
        assert d <= tol, (kind, name, d)


@pytest.mark.parametrize("kind", KINDS)
def test_single_ops_and_their_gradients_match_the_fixture(fx, kind):
    plan = _plan(fx, kind)
    cnt_pt = plan.counts().double()[fx[f"{kind}_index"]]
    x = fx[f"{kind}_op_pool_in"].clone().requires_grad_(True)
    out = pool_local(x, plan, kind)
    assert torch.equal(out.detach(), fx[f"{kind}_pooled1_cells"][fx[f"{kind}_index"]])
    g = fx["op_pool_cot"]
    out.backward(g)
    x64 = x.detach().double().requires_grad_(True)
    pool._pool_local_ref(x64, plan, kind).backward(g.double())
    xa = x.detach().double().requires_grad_(True)
    pool._pool_local_ref(xa, plan, kind).backward(g.double().abs())       # sum|terms| (/ count for the mean) where the sum lands
    bound = cnt_pt.unsqueeze(1) * U * xa.grad + (U * x64.grad.abs() if kind == "mean" else 0.0)
    assert_within(x.grad, x64.grad, bound, f"{kind} pool backward restatement vs float64")
    assert_within(fx[f"{kind}_op_pool_grad"], x64.grad, bound, f"{kind} pool backward fixture vs float64")
    if kind == "max":
        assert torch.equal(x.grad == 0, x64.grad == 0)                     # nothing lands beside the argmax rows
    # plane: grad_c = grad_plane / count, one term and one division
    c = fx[f"{kind}_op_plane_in"].clone().requires_grad_(True)
    cot = fx["cot"].reshape(c.shape[1], plan.n_cells)
    plane_mean(c, plan).backward(cot)
    c64 = c.detach().double().requires_grad_(True)
    pool._plane_mean_ref(c64, plan).backward(cot.double())
    bound = 2 * U * c64.grad.abs()
    assert_within(c.grad, c64.grad, bound, f"{kind} plane backward restatement vs float64")
    assert_within(fx[f"{kind}_op_plane_grad"], c64.grad, bound, f"{kind} plane backward fixture vs float64")


def test_scatter_max_matches_the_fixture_bit_for_bit(fx):
    x = fx["max_op_pool_in"]
    T = x.shape[0]
    out, arg = scatter_max(x.t().unsqueeze(0), fx["max_index"].reshape(1, 1, T), dim_size=int(fx["dims"][4]) ** 2)
    assert torch.equal(out[0], fx["max_scatter_out"]) and torch.equal(arg[0], fx["max_scatter_arg"])
    assert arg.dtype == torch.int64 and out.shape == (1, x.shape[1], 64)
    empty = PoolPlan(fx["max_index"], 64).counts() == 0
    assert empty.any() and (out[0][:, empty] == 0).all() and (arg[0][:, empty] == T).all()


def test_duplicate_rows_tie_to_the_lower_index():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(12, 5, generator=g)
    idx = torch.tensor([0, 1, 1, 0, 2, 1, 0, 2, 1, 1, 0, 1])
    top = x[idx == 1].max(dim=0).values + 1.0
    x[2], x[8] = top, top                                                  # two identical rows hold every channel's maximum of cell 1
    x = x.requires_grad_(True)
    plan = PoolPlan(idx, 4)                                                # cell 3 is empty
    out = pool_local(x, plan, "max")
    assert torch.equal(out[idx == 1], top.expand(int((idx == 1).sum()), 5))
    assert (pool.pool_argmax(x, plan)[1] == 2).all() and (pool.pool_argmax(x, plan)[3] == 12).all()
    cot = torch.randn(12, 5, generator=g)
    out.backward(cot)
    want = cot[[1, 2, 5, 8, 9, 11]].double().sum(0)
    assert torch.allclose(x.grad[2].double(), want, rtol=0, atol=6 * U * cot[[1, 2, 5, 8, 9, 11]].abs().double().sum(0).max().item())
    assert (x.grad[8] == 0).all() and (x.grad[[1, 5, 9, 11]] == 0).all()


def test_pool_cat_is_cat_of_net_and_pooled():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(40, 6, generator=g)
    plan = PoolPlan(torch.randint(0, 7, (40,), generator=g, dtype=torch.int32), 9)
    for kind in KINDS:
        cat = pool_cat(x, plan, kind)
        assert torch.equal(cat[:, :6], x) and torch.equal(cat[:, 6:], pool_local(x, plan, kind))
    buf = torch.zeros(40, 12)
    buf[:, :6] = x
    r = pool_local(buf[:, :6], plan, "max", out=buf[:, 6:])
    assert r.data_ptr() == buf[:, 6:].data_ptr() and torch.equal(buf, pool_cat(x, plan, "max"))
    with pytest.raises(RuntimeError):
        pool_local(x.clone().requires_grad_(True), plan, "max", out=buf[:, 6:])
    with pytest.raises(ValueError):
        pool_local(x, plan, "sum")


def test_out_of_range_indices_are_skipped_and_reported():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(30, 4, generator=g)
    idx = torch.randint(0, 5, (30,), generator=g)
    good = PoolPlan(idx, 5)
    bad_idx = idx.clone()
    bad_idx[[3, 17]] = torch.tensor([5, -1])
    bad = PoolPlan(bad_idx, 5)
    good.check()
    with pytest.raises(IndexError):
        bad.check()
    keep = torch.ones(30, dtype=torch.bool)
    keep[[3, 17]] = False
    sub = PoolPlan(idx[keep], 5)
    for kind in KINDS:
        out = pool_local(x, bad, kind)
        assert (out[[3, 17]] == 0).all() and torch.equal(out[keep], pool_local(x[keep], sub, kind))
    assert torch.equal(plane_mean(x, bad), plane_mean(x[keep], sub))


def test_scatter_drop_ins_cover_the_reference_call_forms():
    g = torch.Generator().manual_seed(3)
    B, Cc, T, n = 2, 3, 25, 6
    src = torch.randn(B, Cc, T, generator=g)
    index = torch.randint(0, n - 1, (B, 1, T), generator=g)               # cell n-1 stays empty
    out, arg = scatter_max(src, index, dim_size=n)
    mean = scatter_mean(src, index, dim_size=n)
    for b in range(B):
        for c in range(n):
            pts = torch.nonzero(index[b, 0] == c).flatten()
            if pts.numel() == 0:
                assert (out[b, :, c] == 0).all() and (arg[b, :, c] == T).all() and (mean[b, :, c] == 0).all()
                continue
            assert torch.equal(out[b, :, c], src[b][:, pts].max(dim=1).values)
            assert torch.equal(src[b].gather(1, arg[b, :, c:c + 1]).flatten(), out[b, :, c])
            assert torch.allclose(mean[b, :, c], src[b][:, pts].mean(dim=1), rtol=0, atol=1e-6)
    fea = torch.zeros(B, Cc, n)                                            # generate_plane_features' form
    ret = scatter_mean(src, index, out=fea)
    assert ret is fea and torch.equal(fea, mean)
    ret = scatter_mean(src, index, out=fea)                                # accumulated into, not overwritten
    assert torch.equal(fea, mean + mean)
    assert torch.equal(scatter_max(src, index, dim=2, dim_size=n)[0], out)
    for call in (lambda: scatter_max(src, index, dim=1, dim_size=n), lambda: scatter_max(src, index),
                 lambda: scatter_max(src[0], index[0], dim_size=n), lambda: scatter_mean(src, index.expand(B, Cc, T), dim_size=n),
                 lambda: scatter_mean(src, index, dim=0, dim_size=n), lambda: scatter_max(src, index, out=fea)):
        with pytest.raises(NotImplementedError):
            call()


def test_encoder_has_the_reference_state_dict_keys(fx):
    cfg = fixture_cfg(fx, "max")
    m = LocalPoolPointnet(cfg)
    want = ["fc_pos.weight", "fc_pos.bias", "fc_c.weight", "fc_c.bias"]
    for i in range(cfg["n_blocks"]):
        want += [f"blocks.{i}.fc_0.weight", f"blocks.{i}.fc_0.bias", f"blocks.{i}.fc_1.weight", f"blocks.{i}.fc_1.bias",
                 f"blocks.{i}.shortcut.weight"]
    assert sorted(m.state_dict()) == sorted(want) == sorted(fixture_weights(fx))
    missing, unexpected = m.load_state_dict(fixture_weights(fx), strict=True)
    assert not missing and not unexpected
    assert torch.equal(m.blocks[2].shortcut.weight, fx["w.blocks.2.shortcut.weight"])
    assert LocalPoolPointnet().cfg.plane_size == 32 and LocalPoolPointnet(hidden_dim=8).fc_pos.out_features == 16
    with pytest.raises(ValueError):
        LocalPoolPointnet(scatter_type="sum")
    base = type("LocalPoolPointnet", (torch.nn.Module,), {"forward": lambda self, p: None})
    cls = pool.fused_pointnet_cls(base)
    assert issubclass(cls, base) and cls.__name__ == "LocalPoolPointnet" and cls.forward is not base.forward


# ---- C-ABI (include/gh_pool.h) ----------------------------------------------------------------------------------------------------
def test_pool_header_mirror_and_library_agree(gh_lib_path):
    h = open(os.path.join(ROOT, "include", "gh_pool.h")).read()
    assert header_symbols("gh_pool.h") == sorted(_abi.POOL_SYMBOLS)
    assert not set(_abi.POOL_SYMBOLS) & (set(_abi.EXPORTED_SYMBOLS) | set(_abi.METRICS_SYMBOLS))
    for name in ("GH_POOL_MAX", "GH_POOL_MEAN", "GH_POOL_MAX_CELLS"):
        assert getattr(_abi, name) == int(re.search(rf"#define {name} (\d+)", h).group(1)), name
    L = C.CDLL(gh_lib_path)
    for s in _abi.POOL_SYMBOLS:
        getattr(L, s)


def test_pool_arguments_are_validated_before_any_launch(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    _abi.declare_pool(L)
    INV, SMALL, UNSUP = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_WORKSPACE_SMALL, _abi.GH_ERR_UNSUPPORTED
    T, Cc, n = 1000, 128, 1024
    nbytes = L.gh_pool_plan_workspace(T, n)
    assert nbytes > 0 and nbytes % 256 == 0 and L.gh_pool_plan_workspace(98562, n) > nbytes
    assert L.gh_pool_plan_workspace(0, n) == 0 and L.gh_pool_plan_workspace(T, 0) == 0
    A, B, D, E, F = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))         # far apart; never dereferenced
    plan = lambda index=A, T=T, n=n, cs=B, order=D, flag=E, ws=F, nb=nbytes: L.gh_pool_plan(index, 1, T, n, cs, order, flag, ws, nb, None)
    assert plan(index=None) == INV and plan(cs=None) == INV and plan(order=None) == INV and plan(flag=None) == INV
    assert plan(ws=None) == INV and plan(T=0) == INV and plan(n=0) == INV and plan(n=-3) == INV
    assert plan(n=_abi.GH_POOL_MAX_CELLS + 1) == UNSUP
    assert plan(nb=nbytes - 1) == SMALL and plan(nb=0) == SMALL
    assert plan(index=C.c_void_p((1 << 24) + 4)) == INV                     # int64 alignment

    def fwd(x=A, xs=Cc, T=T, Cc=Cc, n=n, cs=B, order=D, red=0, out=E, os_=Cc, col=0, arg=F):
        return L.gh_pool_forward(x, xs, T, Cc, n, cs, order, red, out, os_, col, arg, None)
    assert fwd(x=None) == INV and fwd(out=None) == INV and fwd(cs=None) == INV and fwd(order=None) == INV
    assert fwd(arg=None) == INV                                            # max needs argmax
    assert fwd(Cc=0) == INV and fwd(Cc=-1) == INV and fwd(n=0) == INV and fwd(T=0) == INV and fwd(red=2) == INV
    assert fwd(xs=Cc - 1) == INV and fwd(os_=Cc - 1) == INV and fwd(col=1) == INV and fwd(col=-1) == INV
    assert fwd(n=_abi.GH_POOL_MAX_CELLS + 1) == UNSUP
    base = 1 << 24
    assert fwd(out=A) == INV                                               # in place
    assert fwd(xs=2 * Cc, out=A, os_=2 * Cc, col=Cc - 1) == INV            # the halves of a cat buffer, one column too far left
    assert fwd(xs=2 * Cc, out=C.c_void_p(base + 4 * (2 * Cc * 3 + 5)), os_=2 * Cc, col=0) == INV     # shifted rows, columns still collide
    assert fwd(xs=Cc, out=C.c_void_p(base + 4 * Cc * 10), os_=2 * Cc) == INV                          # ranges overlap, strides differ

    def bwd(g=A, gs=Cc, col=0, T=T, Cc=Cc, n=n, cs=B, order=D, red=0, arg=F, gx=E, gxs=Cc, acc=0):
        return L.gh_pool_backward(g, gs, col, T, Cc, n, cs, order, red, arg, gx, gxs, acc, None)
    assert bwd(g=None) == INV and bwd(gx=None) == INV and bwd(arg=None) == INV and bwd(cs=None) == INV
    assert bwd(Cc=0) == INV and bwd(n=0) == INV and bwd(red=-1) == INV and bwd(gs=Cc - 1) == INV and bwd(gxs=1) == INV
    assert bwd(gx=A) == INV and bwd(gs=2 * Cc, col=Cc, gx=A, gxs=2 * Cc - 1) == INV

    pf = lambda x=A, xs=Cc, T=T, Cc=Cc, n=n, cs=B, order=D, plane=E: L.gh_plane_mean_forward(x, xs, T, Cc, n, cs, order, plane, None)
    assert pf(x=None) == INV and pf(plane=None) == INV and pf(order=None) == INV and pf(Cc=0) == INV and pf(n=0) == INV
    assert pf(xs=3) == INV and pf(plane=A) == INV and pf(plane=C.c_void_p(base + 4 * Cc * (T - 1))) == INV
    pb = lambda gp=A, T=T, Cc=Cc, n=n, cs=B, order=D, gx=E, gxs=Cc: L.gh_plane_mean_backward(gp, T, Cc, n, cs, order, gx, gxs, None)
    assert pb(gp=None) == INV and pb(gx=None) == INV and pb(cs=None) == INV and pb(Cc=0) == INV and pb(n=0) == INV
    assert pb(gxs=Cc - 1) == INV and pb(gx=A) == INV


# ---- the float64 loop of tests/pool_helpers.py against the restatement, on every case of the edge sweep ------------------------------
# tests/test_gpu_pool_edges.py compares the kernels with the same loop on the same cases: here the loop and the inputs are proven
# against the restatement (and the restatement against the loop) before a GPU sees them.
from tests.pool_helpers import (LADDER, NAN_VALUES, SWEEP, TIE_VALUES, assert_within_or_same_nonfinite, case_id, loop_pool,      # noqa: E402
                                permute_within_cells, plane_bounds, pool_bounds, sweep_case)


def test_the_sweep_holds_every_listed_size_and_the_ladder_is_exact():
    for axis, want in ((0, {1, 3, 255, 256, 257, 700, 3000}), (1, {1, 16, 63, 64, 65, 100, 130}),
                       (2, {1, 7, 8, 9, 1023, 1024, 1025, 2500, 8192})):
        assert want <= {c[axis] for c in SWEEP}, axis
    assert {c[3] for c in SWEEP} >= {"random", "own_cell", "all_in_first", "all_in_last", "ladder", "all_bad"}
    assert {c[4] for c in SWEEP} >= {"normal", "grid", "const_col", "dup_rows", "inf", *NAN_VALUES}
    for case in SWEEP:
        if case[3] != "ladder":
            continue
        s = sweep_case(case)
        assert s.max.counts[:len(LADDER)].tolist() == list(LADDER), case_id(case)
        pts = torch.nonzero(s.index == 12).flatten()                                     # the 300-point cell
        assert len(set((pts // 256).tolist())) >= 3, "a cell's points are spread over several 256-point blocks"
        if case[6]:
            bad = (s.index.long() < 0) | (s.index.long() >= s.n)
            assert bad[[0, 255, 256, 257, s.T - 1]].all() and len(set(s.index[bad].tolist())) == 3


def test_the_tie_patterns_of_the_sweep_do_tie():
    """What makes the bit-for-bit argmax comparisons a test of the tie rule. In a cell of k grid values (7 levels) the maximum is
    attained once with probability <= (k / 7) (6 / 7)^(k - 1), 4 % at k = 32: the cells of 32 points and more tie in nearly every
    channel. Identical rows tie in every channel of every cell of two points and more, constant columns in theirs."""
    seen = set()
    for case in SWEEP:
        if case[4] not in TIE_VALUES or case[3] in ("own_cell", "all_bad"):
            continue
        s = sweep_case(case)
        least = 32 if case[4] == "grid" else 2
        attained = (s.x.double() == s.max.pooled) & (s.max.count_pt > 0).unsqueeze(1)
        times = torch.zeros(s.n, s.C).index_add_(0, s.index.long().clamp(0, s.n - 1), attained.float())[s.max.counts >= least]
        if case[4] == "const_col":
            times = times[:, [0, s.C - 1]]
        if times.numel():
            seen.add(case[4])
            assert (times > 1).float().mean() >= 0.9, case_id(case)
            assert (s.max.argmax[s.max.counts >= least] < s.T).all()
    assert seen == set(TIE_VALUES)


@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_loop_yardstick_and_restatement_agree_on_the_sweep(case):
    s = sweep_case(case)
    plan = PoolPlan(s.index, s.n)
    assert torch.equal(plan.cell_start, s.max.cell_start) and torch.equal(plan.order, s.max.order)
    assert torch.equal(plan.counts().long(), s.max.counts)
    bad = bool(((s.index.long() < 0) | (s.index.long() >= s.n)).any())
    assert int(plan.flag) == int(bad)
    # maxima: bit for bit
    vals, arg = pool._cell_max(s.x, plan)
    assert torch.equal(arg, s.max.argmax)
    want = torch.where(arg == s.T, torch.zeros(()), s.x.gather(0, arg.clamp(max=s.T - 1)))
    assert torch.equal(vals, want) and not torch.isnan(vals).any()
    x = s.x.clone().requires_grad_(True)
    out = pool._pool_local_ref(x, plan, "max")
    assert torch.equal(out.detach(), s.max.pooled.float())
    out.backward(s.cot)
    _, bwd, _ = pool_bounds(s.max, "max")
    assert_within(x.grad, s.max.grad, bwd, "max backward, restatement vs loop")
    assert (x.grad[~s.max.lands] == 0).all()
    # means: float32 and float64 restatement, both within the bound of the loop
    fwd, bwd, _ = pool_bounds(s.mean, "mean")
    for acc in (None, torch.float64):
        x = s.x.clone().requires_grad_(True)
        out = pool._pool_local_ref(x, plan, "mean", acc=acc)
        assert_within_or_same_nonfinite(out, s.mean.pooled, fwd, f"mean forward, restatement ({acc}) vs loop")
        out.backward(s.cot.to(out.dtype))
        assert_within_or_same_nonfinite(x.grad, s.mean.grad, bwd, f"mean backward, restatement ({acc}) vs loop")
        pf, pb = plane_bounds(s.mean)
        c = s.x.clone().requires_grad_(True)
        plane = pool._plane_mean_ref(c, plan, acc=acc)
        assert plane.shape == (s.C, s.n)
        assert_within_or_same_nonfinite(plane, s.mean.plane, pf, f"plane forward, restatement ({acc}) vs loop")
        plane.backward(s.plane_cot.to(plane.dtype))
        assert_within_or_same_nonfinite(c.grad, s.mean.plane_grad, pb, f"plane backward, restatement ({acc}) vs loop")


def test_a_nan_never_wins_a_maximum_and_a_cell_of_nans_is_empty():
    """The rule of include/gh_pool.h on a cell small enough to read: wherever the NaN sits the maximum is that of the other rows."""
    nan, inf = float("nan"), float("inf")
    idx = torch.tensor([0, 1, 0, 2, 0, 1, 7, 3, 3])                       # cell 4 is empty, point 6 has no cell
    #                   cell 0: rows 0, 2, 4        cell 1: rows 1, 5     cell 2: row 3      cell 3: rows 7, 8
    x = torch.tensor([[nan, 1.0, 5.0, nan], [nan, 2.0, -inf, nan], [3.0, nan, 5.0, nan], [nan, 4.0, nan, 0.0], [3.0, 0.0, nan, nan],
                      [nan, nan, -inf, 1.0], [nan, inf, nan, nan], [-inf, -inf, nan, 2.0], [-inf, nan, nan, 2.0]], requires_grad=True)
    plan = PoolPlan(idx, 5)
    arg = pool.pool_argmax(x, plan)
    assert arg.tolist() == [[2, 0, 0, 9], [9, 1, 1, 5], [9, 3, 9, 3], [7, 7, 9, 7], [9, 9, 9, 9]]
    out = pool_local(x, plan, "max")
    want = torch.tensor([[3.0, 1.0, 5.0, 0.0], [0.0, 2.0, -inf, 1.0], [3.0, 1.0, 5.0, 0.0], [0.0, 4.0, 0.0, 0.0], [3.0, 1.0, 5.0, 0.0],
                         [0.0, 2.0, -inf, 1.0], [0.0, 0.0, 0.0, 0.0], [-inf, -inf, 0.0, 2.0], [-inf, -inf, 0.0, 2.0]])
    assert torch.equal(out.detach(), want)
    out.backward(torch.ones(9, 4))
    grad = torch.zeros(9, 4)
    for c, row in enumerate(arg.tolist()):
        for ch, p in enumerate(row):
            if p < 9:
                grad[p, ch] = float((idx == c).sum())
    assert torch.equal(x.grad, grad)
    lp = loop_pool(x, idx, 5, "max", torch.ones(9, 4))
    assert torch.equal(lp.argmax, arg) and torch.equal(lp.pooled.float(), want) and torch.equal(lp.grad.float(), grad)
    vals, sarg = scatter_max(x.detach().t().unsqueeze(0), idx.reshape(1, 1, 9), dim_size=5)
    assert torch.equal(sarg[0].t(), arg) and not torch.isnan(vals).any()
    mean = pool_local(x.detach(), plan, "mean")                          # means propagate, inside the cell and nowhere else
    assert torch.isnan(mean[[0, 2, 4], 0]).all() and (mean[6] == 0).all() and (mean[[7, 8], 3] == 2.0).all()
    assert torch.equal(torch.isnan(mean[3]), torch.isnan(x.detach()[3]))
    assert (plane_mean(x.detach(), plan)[:, 4] == 0).all()


@pytest.mark.parametrize("case", [c for c in SWEEP if c[4] in NAN_VALUES], ids=case_id)
def test_the_maximum_does_not_depend_on_where_a_nan_sits_in_its_cell(case):
    s = sweep_case(case)
    plan = PoolPlan(s.index, s.n)
    assert torch.isnan(s.x).any()
    out, empty = pool_local(s.x, plan, "max"), pool.pool_argmax(s.x, plan) == s.T
    for seed in (1, 2):
        y = permute_within_cells(s.index, s.x, s.n, seed)
        assert not torch.equal(torch.isnan(y), torch.isnan(s.x)) or case[4] in ("nan_all", "nan_bad")
        assert torch.equal(pool_local(y, plan, "max"), out) and torch.equal(pool.pool_argmax(y, plan) == s.T, empty)
        lp = loop_pool(y, s.index, s.n, "max")
        assert torch.equal(lp.pooled, s.max.pooled) and torch.equal(lp.argmax, pool.pool_argmax(y, plan))
