"""guassianhand_amd.res_block on CPU tensors: the folded algebra against tests/golden/pointnet_fixture.npz (the reference's own
LocalPoolPointnet, T = 2000, H = 16) and against the unfolded statements in float64, the cell rows, the zero row of out-of-range
points, and the C-ABI surface of include/gh_res.h (argument checks only, nothing is launched)."""
import ctypes as C
import os
import re

import pytest
import torch

from guassianhand_amd import _abi, pool, res_block
from guassianhand_amd.pool import LocalPoolPointnet, PoolPlan
from tests import res_block_cases as rc
from tests.helpers import header_symbols
from tests.pool_helpers import NAN_VALUES, SWEEP, TIE_VALUES, U, case_id, fixture_cfg, fixture_weights, load_fixture, rel_l2, sweep_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("max", "mean")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture()
def one_thread():
    """The fixture's GEMMs ran on one thread (tests/cpu_numerics.py)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _fixture_encoder(fx, kind, dtype=torch.float32, **kw):
    m = LocalPoolPointnet(fixture_cfg(fx, kind), **kw)
    m.load_state_dict(fixture_weights(fx))
    return m.to(dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_folded_encoder_reproduces_the_reference_fixture(fx, kind, one_thread):
    """d32 <= 4 ref_err + d64: the folded float32 plane may be as far from the fixture as the fixture's own float32 error (d64, the
    exact algebra's distance to it) plus four times what the unfolded float32 path loses against its own float64 run."""
    want = fx[f"{kind}_plane"]
    folded = _fixture_encoder(fx, kind, blocks="folded")
    p = fx["p"].clone().requires_grad_(True)
    plane = folded(p)
    assert plane.shape == want.shape and plane.dtype == torch.float32
    d32 = float((plane.detach().double() - want.double()).abs().max())
    with torch.no_grad():
        d64 = float((_fixture_encoder(fx, kind, torch.float64, blocks="folded")(fx["p"].double()) - want.double()).abs().max())
        ref_err = float((_fixture_encoder(fx, kind)(fx["p"]).double() - _fixture_encoder(fx, kind, torch.float64)(fx["p"].double())).abs().max())
    print(f"{kind} plane: d32 {d32:.3e}  d64 {d64:.3e}  ref_err {ref_err:.3e}  max|plane| {float(want.abs().max()):.3e}")
    assert d32 <= 4 * ref_err + d64
    plane.backward(fx["cot"])
    tol = 2 * 5 * int(PoolPlan(fx[f"{kind}_index"], int(fx["dims"][4]) ** 2).counts().max()) * U      # test_pool_cpu.py's bound
    for name, got in (("grad_p", p.grad), ("grad_fc_pos_w", folded.fc_pos.weight.grad)):
        d = rel_l2(got, fx[f"{kind}_{name}"])
        print(f"{kind} {name}: rel-L2 to the fixture {d:.3e} (bound {tol:.3e})")
        assert d <= tol, (kind, name, d)


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("kind", KINDS)
def test_folded_equals_unfolded_in_float64(kind):
    cfg = dict(input_channels=5, c_dim=12, hidden_dim=8, scatter_type=kind, plane_size=4, n_blocks=5, radius=1.0)
    ref = rc.encoder(cfg, seed=3, dtype=torch.float64)
    fold = rc.encoder(cfg, seed=3, dtype=torch.float64, blocks="folded")
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), fold.state_dict().values()))
    assert float(ref.blocks[1].fc_1.weight.detach().abs().max()) > 0
    gen = torch.Generator().manual_seed(5)
    p0 = (1.3 * torch.rand(2, 300, 5, generator=gen, dtype=torch.float64) - 0.65)
    p0[0, :40, :2] = 0.9                                                   # a crowded cell; others stay empty
    cot = torch.randn(2, 12, 4, 4, generator=gen, dtype=torch.float64)
    grads = []
    for m in (ref, fold):
        p = p0.clone().requires_grad_(True)
        plane = m(p)
        plane.backward(cot)
        grads.append((plane.detach(), p.grad, {k: v.grad for k, v in m.named_parameters()}))
    (pr, gr, wr), (pf, gf, wf) = grads
    print(f"{kind}: plane {_rel(pf, pr):.2e}, grad_p {_rel(gf, gr):.2e}, parameters {max(_rel(wf[k], wr[k]) for k in wr):.2e}")
    assert _rel(pf, pr) <= 1e-12 and _rel(gf, gr) <= 1e-12
    for k in wr:
        assert wf[k] is not None and _rel(wf[k], wr[k]) <= 1e-12, k
    # block by block, on a plan with an empty cell and an out-of-range point
    idx = torch.randint(0, 5, (200,), generator=gen)
    idx[idx == 2] = 1
    idx[17] = 9
    plan = PoolPlan(idx, 5)
    row_of = res_block.row_index(plan)
    net = torch.randn(200, 8, generator=gen, dtype=torch.float64)
    x0 = torch.randn(200, 16, generator=gen, dtype=torch.float64)
    assert _rel(res_block.folded_block(ref.blocks[0], x0, None, None), ref.blocks[0](x0)) <= 1e-12
    for block in ref.blocks[1:]:
        m = res_block.cell_max(net, plan) if kind == "max" else res_block.cell_mean(net, plan)
        cat = pool.pool_cat(net, plan, kind)
        assert torch.equal(m[row_of.long()], cat[:, 8:])
        assert _rel(res_block.folded_block(block, net, m, row_of, plan=plan), block(cat)) <= 1e-12


@pytest.mark.parametrize("case", [c for c in SWEEP if c[4] in NAN_VALUES + TIE_VALUES + ("inf",) or c[3] in ("ladder", "all_bad")], ids=case_id)
def test_cell_max_is_pool_cell_max_with_a_zero_row(case):
    s = sweep_case(case)
    plan = PoolPlan(s.index, s.n)
    m = res_block.cell_max(s.x, plan)
    vals, arg = pool._cell_max(s.x, plan)
    assert m.shape == (s.n + 1, s.C) and torch.equal(m[:s.n], vals) and (m[s.n] == 0).all() and not torch.isnan(m).any()
    assert torch.equal(arg, s.max.argmax)
    assert torch.equal(m[res_block.row_index(plan).long()], s.max.pooled.float())          # the float64 loop's pooled rows
    x = s.x.clone().requires_grad_(True)
    res_block.cell_max(x, plan)[res_block.row_index(plan).long()].backward(s.cot)
    assert (x.grad[~s.max.lands] == 0).all()


def test_plane_linear_gives_exact_zeros_for_empty_cells():
    gen = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 6, (50,), generator=gen) * 2                    # the odd cells stay empty
    plan = PoolPlan(idx, 12)
    fc = torch.nn.Linear(8, 5)
    net = torch.randn(50, 8, generator=gen)
    plane = res_block.plane_linear(net, plan, fc)
    empty = plan.counts() == 0
    assert plane.shape == (5, 12) and empty.sum() >= 6 and (plane[:, empty] == 0).all() and (plane[:, ~empty] != 0).all()
    want = pool.plane_mean(fc(net.double().float()), plan)
    assert torch.allclose(plane, want, rtol=0, atol=64 * U * float(want.abs().max()))


def test_out_of_range_points_take_the_zero_row_and_are_still_reported():
    gen = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 5, (30,), generator=gen)
    idx[[3, 17]] = torch.tensor([5, -1])
    plan = PoolPlan(idx, 5)
    with pytest.raises(IndexError):
        plan.check()
    row_of = res_block.row_index(plan)
    assert row_of.dtype == torch.int32 and row_of[[3, 17]].tolist() == [5, 5] and torch.equal(row_of[idx.clamp(0, 4) == idx].long(), idx[idx.clamp(0, 4) == idx])
    block = pool.ResnetBlockFC(8, 4)
    torch.nn.init.normal_(block.fc_1.weight)
    net = torch.randn(30, 4, generator=gen)
    for kind in KINDS:
        m = res_block.cell_max(net, plan) if kind == "max" else res_block.cell_mean(net, plan)
        got = res_block.folded_block(block, net, m, row_of, plan=plan)
        want = block(pool.pool_cat(net, plan, kind))
        assert torch.allclose(got, want, rtol=0, atol=32 * U * float(want.abs().max()))
        assert torch.allclose(got[[3, 17]], block(torch.cat([net[[3, 17]], torch.zeros(2, 4)], dim=1)), rtol=0, atol=32 * U * float(want.abs().max()))


def test_pool_record_receives_the_cell_rows(fx):
    m = _fixture_encoder(fx, "max", blocks="folded")
    m.pool_record = []
    with torch.no_grad():
        m(fx["p"])
    n = int(fx["dims"][4]) ** 2
    assert len(m.pool_record) == int(fx["dims"][5]) - 1 and all(r.shape == (n, int(fx["dims"][2])) for r in m.pool_record)
    want = fx["max_pooled1_cells"]                                          # a maximum of block 0's rows: their rounding, nothing summed
    assert torch.allclose(m.pool_record[0], want, rtol=0, atol=64 * U * float(want.abs().max()))


@pytest.mark.parametrize("kind", KINDS)
def test_blocks_none_leaves_the_forward_as_it_was(fx, kind, one_thread):
    """The statements of pointnet_forward before `blocks` existed, restated here, give the same bits as blocks=None and "torch"."""
    m = _fixture_encoder(fx, kind)
    p = fx["p"]
    with torch.no_grad():
        net = m.blocks[0](m.fc_pos(p))[0]
        plan = PoolPlan(pool.cell_index(p, float(m.cfg.radius), int(m.cfg.plane_size))[0], int(m.cfg.plane_size) ** 2)
        for block in m.blocks[1:]:
            net = block(pool.pool_cat(net, plan, kind))
        want = pool.plane_mean(m.fc_c(net), plan).reshape(1, -1, int(m.cfg.plane_size), int(m.cfg.plane_size))
        assert m.block_ops is None and torch.equal(m(p), want)
        assert torch.equal(pool.pointnet_forward(m, p, blocks="torch"), want)
        assert torch.equal(_fixture_encoder(fx, kind, blocks="torch")(p), want)
    with pytest.raises(ValueError):
        pool.pointnet_forward(m, p, blocks="fused")


def test_the_config_class_is_the_same_construction_with_folded_blocks(fx, monkeypatch):
    """tgs_pointnet.LocalPoolPointnetFolded over a stand-in for the reference's module (the reference itself is not needed here)."""
    import sys
    import types
    from guassianhand_amd import tgs_pointnet

    class Base(torch.nn.Module):                                           # the reference's attributes, as pointnet_forward reads them
        def __init__(self, cfg):
            super().__init__()
            inner = LocalPoolPointnet(cfg)
            self.cfg, self.fc_pos, self.blocks, self.fc_c = inner.cfg, inner.fc_pos, inner.blocks, inner.fc_c

    names = ("tgs", "tgs.models", "tgs.models.pointclouds", "tgs.models.pointclouds.pointnet_texture")
    for n in names:
        monkeypatch.setitem(sys.modules, n, types.ModuleType(n))
    sys.modules[names[-1]].LocalPoolPointnet = Base
    monkeypatch.setitem(sys.modules, "torch_scatter", sys.modules.get("torch_scatter") or types.ModuleType("torch_scatter"))   # no shim left behind
    monkeypatch.setattr(tgs_pointnet, "_cache", {})
    plain, folded = tgs_pointnet.LocalPoolPointnet, tgs_pointnet.LocalPoolPointnetFolded
    assert issubclass(folded, plain) and issubclass(plain, Base) and folded.block_ops == "folded" and not hasattr(plain, "block_ops")
    assert tgs_pointnet.LocalPoolPointnetFolded is folded
    a, b = plain(fixture_cfg(fx, "max")), folded(fixture_cfg(fx, "max"))
    a.load_state_dict(fixture_weights(fx))
    b.load_state_dict(fixture_weights(fx))
    a.pool_record, b.pool_record = [], []
    with torch.no_grad():
        pa, pb = a(fx["p"]), b(fx["p"])
    assert a.pool_record[0].shape == (fx["p"].shape[1], int(fx["dims"][2])) and b.pool_record[0].shape == (int(fx["dims"][4]) ** 2, int(fx["dims"][2]))
    assert not torch.equal(pa, pb) and torch.allclose(pa, pb, rtol=0, atol=64 * U * float(pa.abs().max()))
    with pytest.raises(AttributeError):
        tgs_pointnet.LocalPoolPointnetFused


def test_res_rows_refuses_what_does_not_fit():
    x, u, W = torch.zeros(4, 8), torch.zeros(1, 4), torch.zeros(4, 8)
    W1 = torch.zeros(4, 4)
    assert res_block.res_rows(x, u, u, None, W, W, W1).shape == (4, 4)
    for call in (lambda: res_block.res_rows(x, u, u, None, W[:, :4], W, W1), lambda: res_block.res_rows(x, torch.zeros(1, 3), u, None, W, W, W1),
                 lambda: res_block.res_rows(x, u, u, torch.zeros(3, dtype=torch.int32), W, W, W1),
                 lambda: res_block.res_rows(x, u, u, None, W, W, W1, ops="hip")):
        with pytest.raises(ValueError):
            call()


# ---- C-ABI (include/gh_res.h) -------------------------------------------------------------------------------------------------------
def test_res_header_mirror_and_library_agree(gh_lib_path):
    h = open(os.path.join(ROOT, "include", "gh_res.h")).read()
    assert header_symbols("gh_res.h") == sorted(_abi.RES_SYMBOLS)
    assert set(_abi.RES_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    for name in ("GH_RES_ROWS", "GH_RES_MAX_H"):
        assert getattr(_abi, name) == int(re.search(rf"#define {name} (\d+)", h).group(1)), name
    assert res_block.WIDTHS == tuple(range(32, _abi.GH_RES_MAX_H + 1, 32))
    L = C.CDLL(gh_lib_path)
    for s in _abi.RES_SYMBOLS:
        getattr(L, s)


def test_res_arguments_are_validated_before_any_launch(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    _abi.bind_res(L)
    INV, UNSUP = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED
    T, H = 1000, 128
    A, B, D, E, F, G, J, K = (C.c_void_p(k << 24) for k in range(1, 9))     # far apart; never dereferenced

    def fwd(x=A, xs=None, T=T, Cin=H, H=H, u=B, s=D, R=3, row_of=E, W0=F, w0s=None, Ws=G, wss=None, W1=J, out=K, os_=None, mask=None):
        return L.gh_res_forward(x, Cin if xs is None else xs, T, Cin, H, u, s, R, row_of, W0, Cin if w0s is None else w0s, Ws,
                                Cin if wss is None else wss, W1, out, H if os_ is None else os_, mask, None)
    for H_bad in (0, 16, 48, 160, -32):
        assert fwd(H=H_bad, Cin=H_bad) == INV, H_bad
    assert fwd(Cin=3 * H) == INV and fwd(Cin=H // 2) == INV and fwd(R=0) == INV and fwd(R=-1) == INV and fwd(T=-1) == INV
    assert fwd(x=None) == INV and fwd(u=None) == INV and fwd(s=None) == INV and fwd(W0=None) == INV and fwd(Ws=None) == INV
    assert fwd(W1=None) == INV and fwd(out=None) == INV
    assert fwd(xs=H - 1) == INV and fwd(w0s=H - 1) == INV and fwd(wss=H - 1) == INV and fwd(os_=H - 1) == INV
    assert fwd(Cin=2 * H, xs=2 * H - 1) == INV and fwd(x=C.c_void_p((1 << 24) + 2)) == INV
    assert fwd(T=0) == _abi.GH_OK and fwd(T=0, row_of=None, Cin=2 * H) == _abi.GH_OK        # nothing to do: no launch

    def bwd(g=A, gs=None, x=B, xs=None, T=T, Cin=H, H=H, mask=D, W0=F, w0s=None, Ws=G, wss=None, W1=J, dx=K, dxs=None, dh=None):
        return L.gh_res_backward(g, H if gs is None else gs, x, Cin if xs is None else xs, T, Cin, H, mask, W0, Cin if w0s is None else w0s,
                                 Ws, Cin if wss is None else wss, W1, dx, Cin if dxs is None else dxs, dh, None)
    assert bwd(H=48, Cin=48) == INV and bwd(Cin=3 * H) == INV and bwd(T=-1) == INV
    assert bwd(g=None) == INV and bwd(x=None) == INV and bwd(mask=None) == INV and bwd(W0=None) == INV and bwd(dx=None) == INV
    assert bwd(gs=H - 1) == INV and bwd(xs=H - 1) == INV and bwd(dxs=H - 1) == INV and bwd(w0s=1) == INV and bwd(wss=1) == INV
    assert bwd(T=0) == _abi.GH_OK

    n = 1024
    cs = lambda x=A, xs=H, T=T, Cc=H, n=n, st=B, order=D, tail=1, y=E: L.gh_res_cell_sum(x, xs, T, Cc, n, st, order, tail, y, None)
    assert cs(x=None) == INV and cs(y=None) == INV and cs(st=None) == INV and cs(order=None) == INV and cs(Cc=0) == INV and cs(n=0) == INV
    assert cs(xs=H - 1) == INV and cs(T=-1) == INV and cs(n=_abi.GH_POOL_MAX_CELLS + 1) == UNSUP and cs(T=0) == _abi.GH_OK
    cm = lambda x=A, xs=H, T=T, Cc=H, n=n, st=B, order=D, vals=E, arg=F: L.gh_res_cell_max(x, xs, T, Cc, n, st, order, vals, arg, None)
    assert cm(x=None) == INV and cm(vals=None) == INV and cm(arg=None) == INV and cm(order=None) == INV and cm(Cc=0) == INV
    assert cm(xs=H - 1) == INV and cm(n=_abi.GH_POOL_MAX_CELLS + 1) == UNSUP and cm(T=0) == _abi.GH_OK
    cb = lambda gm=A, arg=B, T=T, Cc=H, n=n, gx=D, gxs=H: L.gh_res_cell_max_backward(gm, arg, T, Cc, n, gx, gxs, None)
    assert cb(gm=None) == INV and cb(arg=None) == INV and cb(gx=None) == INV and cb(Cc=0) == INV and cb(n=0) == INV and cb(gxs=H - 1) == INV
    assert cb(T=0) == _abi.GH_OK
