"""tests/row_block_edge_cases.py without a device: every generator's conditions on its float64 reference alone (the figures are printed),
and the behaviour of the torch statements that tests/test_gpu_row_block_edges.py asks of the kernels: relu'(0) = 0 for either zero, a
unit on the kink passes nothing on and takes no gradient, a NaN stays in its row or its batch element, and zero cotangents give
gradients that are +0.0 in every element — so the GPU file asks the kernels for bit-zero, not for a signed zero."""
import pytest
import torch
import torch.nn.functional as F

from tests import gs_trunk_cases as TC
from tests import row_block_edge_cases as E
from tests.fit_cases import bits

F64 = torch.float64
same = torch.equal                                               # "unchanged" on the CPU: the same values, NaN nowhere among them
CASE_ID = TC.case_id


# ---- the generators' conditions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(len(E.LN_KINDS)))
@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_layernorm_rows_conditions(P, Cf, K, kind):
    c = E.vert_ln_case(P, Cf, K, kind)
    E.vert_ln_conditions(c)
    assert set(E.TILE_ROWS) <= set(c["rows"]) and max(c["rows"]) == P - 1


@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_dominant_and_kink_conditions(P, Cf, K):
    E.vert_dominant_conditions(E.vert_dominant_case(P, Cf, K))
    E.vert_kink_conditions(E.vert_kink_case(P, Cf, K))


@pytest.mark.parametrize("P,Cf,K", E.VERT_TAIL_SHAPES)
def test_vert_tails_conditions(P, Cf, K):
    c = E.vert_tails_case(P, Cf, K)
    E.vert_tails_conditions(c)
    ref = E.vert_run("f64", c)
    assert all(bool(torch.isfinite(ref[f]).all()) for f in E.VERT_FIELDS)


@pytest.mark.parametrize("layout,kind", E.COND_LN)
def test_cond_layernorm_rows_conditions(layout, kind):
    E.cond_ln_conditions(E.cond_ln_case(layout, kind))


def test_cond_combination_conditions():
    """Across the broadcast vectors the delta^2 term runs from nothing to all of M."""
    share = {k: E.cond_combo_conditions(E.cond_combo_case(k)) for k in E.COND_COMBOS}
    assert float(share["m64"].min()) > 0.99 and float(share["d50"].min()) < 1e-6
    E.cond_kink_conditions(E.cond_kink_case())


@pytest.mark.parametrize("kind", range(len(E.LN_KINDS)))
@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_layernorm_rows_conditions(shape, kind):
    E.attn_ln_conditions(E.attn_ln_case(shape, kind))


@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_dominant_and_kink_conditions(shape):
    E.attn_dominant_conditions(E.attn_dominant_case(shape))
    c = E.attn_kink_case(shape)
    E.attn_kink_conditions(c)
    assert c["units"][1] % 32 == (c["hid"] - 1) % 32             # the last bit of the mask's last word


@pytest.mark.parametrize("case", E.TRUNK_RELU, ids=CASE_ID)
def test_trunk_kink_conditions(case):
    E.trunk_kink_conditions(E.trunk_kink_case(case), CASE_ID(case))


@pytest.mark.parametrize("case", E.TRUNK_SILU, ids=CASE_ID)
def test_trunk_ladder_conditions(case):
    c = E.trunk_ladder_case(case)
    E.trunk_ladder_conditions(c, CASE_ID(case))
    ref = E.trunk_run("f64", c)
    assert all(bool(torch.isfinite(ref[f]).all()) for f in TC.OUT)


@pytest.mark.parametrize("case", E.TRUNK_HEAD, ids=CASE_ID)
def test_trunk_head_conditions(case):
    for q in E.QUAT_SCALES:
        c = E.trunk_head_case(case, q)
        E.trunk_head_conditions(c, CASE_ID(case))
        ref = E.trunk_run("f64", c)
        assert all(bool(torch.isfinite(ref[f]).all()) for f in TC.OUT)
    assert E.QUAT_SCALES[0] == 1e-6 and E.QUAT_SCALES[-1] == 1e4


# ---- the torch statements at the kink ---------------------------------------------------------------------------------------------------
def test_relu_has_no_slope_at_either_zero():
    for dtype in (torch.float32, F64):
        x = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=dtype, requires_grad=True)
        F.relu(x).backward(torch.ones(4, dtype=dtype))
        assert same(x.grad, torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=dtype))
        assert float(F.linear(torch.ones(1, 3), torch.zeros(1, 3), torch.tensor([-0.0]))) == 0.0


def _kink_pair(run, plain, cut, fields):
    """The statements on the case and on the one whose outgoing weights are cut: the same values in every field, either precision."""
    for mode in ("torch32", "f64"):
        a, b = run(mode, plain), run(mode, cut)
        for f in fields:
            assert same(a[f], b[f]), (mode, f)
    return run("torch32", plain)


@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_statements_at_the_kink(P, Cf, K):
    c = E.vert_kink_case(P, Cf, K)
    res = _kink_pair(E.vert_run, c, E.vert_kink_case(P, Cf, K, True), E.VERT_FIELDS)
    u = list(c["units"])
    assert float(res["grad_fc1_weight"][u].abs().max()) == 0.0 and float(res["grad_fc1_bias"][u].abs().max()) == 0.0
    assert float(res["grad_fc1_weight"].abs().max()) > 0


def test_cond_statements_at_the_kink():
    _kink_pair(E.cond_run, E.cond_kink_case(), E.cond_kink_case(True), E.COND_FIELDS)


@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_statements_at_the_kink(shape):
    _kink_pair(E.attn_run, E.attn_kink_case(shape), E.attn_kink_case(shape, True), E.ATTN_FIELDS)


@pytest.mark.parametrize("case", E.TRUNK_RELU, ids=CASE_ID)
def test_trunk_statements_at_the_kink(case):
    """Cutting W2's columns for the zero-row units changes nothing on any row; cutting those for the live units changes nothing on
    the rows of zeros, where alone they sit on the kink (and does change other rows, where they are ordinary units)."""
    c = E.trunk_kink_case(case)
    _kink_pair(E.trunk_run, c, E.trunk_kink_case(case, "units"), TC.OUT)
    rows = list(c.zero_rows)
    for mode in ("torch32", "f64"):
        a, b = E.trunk_run(mode, c), E.trunk_run(mode, E.trunk_kink_case(case, "live"))
        for f in TC.OUT:
            assert same(a[f][rows], b[f][rows]), (mode, f)
        assert not same(a["grad_x"], b["grad_x"])
        assert float(a["grad_x"][rows].abs().max()) > 0


# ---- NaN containment and zero cotangents of the torch statements ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_statements_contain_a_nan_and_keep_a_zero_cotangent(shape):
    c = E.attn_nan_case(shape)
    for mode in ("torch32", "f64"):
        E.check_attn_containment(lambda x, mode=mode: E.attn_run(mode, c, idx=c["idx"], x=x), c, same)
    listed = torch.zeros(E.ATTN_NAN["V"], dtype=torch.bool)
    listed[c["idx"].long()] = True
    assert int(listed.sum()) == E.ATTN_NAN["listed"] > 64        # the listed rows of batch element 0 reach into the second tile
    k = E.attn_kink_case(shape)
    for mode in ("torch32", "f64"):
        g = E.attn_run(mode, k, cot=torch.zeros_like(k["cot"]))["grad_x"]
        assert E.is_plus_zero(g), mode


@pytest.mark.parametrize("case", E.TRUNK_SILU + E.TRUNK_RELU, ids=CASE_ID)
def test_trunk_statements_contain_a_nan_and_keep_zero_cotangents(case):
    c = TC.make(case)
    for mode in ("torch32", "f64"):
        E.check_trunk_containment(lambda x, mode=mode: E.trunk_run(mode, c, x=x), c, same)
        z = TC.run(E.zero_cotangents(c), mode)
        assert E.is_plus_zero(z["grad_x"]) and E.is_plus_zero(z["grad_pts"]), mode
    assert bits(torch.zeros(1)).item() == 0 and bits(torch.tensor([-0.0])).item() != 0
