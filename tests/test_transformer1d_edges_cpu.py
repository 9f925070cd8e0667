"""tests/transformer1d_edge_cases.py without a device: every generator's conditions on its float64 reference alone (the figures are
printed: max|s| and the p_max shares of the ladder, the dominant key's gap, the gate's span, the rows' mean / deviation), and the
properties that need no kernel, NaN containment and the zero cotangent, against the torch statements and transformer1d_ref, so that what
the GPU file asks of the kernels is what the statements themselves do."""
import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import transformer1d as X
from tests import transformer1d_cases as K
from tests import transformer1d_edge_cases as E

F64 = torch.float64
same = torch.equal                                               # "unchanged" on the CPU: the same float64 values, NaN nowhere among them


# ---- the generators' conditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.LADDER_N)
@pytest.mark.parametrize("D", E.HEAD_DIMS)
def test_ladder_conditions(D, N):
    c = E.ladder_case(D, N)
    m = E.ladder_conditions(c)
    assert m["max|s|"] > 20                                      # and the ladder does reach far: a stage's maximum can dwarf the last one's
    ref = E.attention_all(c["qkv"], c["dout"], c["B"], N, c["heads"], D, F64)
    assert all(bool(torch.isfinite(ref[f]).all()) and float(ref[f].abs().max()) > 0 for f in E.ATTN_FIELDS)


@pytest.mark.parametrize("N,key", E.DOMINANT)
@pytest.mark.parametrize("D", E.HEAD_DIMS)
def test_dominant_key_conditions(D, N, key):
    c = E.dominant_case(D, N, key)
    E.dominant_conditions(c)
    # the key's place in the forward's stages: the last key of a full stage, or the one key of the last stage's even or odd tile
    assert key == N - 1 and (key % K.ATTN_KEYS == K.ATTN_KEYS - 1 or key % 32 == 0)


@pytest.mark.parametrize("Kc", E.LN_K)
@pytest.mark.parametrize("constant", [False, True])
def test_layernorm_rows_conditions(Kc, constant):
    d = E.ln_rows_case(Kc, "plain", constant)
    E.ln_rows_conditions(d, constant)
    if constant:
        # small dyadic constants: every partial sum of K <= 512 of them is exact in float32, in any order
        for v in set(E.CONST_ROWS.values()):
            assert float(torch.tensor(v * Kc, dtype=torch.float32)) == v * Kc and (v * 4).is_integer()


@pytest.mark.parametrize("Cc", E.GN_C)
def test_group_step_conditions(Cc):
    d = E.gn_step_case(Cc)
    E.gn_step_conditions(d)
    assert d["x"].shape == (E.GN_B, Cc, 2 * K.GN_CHUNK + 1)


def test_geglu_tails_conditions():
    d = E.geglu_tails_case()
    mid, high = E.geglu_tails_conditions(d)
    y = K.linear_ref(d, "ln", "geglu", F64)
    assert bool(torch.isfinite(y).all()) and not bool((mid & high).any())
    # the high band is judged on its own, larger scale; the middle band is not drowned by it
    assert float(y[:, high].abs().max()) > 2 * float(y[:, mid].abs().max()) > 0


# ---- NaN containment and zero cotangents of the torch statements ----------------------------------------------------------------------------
def test_attention_statements_contain_a_nan_and_keep_a_zero_cotangent():
    c = E.nan_attention_case()
    run = lambda qkv, dout: E.attention_all(qkv, dout, c["B"], c["N"], c["heads"], c["D"], F64)
    E.check_attention_containment(run, c, same)
    E.check_attention_zero_cotangent(run, c)


@pytest.mark.parametrize("epi", K.EPILOGUES)
@pytest.mark.parametrize("pro", K.PROLOGUES)
def test_linear_statements_contain_a_nan(pro, epi):
    E.check_linear_containment(lambda d, x: K.linear_ref(dict(d, x=x), pro, epi, F64), pro, epi, same)


def test_row_backward_statements_contain_a_nan_and_keep_a_zero_cotangent():
    d = E.nan_rows_backward_case()
    # the statements take their moments from x, so mom is no operand of theirs
    ln = lambda dn, x, g: K.ln_ref(x, dn, g, d["gamma"], d["beta"], F64)["g"]
    E.check_rows_containment(ln, ("dn", "x", "g"), d, same)
    assert same(ln(torch.zeros_like(d["dn"]), d["x"], d["g"]), d["g"].double())
    ge = lambda g, h: K.geglu_ref(dict(d, g=g, h=h), F64)["dadg"]
    E.check_rows_containment(ge, ("g", "h"), dict(d, h=d["x"]), same)
    assert bool((ge(torch.zeros_like(d["g"]), d["x"]) == 0).all())


def test_group_statements_contain_a_nan_and_keep_a_zero_cotangent():
    d = E.nan_groups_case()
    mom = lambda t: torch.stack(list(E.group_moments_ref(t["x"].double(), t["G"]).values()), dim=-1)
    E.check_groups_containment(mom, d, same, "x", per_group=True)
    bwd = lambda t: K.gn_ref(t["x"], t["dy"], t["dout"], t["gamma"], t["beta"], t["G"], F64)["dx"]
    E.check_groups_containment(bwd, d, same, "dy", per_group=False)
    assert same(bwd(dict(d, dy=torch.zeros_like(d["dy"]))), d["dout"].double())


def test_whole_stack_statements_contain_a_nan_and_keep_a_zero_cotangent():
    x, dout = E.stack_inputs()
    p = X._map(X.params_of(E.stack_module()), lambda t: t.double())

    def run(x_, dout_):
        t = x_.double().requires_grad_(True)
        out = X.transformer1d_ref(p, t)
        return out.detach(), torch.autograd.grad(out, t, dout_.double())[0]

    E.check_stack(run, x, dout, same)
