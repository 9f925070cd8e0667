"""The four row-tile blocks — the vertex MLPs (include/gh_vert.h), the point conditioning (include/gh_cond.h), the attention block's
row work (include/gh_attn_rows.h) and the Gaussian trunk with its head (include/gh_trunk.h) — at the value edges of
tests/row_block_edge_cases.py, on the device. Values are held to tests/fit_cases.three_way: the kernel, the float32 torch statements and
the float64 ones run on the device on the same float32 inputs, and

    max|kernel - f64|  <=  4 max|torch32 - f64|  +  2^-20 max|f64|

per field and per group of rows (each kind of edge row on its own, the tame rows on their own; for an activation's tails, per band of
the float64 pre-activation), no element excluded, a group's floor from that group's own max|f64|. vert's parameter gradients sum over
the rows and are judged whole. "Unchanged" and "exactly zero" are torch.equal on fit_cases.bits. Every test that compares values first
asserts its generator's conditions on the float64 reference (tests/test_row_block_edges_cpu.py prints them). The worst error / bound
ratios are recorded under "<block>_edge_<family>" by three_way and printed by each test.

Worst error / bound per family measured on an MI355X (1 = the bound; DESIGN.md has the table with the fields): vert_edge_ln 0.864,
vert_edge_dominant 0.175, vert_edge_kink 0.259, vert_edge_tails 0.540, cond_edge_ln 0.177, cond_edge_combination 0.141, cond_edge_kink
0.152, attn_edge_ln 0.316, attn_edge_dominant 0.087, attn_edge_kink 0.551, trunk_edge_kink 0.264, trunk_edge_silu_ladder 0.557,
head_edge_tails 0.783. The tame rows of every family stay at or below 0.551. The file's 57 tests take 4.8 s."""
import pytest
import torch

from tests import gs_trunk_cases as TC
from tests import row_block_edge_cases as E
from tests.fit_cases import bits, report, three_way

pytestmark = pytest.mark.gpu

MODES = ("f64", "torch32", "kernel")
CASE_ID = TC.case_id


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert (_abi.GH_VERT_ROWS, _abi.GH_COND_ROWS, _abi.GH_TRUNK_ROWS) == (64, 64, TC.R)
    return torch.device("cuda:0")


def unchanged(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def judged(name, tag, res, parts):
    """res: {mode: fields}; parts: (fields, groups) pairs, and (fields, None) for fields judged whole."""
    sp = {m: {} for m in MODES}
    for fields, groups in parts:
        for m in MODES:
            sp[m].update(E.split(res[m], fields, groups) if groups is not None else {f: res[m][f] for f in fields})
    three_way(sp["kernel"], sp["torch32"], sp["f64"], tuple(sp["f64"]), tag=tag, name=name)
    report(name)


def all_modes(run, c, dev):
    return {m: run(m, c, dev) for m in MODES}


# ---- vert -------------------------------------------------------------------------------------------------------------------------------
def vert_params():
    from tests.vert_cases import names
    return names()[2:]


def vert_judged(name, tag, c, dev, out_groups=None):
    res = all_modes(E.vert_run, c, dev)
    judged(name, tag, res, [(("out",), out_groups or c["groups"]), (("grad_x", "grad_pts"), c["groups"]), (vert_params(), None)])
    return res


@pytest.mark.parametrize("kind", range(len(E.LN_KINDS)))
@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_layernorm_rows_with_large_means(dev, P, Cf, K, kind):
    """[x, pts] of the rows at tile positions 0, 31, 32, 63, 64 and of the last row has the mean and deviation of LN_KINDS[kind]: a
    variance formed in one pass is lost entirely on the first three kinds and to 1e-3 on the fourth."""
    c = E.vert_ln_case(P, Cf, K, kind)
    E.vert_ln_conditions(c)
    vert_judged("vert_edge_ln", f"vert LN P={P} Cf={Cf} K={K} rows {E.LN_KINDS[kind]}", c, dev)


@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_one_dominant_column(dev, P, Cf, K):
    """One entry of 1e4 in a tame row, at column 0 and at the last column of each wave's share: all of m2 sits in one wave's partial."""
    c = E.vert_dominant_case(P, Cf, K)
    E.vert_dominant_conditions(c)
    vert_judged("vert_edge_dominant", f"vert dominant P={P} Cf={Cf} K={K}", c, dev)


@pytest.mark.parametrize("P,Cf,K", E.VERT_SHAPES)
def test_vert_units_exactly_on_the_kink(dev, P, Cf, K):
    """Two units of fc1 whose pre-activation is +0.0 and 0 + -0.0 on every row: they take no gradient, to the bit, and hand nothing
    on — the run with their columns of fc2 zeroed gives the same bits."""
    c = E.vert_kink_case(P, Cf, K)
    E.vert_kink_conditions(c)
    res = vert_judged("vert_edge_kink", f"vert kink P={P} Cf={Cf} K={K}", c, dev)["kernel"]
    u = list(c["units"])
    assert E.is_plus_zero(res["grad_fc1_weight"][u]) and E.is_plus_zero(res["grad_fc1_bias"][u])
    cut = E.vert_run("kernel", E.vert_kink_case(P, Cf, K, True), dev)
    for f in E.VERT_FIELDS:
        assert unchanged(res[f], cut[f]), f


@pytest.mark.parametrize("P,Cf,K", E.VERT_TAIL_SHAPES)
def test_vert_activation_tails(dev, P, Cf, K):
    """The final pre-activation from -100 to 100: the sigmoid and its (1 - s) s, the tanh and its 1 - t^2, per band."""
    c = E.vert_tails_case(P, Cf, K)
    E.vert_tails_conditions(c)
    res = vert_judged("vert_edge_tails", f"vert tails P={P} Cf={Cf} K={K}", c, dev, out_groups=c["groups_out"])["kernel"]
    assert all(bool(torch.isfinite(res[f]).all()) for f in E.VERT_FIELDS)


# ---- cond -------------------------------------------------------------------------------------------------------------------------------
def cond_judged(name, tag, c, dev):
    res = all_modes(E.cond_run, c, dev)
    judged(name, tag, res, [(E.COND_FIELDS, c["groups"])])
    return res


@pytest.mark.parametrize("layout,kind", E.COND_LN)
def test_cond_layernorm_rows_with_large_means(dev, layout, kind):
    c = E.cond_ln_case(layout, kind)
    E.cond_ln_conditions(c)
    cond_judged("cond_edge_ln", f"cond LN {layout} rows {E.LN_KINDS[kind]}", c, dev)


@pytest.mark.parametrize("kind", E.COND_COMBOS)
def test_cond_moment_combination(dev, kind):
    """The row's own moments against the folded (m_e, M_e): M_e = 0, a vector whose mean is all of M (the delta^2 term above 0.99 of
    it), one whose deviation is (the term below 1e-6), De = 1, and sine arguments near 400 at L = 8, where the float32 product
    x * f_l is part of the specification and the float32 torch path shares it."""
    c = E.cond_combo_case(kind)
    E.cond_combo_conditions(c)
    cond_judged("cond_edge_combination", f"cond combination {kind}", c, dev)


def test_cond_units_exactly_on_the_kink(dev):
    c = E.cond_kink_case()
    E.cond_kink_conditions(c)
    res = cond_judged("cond_edge_kink", "cond kink", c, dev)["kernel"]
    cut = E.cond_run("kernel", E.cond_kink_case(True), dev)
    for f in E.COND_FIELDS:
        assert unchanged(res[f], cut[f]), f


# ---- the attention block ----------------------------------------------------------------------------------------------------------------
def attn_judged(name, tag, c, dev):
    res = all_modes(E.attn_run, c, dev)
    judged(name, tag, res, [(E.ATTN_FIELDS, c["groups"])])
    return res


@pytest.mark.parametrize("kind", range(len(E.LN_KINDS)))
@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_layernorm_rows_with_large_means(dev, shape, kind):
    """LN1 through the gathered row, LN2 through y = x + fc(attention), whose mean is x's."""
    c = E.attn_ln_case(shape, kind)
    E.attn_ln_conditions(c)
    attn_judged("attn_edge_ln", f"attn LN F={c['F']} hid={c['hid']} rows {E.LN_KINDS[kind]}", c, dev)


@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_one_dominant_column(dev, shape):
    c = E.attn_dominant_case(shape)
    E.attn_dominant_conditions(c)
    attn_judged("attn_edge_dominant", f"attn dominant F={c['F']} hid={c['hid']}", c, dev)


@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_units_exactly_on_the_kink(dev, shape):
    """ff.fc1's unit 3 and its last one — the last bit of the mask's last word, 18 bits wide at hid = 50."""
    c = E.attn_kink_case(shape)
    E.attn_kink_conditions(c)
    res = attn_judged("attn_edge_kink", f"attn kink F={c['F']} hid={c['hid']}", c, dev)["kernel"]
    cut = E.attn_run("kernel", E.attn_kink_case(shape, True), dev)
    for f in E.ATTN_FIELDS:
        assert unchanged(res[f], cut[f]), f


@pytest.mark.parametrize("shape", E.ATTN_SHAPES)
def test_attn_contains_a_nan_and_keeps_a_zero_cotangent(dev, shape):
    """A NaN in the listed row of batch element 0 that shares its 64-row tile with 63 rows of batch element 1: those, and every
    unlisted row, keep their bits forward and backward. A zero cotangent gives +0.0 everywhere, as the statements do."""
    c = E.attn_nan_case(shape)
    E.check_attn_containment(lambda x: E.attn_run("kernel", c, dev, idx=c["idx"], x=x), c, unchanged)
    k = E.attn_kink_case(shape)
    assert E.is_plus_zero(E.attn_run("kernel", k, dev, cot=torch.zeros_like(k["cot"]))["grad_x"])
    assert E.is_plus_zero(E.attn_run("kernel", c, dev, idx=c["idx"], cot=torch.zeros_like(c["cot"]))["grad_x"])


# ---- the trunk and the head -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.TRUNK_RELU, ids=CASE_ID)
def test_trunk_units_exactly_on_the_kink(dev, case):
    """Units with a zero weight row, 0 on every row, and units with their weight rows and a zero bias, 0 on the three rows of x
    that are zero: there a gate that opened at 0 would add d W1[u, :] to grad_x. The rows of zeros are judged as a group of their
    own and keep their bits when W2's columns for those units are zeroed; every row keeps them when the zero-row units' are."""
    c = E.trunk_kink_case(case)
    E.trunk_kink_conditions(c, CASE_ID(case))
    res = all_modes(E.trunk_run, c, dev)
    judged("trunk_edge_kink", f"trunk kink {CASE_ID(case)}", res, [(TC.OUT, c.groups)])
    cut = E.trunk_run("kernel", E.trunk_kink_case(case, "units"), dev)
    live = E.trunk_run("kernel", E.trunk_kink_case(case, "live"), dev)
    rows = list(c.zero_rows)
    assert float(res["kernel"]["grad_x"][rows].abs().max()) > 0
    for f in TC.OUT:
        assert unchanged(res["kernel"][f], cut[f]), f
        assert unchanged(res["kernel"][f][rows], live[f][rows]), f


@pytest.mark.parametrize("case", E.TRUNK_SILU, ids=CASE_ID)
def test_trunk_silu_row_ladder(dev, case):
    """Rows of x scaled from 0.25 to 64: hidden pre-activations to +-180, where expf(-v) overflows in v / (1 + expf(-v)) and in the
    derivative's sigmoid. The rows are judged by the band of their largest |v1|."""
    c = E.trunk_ladder_case(case)
    E.trunk_ladder_conditions(c, CASE_ID(case))
    res = all_modes(E.trunk_run, c, dev)
    assert all(bool(torch.isfinite(res["kernel"][f]).all()) for f in TC.OUT)
    judged("trunk_edge_silu_ladder", f"trunk ladder {CASE_ID(case)}", res, [(TC.OUT, c.groups)])


@pytest.mark.parametrize("case", E.TRUNK_HEAD, ids=CASE_ID)
def test_head_activation_tails_through_the_trunk(dev, case):
    """Opacity, colour and the restricted offset at raw values to +-100, per band of the raw value; quaternion norms from 1e-6 to 1e4,
    one scale per run; every field of every run whole as well."""
    for q in E.QUAT_SCALES:
        c = E.trunk_head_case(case, q)
        E.trunk_head_conditions(c, CASE_ID(case))
        res = all_modes(E.trunk_run, c, dev)
        assert all(bool(torch.isfinite(res["kernel"][f]).all()) for f in TC.OUT)
        judged("head_edge_tails", f"head tails {CASE_ID(case)} qscale {q:g}", res, [(TC.OUT, None)] + [((f,), b) for f, b in c.bands.items()])


@pytest.mark.parametrize("case", E.TRUNK_SILU + E.TRUNK_RELU, ids=CASE_ID)
def test_trunk_contains_a_nan_and_keeps_zero_cotangents(dev, case):
    """A NaN in row 31, and in row 32, of P = 129 — the last lane of one wave, the first of the next: all other rows keep their bits,
    in the five outputs and in grad_x. All five cotangents zero: grad_x and grad_pts are +0.0 everywhere, as the statements give them."""
    c = TC.make(case)
    E.check_trunk_containment(lambda x: E.trunk_run("kernel", c, dev, x=x), c, unchanged)
    z = E.trunk_run("kernel", E.zero_cotangents(c), dev)
    assert E.is_plus_zero(z["grad_x"]) and E.is_plus_zero(z["grad_pts"])
