"""The Transformer1D kernels (include/gh_xf.h) at the value edges of tests/transformer1d_edge_cases.py, on the device. Values are held
to tests/fit_cases.three_way: the kernel, the float32 torch statements and the float64 ones run on the device on the same float32
inputs, and per field max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64|, no element excluded; the three errors are printed.
"Unchanged" and "exact" are torch.equal on fit_cases.bits. Every test that compares values first asserts its generator's conditions on
the float64 reference (tests/test_transformer1d_edges_cpu.py prints them).

The worst error / bound ratios are recorded under the names "xf_edge_*" by fit_cases.three_way and printed by each test.

Worst error / bound ratios measured on an MI355X (1 = the bound; no kernel missed it, and gh_xf.hip needed no change):

    xf_edge_ladder              out 0.236   lse 0.138   dq 0.377   dk 0.393   dv 0.325
    xf_edge_dominant            out 0.000   lse 0.151   dq 0.250   dk 0.250   dv 0.147
    xf_edge_ln_rows             y 0.313
    xf_edge_ln_rows_backward    g 0.091   rows 8 + N(0, 1) 0.130   rows 64 + N(0, 1) 0.172   rows 1e-3 N(0, 1) 0.091   constant rows 0.088
    xf_edge_gn_step             mean 0.142   m2 0.110   y 0.055   dx 0.096
    xf_edge_geglu_tails         y 0.243   |gate| <= 4: 0.272   gate > 4: 0.243

In the dominant-key cases the kernel's out is v[key] bit for bit, and the float64 dq and dk are below 2e-10 (the softmax is saturated in
every row): the kernel and the float32 statements miss them by the same 4 digits, about the size of the field itself, as both find the
dominant key's dp - delta to be exactly 0; the ratio 0.250 is then 1 / 4 by construction and judges nothing. out, lse and dv do."""
import pytest
import torch

from tests import transformer1d_cases as K
from tests import transformer1d_edge_cases as E
from tests.fit_cases import bits, report, three_way

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert (_abi.GH_XF_ROWS, _abi.GH_XF_COLS, _abi.GH_XF_ATTN_ROWS, _abi.GH_XF_ATTN_KEYS, _abi.GH_XF_GN_CHUNK) == \
        (K.ROW_TILE, K.COL_TILE, K.ATTN_ROWS, K.ATTN_KEYS, K.GN_CHUNK)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def X():
    from guassianhand_amd import transformer1d
    return transformer1d


def unchanged(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def judged(name, kernel, torch32, f64, fields, tag):
    three_way(kernel, torch32, f64, fields, tag=tag, name=name)
    report(name)


# ---- attention: out, lse, dq, dk, dv ----------------------------------------------------------------------------------------------------
def attention_three_way(X, c, name, tag):
    qkv, dout, B, N, heads, D = (c[k] for k in ("qkv", "dout", "B", "N", "heads", "D"))
    got = E.attention_kernel_all(X, qkv, dout, B, N, heads, D)
    judged(name, got, E.attention_all(qkv, dout, B, N, heads, D, F32), E.attention_all(qkv, dout, B, N, heads, D, F64), E.ATTN_FIELDS, tag)
    return got


@pytest.mark.parametrize("N", E.LADDER_N)
@pytest.mark.parametrize("D", E.HEAD_DIMS)
def test_attention_temperature_ladder(dev, X, D, N):
    """Query temperatures from 0.25 to 12 in one launch: rows that one key saturates beside flat ones, |s| up to 35 .. 53, so that a
    stage's maximum dwarfs the one before it in the forward's alpha, the pair join's a0 / a1 and lse, and the backward's
    p = exp(s scale - lse) runs from 1 down to underflow."""
    c = E.ladder_case(D, N)
    E.ladder_conditions(c)
    attention_three_way(X, E.to(c, dev), "xf_edge_ladder", f"ladder D={D} N={N}")


@pytest.mark.parametrize("N,key", E.DOMINANT)
@pytest.mark.parametrize("D", E.HEAD_DIMS)
def test_attention_dominant_key_at_a_stage_edge(dev, X, D, N, key):
    """One key outweighs the rest by e^25: the last key of a full stage (64, 63), the one key of the last stage in the even wave's
    tile (65, 64), (129, 128), and in the odd wave's (97, 96). out is then v[key] to 2^-20 max|v|."""
    c = E.dominant_case(D, N, key)
    E.dominant_conditions(c)
    c = E.to(c, dev)
    got = attention_three_way(X, c, "xf_edge_dominant", f"dominant key D={D} N={N} key={key}")
    v = c["qkv"][:, 2 * D:]
    off = float((got["out"] - v[key]).abs().max())
    print(f"dominant key D={D} N={N} key={key}: kernel max|out - v[key]| {off:.3e}, max|v| {float(v.abs().max()):.3e}")
    assert off <= 2.0 ** -20 * float(v.abs().max())


def test_attention_contains_a_nan_and_keeps_a_zero_cotangent(dev, X):
    c = E.to(E.nan_attention_case(), dev)
    run = lambda qkv, dout: E.attention_kernel_all(X, qkv, dout, c["B"], c["N"], c["heads"], c["D"])
    E.check_attention_containment(run, c, unchanged)
    E.check_attention_zero_cotangent(run, c)


# ---- LayerNorm rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["plain", "geglu"])
@pytest.mark.parametrize("Kc", E.LN_K)
def test_layernorm_prologue_on_rows_with_large_means(dev, Kc, epi):
    """Rows 8 + N(0, 1), 64 + N(0, 1) and 1e-3 N(0, 1) in one tensor. A variance formed in one pass loses about 64^2 2^-24 = 2e-4 of
    the second kind's; the two-pass form stays within the float32 statements' own error."""
    d = E.ln_rows_case(Kc, epi)
    E.ln_rows_conditions(d)
    d = E.to(d, dev)
    judged("xf_edge_ln_rows", {"y": K.linear_kernel(d, "ln", epi)}, {"y": K.linear_ref(d, "ln", epi, F32)}, {"y": K.linear_ref(d, "ln", epi, F64)},
           ("y",), f"LN rows K={Kc} {epi}")


@pytest.mark.parametrize("constant", [False, True], ids=["rows", "constant_rows"])
@pytest.mark.parametrize("Kc", E.LN_K)
def test_layernorm_backward_on_rows_with_large_means(dev, X, Kc, constant):
    d = E.ln_rows_case(Kc, "plain", constant)
    E.ln_rows_conditions(d, constant)
    d = E.to(d, dev)
    x, dn, g0, gamma, beta = (d[k] for k in ("x", "dn", "g0", "gamma", "beta"))
    got = X.layernorm_backward(dn, x, E.ln_moments(x), gamma, g0.clone())
    # all rows, then each kind of row on its own scale: the rows of deviation 1e-3 (and the constant ones) carry rstd up to 316
    const = torch.zeros(E.LN_T, dtype=torch.bool, device=dev)
    if constant:
        const[list(E.CONST_ROWS)] = True
    kinds = {f"g_{o:g}_{s:g}": (torch.arange(E.LN_T, device=dev) % 3 == i) & ~const for i, (o, s) in enumerate(E.LN_ROWS)}
    if constant:
        kinds["g_const"] = const
    split = lambda r: dict(r, **{k: r["g"][sel].contiguous() for k, sel in kinds.items()})
    judged("xf_edge_ln_rows_backward", split({"g": got}), split(K.ln_ref(x, dn, g0, gamma, beta, F32)), split(K.ln_ref(x, dn, g0, gamma, beta, F64)),
           ("g", *kinds), f"LN backward rows K={Kc} constant={constant}")


@pytest.mark.parametrize("epi", ["plain", "geglu", "bias"])
@pytest.mark.parametrize("Kc", E.LN_K)
def test_layernorm_of_constant_rows_is_exactly_the_zero_rows(dev, X, Kc, epi):
    """Rows of 3.0 and of -0.5: the sums are exact, the mean is the value and every centred value 0, as in the all-zero row. The rows'
    outputs are then the zero row's of the same call bit for bit, for every epilogue without a residual."""
    d = E.ln_rows_case(Kc, "geglu" if epi == "geglu" else "plain", True)
    E.ln_rows_conditions(d, True)
    d = E.to(d, dev)
    if epi == "bias":
        y = X.linear(d["x"], d["w"], prologue="ln", epilogue="bias_res", bias=d["bias"], gamma=d["gamma"], beta=d["beta"], eps=1e-5)
    else:
        y = K.linear_kernel(d, "ln", epi)
    assert bool(torch.isfinite(y).all()) and float(y[E.ZERO_ROW].abs().max()) > 0
    for r in E.CONST_ROWS:
        assert unchanged(y[r], y[E.ZERO_ROW]), (Kc, epi, r)
    assert not unchanged(y[E.ZERO_ROW + 2], y[E.ZERO_ROW])


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", E.GN_C)
def test_group_norm_constant_group_and_step(dev, X, Cc):
    """N = 2 GN_CHUNK + 1: three partials per group, the last of one position. (a) the group of 3.0 has the moments (3.0, 0.0) exactly
    and the norm gives beta there, through the identity weight; (b) the groups with a step of 8 and one value of 100, whose variance is
    the partial means' spread, against the statements."""
    d = E.gn_step_case(Cc)
    const = E.gn_step_conditions(d).to(dev)
    d = E.to(d, dev)
    x, G, N = d["x"], d["G"], d["N"]
    mom = X.group_moments(x, G)
    assert bool((mom[..., 0][const] == E.GN_CONST).all()) and bool((mom[..., 1][const] == 0).all())
    judged("xf_edge_gn_step", {"mean": mom[..., 0].contiguous(), "m2": mom[..., 1].contiguous()}, E.group_moments_ref(x, G),
           E.group_moments_ref(x.double(), G), ("mean", "m2"), f"group moments step C={Cc}")
    kw = dict(prologue="gn", gamma=d["gamma"], beta=d["beta"], eps=1e-6, groups=G, moments=mom)
    y = X.linear(x, torch.eye(Cc, device=dev), **kw).reshape(E.GN_B, N, Cc)
    cpg = Cc // G
    for b, g in enumerate(E.GN_CONST_GROUP):
        ch = slice(g * cpg, (g + 1) * cpg)
        assert unchanged(y[b, :, ch], d["beta"][ch].expand(N, cpg)), (b, g)
    judged("xf_edge_gn_step", {"y": K.linear_kernel(d, "gn", "plain")}, {"y": K.linear_ref(d, "gn", "plain", F32)},
           {"y": K.linear_ref(d, "gn", "plain", F64)}, ("y",), f"gn prologue step C={Cc}")
    got = X.group_norm_backward(d["dy"], x, mom, d["gamma"], d["dout"], G)
    ref = lambda dtype: K.gn_ref(x, d["dy"], d["dout"], d["gamma"], d["beta"], G, dtype)
    judged("xf_edge_gn_step", {"dx": got}, ref(F32), ref(F64), ("dx",), f"group norm backward step C={Cc}")


# ---- the GEGLU epilogue's tails ---------------------------------------------------------------------------------------------------------------
def test_geglu_forward_both_tails(dev):
    """The gate from -12 to 12: erff saturates on both sides, y is 0 or a g. The whole field, then the columns with |gate| <= 4 and
    those with gate > 4 each on their own scale."""
    d = E.geglu_tails_case()
    mid, high = E.geglu_tails_conditions(d)
    d = E.to(d, dev)
    y, t32, f64 = K.linear_kernel(d, "ln", "geglu"), K.linear_ref(d, "ln", "geglu", F32), K.linear_ref(d, "ln", "geglu", F64)
    assert bool(torch.isfinite(y).all())
    band = lambda t, cols: t[:, cols.to(dev)].contiguous()
    judged("xf_edge_geglu_tails", {"y": y, "y_mid": band(y, mid), "y_high": band(y, high)}, {"y": t32, "y_mid": band(t32, mid), "y_high": band(t32, high)},
           {"y": f64, "y_mid": band(f64, mid), "y_high": band(f64, high)}, ("y", "y_mid", "y_high"), "GEGLU forward |gate| up to 12")


# ---- NaN containment and zero cotangents of the row kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", K.EPILOGUES)
@pytest.mark.parametrize("pro", K.PROLOGUES)
def test_linear_contains_a_nan(dev, pro, epi):
    """T = 99 = 3 x 33: rows 33 .. 63 of batch element 1 share the first 64-row tile with batch element 0, its rows 64 and 65 the
    second tile with batch element 2."""
    E.check_linear_containment(lambda d, x: K.linear_kernel(dict(d, x=x), pro, epi), pro, epi, unchanged, device=dev)


def test_row_backwards_contain_a_nan_and_keep_a_zero_cotangent(dev, X):
    d = E.to(E.nan_rows_backward_case(), dev)
    ln = lambda dn, x, mom, g: X.layernorm_backward(dn, x, mom, d["gamma"], g.clone())
    E.check_rows_containment(ln, ("dn", "x", "mom", "g"), d, unchanged)
    assert unchanged(ln(torch.zeros_like(d["dn"]), d["x"], d["mom"], d["g"]), d["g"])
    w2t = d["w2"].t().contiguous()
    ge = lambda g, h, mom: X.geglu_backward(g, h, mom, d["gamma"], d["beta"], d["w1"], d["b1"], w2t)
    E.check_rows_containment(ge, ("g", "h", "mom"), dict(d, h=d["x"]), unchanged)
    assert bool((ge(torch.zeros_like(d["g"]), d["x"], d["mom"]) == 0).all())


def test_group_kernels_contain_a_nan_and_keep_a_zero_cotangent(dev, X):
    d = E.to(E.nan_groups_case(), dev)
    E.check_groups_containment(lambda t: X.group_moments(t["x"], t["G"]), d, unchanged, "x", per_group=True)
    mom = X.group_moments(d["x"], d["G"])
    bwd = lambda t: X.group_norm_backward(t["dy"], t["x"], mom, t["gamma"], t["dout"], t["G"])
    E.check_groups_containment(bwd, d, unchanged, "dy", per_group=False)
    assert unchanged(bwd(dict(d, dy=torch.zeros_like(d["dy"]))), d["dout"])


# ---- the whole stack -------------------------------------------------------------------------------------------------------------------------
def test_whole_stack_contains_a_nan_and_keeps_a_zero_cotangent(dev, X):
    """C = 64, two heads of 32, two layers with attn2, B = 3, N = 65: T = 195, every 64-row tile but the first straddles two batch
    elements. Frozen and fused with grad="input"."""
    x, dout = (t.to(dev) for t in E.stack_inputs())
    m = X.fuse_transformer1d(E.stack_module(dev), grad="input")
    n = K.StandIn.calls

    def run(x_, dout_):
        t = x_.clone().requires_grad_(True)
        out = m(t)
        assert out.requires_grad
        return out.detach(), torch.autograd.grad(out, t, dout_)[0]

    E.check_stack(run, x, dout, unchanged)
    assert K.StandIn.calls == n                                   # the kernels ran, not the base forward
