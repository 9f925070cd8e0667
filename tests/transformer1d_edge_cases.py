"""Shared by tests/test_transformer1d_edges_cpu.py and tests/test_gpu_transformer1d_edges.py: the value edges of the Transformer1D
kernels (include/gh_xf.h). The shapes are swept elsewhere (tests/transformer1d_cases.py); here the data is what a kernel can get wrong
at a tame shape: scores whose maximum moves by tens between two stages of the streaming softmax, one key that takes all the weight and
sits alone in a stage's tile, rows whose mean dwarfs their deviation, groups with a step, gates deep in both tails of the GELU, a NaN
next to rows that must not see it, and cotangents that are exactly zero.

Every generator draws on the CPU from a seeded generator and returns float32 tensors; every value case states, as `*_conditions`,
what it promises about its own float64 reference (the edge is really there, and the reference is not ill-conditioned), returns the
measured figures and asserts them. A test that compares values asserts the conditions first: a case whose reference fails them fails
its test. The two criteria are the project's: tests/fit_cases.three_way for values, torch.equal on fit_cases.bits for "unchanged" and
"exact". Treat what the cached builders return as read-only."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import transformer1d_cases as K

NAN = float("nan")
HEAD_DIMS = (32, 64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def to(d, device):
    """A case's tensors on `device` (other entries as they are)."""
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# ---- attention: out, lse and the three gradients in `dtype` -------------------------------------------------------------------------------
ATTN_FIELDS = ("out", "lse", "dq", "dk", "dv")


def attention_all(qkv, dout, B, N, heads, D, dtype):
    """{out, lse, dq, dk, dv} of the torch statements in `dtype`, on qkv's device."""
    d = K.attention_grads(qkv.clone(), dout, B, N, heads, D, dtype)     # a copy: the float32 statements turn their argument into a leaf
    d.update(out=K.attention_ref(qkv, B, N, heads, D, dtype), lse=K.lse_ref(qkv, B, N, heads, D, dtype))
    return d


def attention_kernel_all(X, qkv, dout, B, N, heads, D):
    """The same five fields through attention_lse and attention_backward; `attention` is bitwise attention_lse's out."""
    from tests.fit_cases import bits
    out, lse = X.attention_lse(qkv, B, N, heads, D)
    assert torch.equal(bits(X.attention(qkv, B, N, heads, D)), bits(out))
    g = X.attention_backward(qkv, out, lse, dout, B, N, heads, D)
    M = heads * D
    return {"out": out, "lse": lse, "dq": g[:, :M].contiguous(), "dk": g[:, M:2 * M].contiguous(), "dv": g[:, 2 * M:].contiguous()}


def scores64(qkv, B, N, heads, D):
    """The float64 scores (B, heads, N, N) and each row's largest softmax weight (B, heads, N)."""
    M = heads * D
    q, k, _v = (t.reshape(B, N, heads, D).transpose(1, 2) for t in qkv.double().split(M, dim=1))
    s = q @ k.transpose(-1, -2) * D ** -0.5
    return s, torch.softmax(s, dim=-1).amax(dim=-1)


# 1. the temperature ladder: query row i of every head times t_i, the N values of t geometric from 0.25 to 12 in a seeded order
LADDER_N = (33, 65, 97, 129)
LADDER_T = (0.25, 12.0)


@functools.lru_cache(maxsize=None)
def ladder_case(D, N, heads=2, B=2):
    gen = _gen(5000 + N + D)
    M = heads * D
    qkv = torch.randn(B * N, 3 * M, generator=gen)
    t = torch.logspace(math.log10(LADDER_T[0]), math.log10(LADDER_T[1]), N, dtype=torch.float64)[torch.randperm(N, generator=gen)].float()
    qkv[:, :M] *= t.repeat(B)[:, None]
    dout = torch.randn(B * N, M, generator=gen)
    return {"qkv": qkv, "dout": dout, "B": B, "N": N, "heads": heads, "D": D}


def ladder_conditions(c):
    """max|s| <= 60 (exp(-s) stays normal and the reference well conditioned), one row saturated and a third of the rows flat."""
    s, p_max = scores64(c["qkv"], c["B"], c["N"], c["heads"], c["D"])
    m = {"max|s|": float(s.abs().max()), "max p_max": float(p_max.max()), "share p_max<0.3": float((p_max < 0.3).double().mean()),
         "share p_max>0.999": float((p_max > 0.999).double().mean())}
    print(f"ladder D={c['D']} N={c['N']}: " + ", ".join(f"{k} {v:.4g}" for k, v in m.items()))
    assert m["max|s|"] <= 60 and m["max p_max"] > 0.999 and m["share p_max<0.3"] >= 1 / 3, m
    return m


# 2. one key that takes all the weight, at the edges of the 64-key stage and of its two 32-key tiles
DOMINANT = ((64, 63), (65, 64), (97, 96), (129, 128))            # (N, key)
DOMINANT_GAP = 25.0


@functools.lru_cache(maxsize=None)
def dominant_case(D, N, key):
    gen = _gen(5100 + N + D)
    u = torch.randn(D, generator=gen, dtype=torch.float64)
    u = (u / u.norm()).float()
    q = 0.5 * torch.randn(N, D, generator=gen) + 6.0 * u
    k = torch.randn(N, D, generator=gen)
    k[key] = 40.0 * math.sqrt(D / 32) * u
    v = torch.randn(N, D, generator=gen)
    dout = torch.randn(N, D, generator=gen)
    return {"qkv": torch.cat([q, k, v], dim=1), "dout": dout, "B": 1, "N": N, "heads": 1, "D": D, "key": key}


def dominant_conditions(c):
    """In float64 every query's score for `key` exceeds its next best by DOMINANT_GAP: the other keys' total weight is below
    N e^-25 < 2e-9, so out is v[key] to far below 2^-20 max|v|."""
    s, _p = scores64(c["qkv"], 1, c["N"], 1, c["D"])
    s = s[0, 0]
    top = s[:, c["key"]]
    rest = s.clone()
    rest[:, c["key"]] = -math.inf
    gap = float((top - rest.amax(dim=1)).min())
    v = c["qkv"][:, 2 * c["D"]:].double()
    off = float((K.attention_ref(c["qkv"], 1, c["N"], 1, c["D"], torch.float64) - v[c["key"]]).abs().max())
    print(f"dominant key D={c['D']} N={c['N']} key={c['key']}: smallest gap {gap:.4g}, max|s| {float(s.abs().max()):.4g}, "
          f"float64 max|out - v[key]| {off:.3g}")
    assert gap >= DOMINANT_GAP and off <= 2.0 ** -24 * float(v.abs().max()), (gap, off)
    return {"gap": gap, "off": off}


# 3, 4. NaN containment and the zero cotangent: B = 3, N = 65, D = 32, two heads; the NaN goes to (b = 1, row 40, head 0)
NAN_ATTN = dict(B=3, N=65, heads=2, D=32, b=1, row=40, head=0, d=3)


@functools.lru_cache(maxsize=None)
def nan_attention_case():
    a = NAN_ATTN
    gen = _gen(5200)
    M = a["heads"] * a["D"]
    qkv = torch.randn(a["B"] * a["N"], 3 * M, generator=gen)
    qkv[:, :M] *= 2.0
    return {"qkv": qkv, "dout": torch.randn(a["B"] * a["N"], M, generator=gen), **a}


def poisoned_qkv(c, which):
    """c's qkv with a NaN in the q ("q") or the k ("k") of (b, row, head)."""
    M = c["heads"] * c["D"]
    qkv = c["qkv"].clone()
    qkv[c["b"] * c["N"] + c["row"], {"q": 0, "k": M}[which] + c["head"] * c["D"] + c["d"]] = NAN
    return qkv


def check_attention_containment(run, c, eq):
    """run(qkv, dout) -> the five fields; eq(a, b): a is unchanged against b. The clean run against a NaN in q, then in k."""
    B, N, heads, D, b, row, head = (c[k] for k in ("B", "N", "heads", "D", "b", "row", "head"))
    clean = run(c["qkv"], c["dout"])
    assert all(bool(torch.isfinite(clean[f]).all()) for f in ATTN_FIELDS)
    per_head = lambda t: t.reshape(B, N, heads, D)                # (T, M) -> (b, n, head, d)
    rows = torch.arange(N, device=clean["out"].device) != row
    for which in ("q", "k"):
        got = run(poisoned_qkv(c, which).to(c["qkv"].device), c["dout"])
        inside = torch.zeros(B, heads, dtype=torch.bool, device=clean["out"].device)
        inside[b, head] = True
        for f in ("out", "dq", "dk", "dv"):
            g, w = per_head(got[f]).transpose(1, 2), per_head(clean[f]).transpose(1, 2)        # (b, head, n, d)
            assert eq(g[~inside], w[~inside]), (which, f, "outside")
        assert eq(got["lse"][~inside], clean["lse"][~inside]), (which, "lse outside")
        if which == "q":
            for f in ("out", "dq"):
                g, w = per_head(got[f])[b, :, head], per_head(clean[f])[b, :, head]               # (n, d)
                assert eq(g[rows], w[rows]), (f, "inside, other rows")
                assert bool(torch.isnan(g[row]).all()), (f, "the poisoned row")
            g, w = got["lse"][b, head], clean["lse"][b, head]
            assert eq(g[rows], w[rows]) and bool(torch.isnan(g[row])), "lse inside"


def check_attention_zero_cotangent(run, c):
    got = run(c["qkv"], torch.zeros_like(c["dout"]))
    for f in ("dq", "dk", "dv"):
        assert bool((got[f] == 0).all()), f


# ---- LayerNorm rows whose mean dwarfs their deviation ------------------------------------------------------------------------------------------
LN_T, LN_K, LN_N_OUT = 257, (32, 64, 512), 65
LN_ROWS = ((8.0, 1.0), (64.0, 1.0), (0.0, 1e-3))                 # (offset, deviation) by row % 3
CONST_ROWS = {10: 3.0, 11: 0.0, 12: -0.5, 64: 3.0, 200: -0.5}    # 6. constant rows beside an all-zero one, in the first tile and past it
ZERO_ROW = 11


@functools.lru_cache(maxsize=None)
def ln_rows_case(Kc, epi="plain", constant=False):
    """K.linear_inputs' weights with the rows of 5.; constant=True also holds the rows of 6. Also dn and g0 of the backward."""
    d = dict(K.linear_inputs(LN_T, Kc, LN_N_OUT, "ln", epi, seed=Kc))
    gen = _gen(5300 + Kc)
    kind = torch.arange(LN_T) % 3
    off, sd = (torch.tensor([r[i] for r in LN_ROWS])[kind][:, None] for i in (0, 1))
    x = off + sd * torch.randn(LN_T, Kc, generator=gen)
    if constant:
        for r, v in CONST_ROWS.items():
            x[r] = v
    d.update(x=x, dn=torch.randn(LN_T, Kc, generator=gen), g0=torch.randn(LN_T, Kc, generator=gen))
    return d


def ln_rows_conditions(d, constant=False):
    """Each kind of row is what it says in float64, and with constant rows the float64 LayerNorm gives beta exactly on them."""
    x = d["x"].double()
    mean, sd = x.mean(1), x.std(1, unbiased=False)
    kind = torch.arange(x.shape[0]) % 3
    keep = torch.ones(x.shape[0], dtype=torch.bool)
    if constant:
        keep[list(CONST_ROWS)] = False
    ratio = {}
    for i, (o, s) in enumerate(LN_ROWS):
        sel = keep & (kind == i)
        assert float((mean[sel] - o).abs().max()) <= s and float((sd[sel] / s - 1).abs().max()) <= 0.5, (o, s)
        ratio[(o, s)] = float((mean[sel].abs() / sd[sel]).max())
    print(f"LayerNorm rows K={x.shape[1]}: largest |mean| / sd per kind " + ", ".join(f"{k} {v:.3g}" for k, v in ratio.items()))
    assert ratio[LN_ROWS[1]] >= 32                               # a one-pass float32 variance would lose about mean^2 2^-24 of 1
    if constant:
        n = F.layer_norm(x, (x.shape[1],), d["gamma"].double(), d["beta"].double(), 1e-5)
        for r in CONST_ROWS:
            assert torch.equal(n[r], d["beta"].double()), r
    return ratio


def ln_moments(x):
    """{mean, rstd} (T, 2) of float32 rows with torch's own statements, as the backward tests take them."""
    return torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)


# ---- GroupNorm: a constant group and a step --------------------------------------------------------------------------------------------------
GN_B, GN_G, GN_C, GN_N = 2, 32, (32, 64), 2 * K.GN_CHUNK + 1
GN_CONST_GROUP = (5, 20)                                         # the constant group of batch element 0 and of 1
GN_CONST = 3.0


@functools.lru_cache(maxsize=None)
def gn_step_case(Cc):
    """x (B, C, N): N(0, 1) on the first chunk, 8 + N(0, 1) on the second, 100 at the one position of the third; one group per batch
    element holds GN_CONST everywhere. With it the weights of the gn-prologue product and the backward's dy and dout."""
    d = dict(K.linear_inputs(GN_B * GN_N, Cc, 65, "gn", "plain", seed=Cc))
    assert d["G"] == GN_G                                        # B, N and x are this case's own, not batch_of's split
    gen = _gen(5400 + Cc)
    x = torch.randn(GN_B, Cc, GN_N, generator=gen)
    x[:, :, K.GN_CHUNK:2 * K.GN_CHUNK] += 8.0
    x[:, :, 2 * K.GN_CHUNK:] = 100.0
    cpg = Cc // GN_G
    for b, g in enumerate(GN_CONST_GROUP):
        x[b, g * cpg:(g + 1) * cpg] = GN_CONST
    d.update(x=x, B=GN_B, N=GN_N, dy=torch.randn(GN_B, Cc, GN_N, generator=gen), dout=torch.randn(GN_B, Cc, GN_N, generator=gen))
    return d


def group_moments_ref(x, G):
    g = x.reshape(x.shape[0], G, -1)
    mean = g.mean(dim=2)
    return {"mean": mean, "m2": (g - mean[..., None]).square().sum(dim=2)}


def gn_step_conditions(d):
    """The constant groups' float64 moments are exactly (GN_CONST, 0); every other group's variance is mostly the step's."""
    m = group_moments_ref(d["x"].double(), GN_G)
    const = torch.zeros(GN_B, GN_G, dtype=torch.bool)
    for b, g in enumerate(GN_CONST_GROUP):
        const[b, g] = True
    assert bool((m["mean"][const] == GN_CONST).all()) and bool((m["m2"][const] == 0).all())
    var = m["m2"][~const] / (d["x"].shape[1] // GN_G * GN_N)
    print(f"GroupNorm step C={d['x'].shape[1]}: group means {float(m['mean'][~const].min()):.3g} .. {float(m['mean'][~const].max()):.3g}, "
          f"variances {float(var.min()):.3g} .. {float(var.max()):.3g}")
    assert float(var.min()) > 15 and 3 < float(m["mean"][~const].min()) and float(m["mean"][~const].max()) < 6
    return const


# ---- the GEGLU epilogue with the gate in both tails ---------------------------------------------------------------------------------------------
GATE_SPAN = 12.0


@functools.lru_cache(maxsize=None)
def geglu_tails_case(T=65, Kc=64, n_out=65):
    """K.linear_inputs for LN -> GEGLU with the gate half as the backward's wide_gate case builds it: weights x 0.02, bias a ramp."""
    d = dict(K.linear_inputs(T, Kc, n_out, "ln", "geglu", seed=5500))
    d["w"], d["bias"] = d["w"].clone(), d["bias"].clone()
    d["w"][n_out:] *= 0.02
    d["bias"][n_out:] = torch.linspace(-GATE_SPAN, GATE_SPAN, n_out)
    return d


def geglu_gate64(d):
    """The float64 gate pre-activation (T, n_out)."""
    t = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    n = F.layer_norm(t["x"], (t["x"].shape[1],), t["gamma"], t["beta"], 1e-5)
    return F.linear(n, t["w"], t["bias"]).chunk(2, dim=-1)[1]


def geglu_tails_conditions(d):
    """The float64 gate spans below -11 and above 11; the bands are the columns whose gate lies in |g| <= 4, and in g > 4, in every row."""
    g = geglu_gate64(d).cpu()
    mid, high = (g.abs() <= 4).all(dim=0), (g > 4).all(dim=0)
    print(f"GEGLU tails: gate {float(g.min()):.4g} .. {float(g.max()):.4g}, columns with |gate| <= 4: {int(mid.sum())}, with gate > 4: {int(high.sum())}")
    assert float(g.min()) < -11 and float(g.max()) > 11 and int(mid.sum()) >= 8 and int(high.sum()) >= 8
    return mid, high


# ---- NaN containment of the row kernels: T = 99 rows of three batch elements, so rows 33 .. 63 share the first tile with batch element 0 ------
NAN_T, NAN_K, NAN_N_OUT, NAN_ROWS = 99, 64, 65, (40, 63, 64)
NAN_CF = dict(b=1, c=37, n=5)                                    # where the channel-first forms take their NaN


@functools.lru_cache(maxsize=None)
def nan_linear_case(pro, epi):
    d = K.linear_inputs(NAN_T, NAN_K, NAN_N_OUT, pro, epi, seed=5600)
    assert (d["B"], d["N"]) == (3, 33)
    return d


def by_row(y, epi, B, N):
    """A product's output as (T, n_out) rows, whatever the epilogue's layout."""
    return y.permute(0, 2, 1).reshape(B * N, -1) if epi == "bias_res_cf" else y


def check_linear_containment(run, pro, epi, eq, device="cpu"):
    """run(d, x) -> the product of case d on x in its place. Rows: a NaN in row r leaves every other output row unchanged and row r
    non-finite. Channel first (gn): a NaN at x[b, c, n] leaves the other batch elements unchanged and makes b non-finite."""
    d = to(nan_linear_case(pro, epi), device)
    B, N = d["B"], d["N"]
    clean = by_row(run(d, d["x"]), epi, B, N)
    assert bool(torch.isfinite(clean).all())
    if pro == "gn":
        x = d["x"].clone()
        x[NAN_CF["b"], NAN_CF["c"], NAN_CF["n"]] = NAN
        got = by_row(run(d, x), epi, B, N).reshape(B, N, -1)
        w = clean.reshape(B, N, -1)
        assert eq(got[0], w[0]) and eq(got[2], w[2]) and not bool(torch.isfinite(got[1]).any()), (pro, epi)
        return
    for r in NAN_ROWS:
        x = d["x"].clone()
        x[r, 7] = NAN
        got = by_row(run(d, x), epi, B, N)
        others = torch.arange(NAN_T, device=got.device) != r
        assert eq(got[others], clean[others]) and not bool(torch.isfinite(got[r]).any()), (pro, epi, r)


@functools.lru_cache(maxsize=None)
def nan_rows_backward_case():
    """The row operands of layernorm_backward (dn, x, mom, g) and of geglu_backward (g, h, mom) at T = 99, K = M = 64."""
    gen = _gen(5700)
    r = lambda *s: torch.randn(*s, generator=gen)
    T, M = NAN_T, NAN_K
    x = r(T, M) + 0.3
    return {"x": x, "dn": r(T, M), "g": r(T, M), "mom": ln_moments(x), "gamma": 1 + 0.1 * r(M), "beta": 0.1 * r(M), "w1": r(8 * M, M) * M ** -0.5,
            "b1": 0.1 * r(8 * M), "w2": r(M, 4 * M) * (4 * M) ** -0.5}


def check_rows_containment(run, operands, d, eq):
    """run(**operands) -> (T, .) rows. A NaN in row r of any one operand changes row r alone, and makes it hold a non-finite value."""
    clean = run(**{k: d[k] for k in operands})
    assert bool(torch.isfinite(clean).all())
    for name in operands:
        for r in NAN_ROWS:
            args = {k: d[k] for k in operands}
            args[name] = args[name].clone()
            args[name][r, 1] = NAN
            got = run(**args)
            others = torch.arange(NAN_T, device=got.device) != r
            assert eq(got[others], clean[others]) and not bool(torch.isfinite(got[r]).all()), (name, r)


@functools.lru_cache(maxsize=None)
def nan_groups_case(Cc=64):
    gen = _gen(5800)
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"x": r(3, Cc, 33) + 0.5, "dy": r(3, Cc, 33), "dout": r(3, Cc, 33), "gamma": 1 + 0.1 * r(Cc), "beta": 0.1 * r(Cc), "G": 32}


def check_groups_containment(run, d, eq, poison, per_group):
    """run(d) -> (B, C, N) or, per_group, (B, G, .). A NaN at `poison`[b = 1, c, n] leaves batch elements 0 and 2 and the other groups
    of batch element 1 unchanged, and reaches its own group."""
    clean = run(d)
    assert bool(torch.isfinite(clean).all())
    p = dict(d)
    p[poison] = d[poison].clone()
    b, c, n = NAN_CF["b"], NAN_CF["c"], NAN_CF["n"]
    p[poison][b, c, n] = NAN
    got = run(p)
    G, cpg = d["G"], d["x"].shape[1] // d["G"]
    grp = lambda t: t if per_group else t.reshape(t.shape[0], G, -1)
    g, w = grp(got), grp(clean)
    others = torch.arange(G, device=g.device) != c // cpg
    assert eq(g[0], w[0]) and eq(g[2], w[2]) and eq(g[b][others], w[b][others]) and not bool(torch.isfinite(g[b, c // cpg]).all())


# ---- the whole stack: T = 195 rows of three batch elements, tiles straddle them ------------------------------------------------------------------
STACK = dict(C=64, heads=2, D=32, layers=2, attn2=True, B=3, N=65)
STACK_NAN = (1, 5, 17)


@functools.lru_cache(maxsize=None)
def stack_inputs():
    s = STACK
    x = K.make_x(s["B"], s["C"], s["N"], seed=5900)
    dout = torch.randn(s["B"], s["C"], s["N"], generator=_gen(5901))
    return x, dout


def stack_module(device="cpu", dtype=torch.float32):
    s = STACK
    return K.make_module(s["C"], s["heads"], s["D"], s["layers"], attn2=s["attn2"], seed=59, device=device, dtype=dtype).requires_grad_(False)


def check_stack(run, x, dout, eq):
    """run(x, dout) -> (out, dx). 11.: a NaN in x[1] makes out[1] NaN everywhere and leaves out and dx of batch elements 0 and 2
    unchanged; a NaN in dout[1] leaves dx[0] and dx[2] unchanged and reaches dx[1]. 12.: dout = 0 gives dx == 0."""
    out, dx = run(x, dout)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    xn = x.clone()
    xn[STACK_NAN] = NAN
    o2, d2 = run(xn, dout)
    assert eq(o2[0], out[0]) and eq(o2[2], out[2]) and bool(torch.isnan(o2[1]).all())
    assert eq(d2[0], dx[0]) and eq(d2[2], dx[2])
    dn = dout.clone()
    dn[STACK_NAN] = NAN
    o3, d3 = run(x, dn)
    assert eq(o3, out) and eq(d3[0], dx[0]) and eq(d3[2], dx[2]) and bool(torch.isnan(d3[1]).any())
    _o, d0 = run(x, torch.zeros_like(dout))
    assert bool((d0 == 0).all())
