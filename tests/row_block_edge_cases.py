"""Shared by tests/test_row_block_edges_cpu.py and tests/test_gpu_row_block_edges.py: the value edges of the four row-tile blocks that
carry a point's features to the rasteriser — the vertex MLPs (include/gh_vert.h), the point conditioning (include/gh_cond.h), the row work
around the interaction attention (include/gh_attn_rows.h) and the Gaussian trunk with its head (include/gh_trunk.h). Their shapes are
swept by their own files; here the shapes are tame and the data is what a kernel can get wrong: LayerNorm rows whose mean dwarfs their
deviation, one column that holds all of a row's variance, cond's combination of the row's moments with the folded ones, hidden units
that sit exactly on the ReLU's kink, activations deep in their tails, a NaN next to rows that must not see it, and cotangents that are
exactly zero.

The inputs, runners and restatements are the blocks' own (vert_cases.make_inputs / run, cond_cases.make_case / run,
attn_block_cases, gs_trunk_cases.make / run, and the packages' `_ref` functions and ops="torch" paths); this module only edits the
tensors they return. Every generator draws on the CPU from a seeded generator and returns float32 tensors; every value case states, as
`*_conditions`, what it promises about its own float64 reference, prints the measured figures and asserts them. A case is a dict; its
"groups" are boolean masks over the rows (or, for a band of an activation, over a field's elements), and a test judges every field on
every group on its own, by tests/fit_cases.three_way, so that an edge group's bound cannot excuse a kernel that is wrong on the tame
rows, or the reverse. `python -m tests.row_block_edge_cases` prints every condition: the seeds were chosen with it."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from guassianhand_amd import attn_block as AB
from guassianhand_amd import vert_mlp as V
from tests import attn_block_cases as AC
from tests import cond_cases as CM
from tests import gs_trunk_cases as TC
from tests import vert_cases as VM

NAN = float("nan")
F64 = torch.float64
GUARD = TC.GUARD
LN_KINDS = ((8.0, 1e-3), (64.0, 1e-3), (-64.0, 1e-3), (64.0, 1.0))      # (mean, deviation) of an edge row
TILE_ROWS = (0, 31, 32, 63, 64)                                         # both ends of a tile's two half-waves, and the next tile's first row
BIG = 1e4                                                               # the dominant column's entry
BANDS = ("mid", "far+", "far-", "deep+", "deep-")                       # |v| <= 4, 4 < |v| <= 20, |v| > 20, by sign
MIN_BAND = 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def edge_rows(P):
    """TILE_ROWS and the last row (the tail tile's), as far as P holds them."""
    return tuple(sorted({r for r in TILE_ROWS + (P - 1,) if r < P}))


def row_groups(P, rows, name="edge"):
    m = torch.zeros(P, dtype=torch.bool)
    m[list(rows)] = True
    return {name: m, "tame": ~m}


def split(res, fields, groups, whole=()):
    """{field[group]: the field's elements under the group's mask} for fields x groups, and the `whole` fields as they are."""
    out = {f: res[f] for f in whole}
    for f in fields:
        for g, sel in groups.items():
            out[f"{f}[{g}]"] = res[f][sel.to(res[f].device)].contiguous()
    return out


def bands(v):
    """BANDS as masks of v's shape, by the float64 pre-activation v."""
    a = v.abs()
    return {"mid": a <= 4, "far+": (a > 4) & (a <= 20) & (v > 0), "far-": (a > 4) & (a <= 20) & (v < 0), "deep+": (a > 20) & (v > 0),
            "deep-": (a > 20) & (v < 0)}


def assert_bands(tag, masks, names=BANDS):
    n = {k: int(masks[k].sum()) for k in names}
    print(f"{tag}: elements per band " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert all(v >= MIN_BAND for v in n.values()), (tag, n)
    return n


def assert_reaches(tag, out, rows):
    """The float64 output of the edge rows is finite and differs between them by more than the three-way rule's floor."""
    o = out.reshape(out.shape[0], -1)[list(rows)]
    spread, top = float((o.amax(0) - o.amin(0)).max()), float(o.abs().max())
    print(f"{tag}: float64 output of the edge rows: max| | {top:.4g}, largest spread of a column across them {spread:.4g}")
    assert bool(torch.isfinite(o).all()) and spread > 2.0 ** -20 * top, (tag, spread, top)


def assert_row_kind(tag, z, m, s):
    """Rows z (n, D) in float64 have mean m to within s and deviation s to within half of it; returns the largest std / |mean|."""
    mean, sd = z.mean(1), z.std(1, unbiased=False)
    ratio = float((sd / mean.abs()).max())
    print(f"{tag}: rows ({m:g}, {s:g}): mean {float(mean.min()):.6g} .. {float(mean.max()):.6g}, deviation {float(sd.min()):.4g} .. "
          f"{float(sd.max()):.4g}, largest std / |mean| {ratio:.3g}")
    assert float((mean - m).abs().max()) <= s and float((sd / s - 1).abs().max()) <= 0.5, (tag, m, s)
    assert ratio <= 1.5 * s / abs(m)
    return ratio


def kink_margin(tag, v, units):
    """v (rows, units) float64: the listed units are exactly 0 on every row; every other unit keeps the project's margin from 0."""
    keep = torch.ones(v.shape[1], dtype=torch.bool)
    keep[list(units)] = False
    assert bool((v[:, list(units)] == 0).all()), tag
    w = v[:, keep]
    m, both = float(w.abs().min() / w.abs().max()), bool((w > 0).any() and (w < 0).any())
    print(f"{tag}: units {tuple(units)} are exactly 0; the others' relu margin {m:.3e} (guard {GUARD:.3e}), both sides: {both}")
    assert m > GUARD and both, (tag, m)
    return m


MEAN_ULPS = 4


def mean_reach(tag, z, gamma, w1, pre, eps=1e-6):
    """A float32 mean of D values near m is known to a few ulp(m), whatever the order of its sum; on a row whose deviation is far
    smaller that is a visible share of every centred column: an error of MEAN_ULPS ulp(|mean|) moves each normalised column by that
    times rstd, all the same way, and unit j's pre-activation by that times |sum_k W1[j, k] gamma[k]|. The float32 statements and a
    kernel may each land anywhere within it, so a unit that close to 0 takes its ReLU gate by the sum's order, not by a fault, and
    its gradient jumps by a term of order 1: no unit of the rows z (float64, with their pre-activations `pre`) may lie within that
    reach of its kink. The case's seed is chosen so. Returns the smallest |pre| / reach."""
    mean, rstd = z.mean(1), (z.var(1, unbiased=False) + eps).rsqrt()
    reach = (MEAN_ULPS * 2.0 ** (torch.floor(torch.log2(mean.abs())) - 23) * rstd)[:, None] * (w1.double() * gamma.double()).sum(1).abs()[None, :]
    live = reach > 0
    worst = float((pre.abs()[live] / reach[live]).min())
    print(f"{tag}: a {MEAN_ULPS} ulp error of the mean reaches up to {float(reach.max()):.3e} in a pre-activation; smallest |pre| / reach {worst:.3g}")
    assert worst > 1, (tag, worst)
    return worst


def dominant_columns(D):
    """Column 0 and the last column of each wave's share of ghr_moments (wave w sums k = w mod 4): D - 4 .. D - 1."""
    cols = (0, D - 4, D - 3, D - 2, D - 1)
    assert {c % 4 for c in cols[1:]} == {0, 1, 2, 3}
    return cols


def assert_dominant(tag, z, cols):
    """Row i of z (float64) holds BIG at cols[i]: of the row's sum of squared deviations that one entry holds all that one of D entries
    can, (D - 1) / D, to within a thousandth."""
    d2 = (z - z.mean(1, keepdim=True)).square()
    share = d2[torch.arange(z.shape[0]), list(cols)] / d2.sum(1)
    print(f"{tag}: dominant columns {tuple(cols)} (k mod 4 = {tuple(c % 4 for c in cols)}), smallest share of m2 {float(share.min()):.6f}")
    assert float(share.min()) > 0.999 * (1 - 1 / z.shape[1]), tag


# ---- vert -------------------------------------------------------------------------------------------------------------------------------
# P = 130 is two tiles and a tail of two rows; Cf = 165 is the first width whose backward runs 32 rows per workgroup, two lanes a row
VERT_SHAPES = ((130, 131, 1), (130, 131, 3), (65, 165, 3))             # (P, Cf, K)
VERT_TAIL_SHAPES = ((130, 131, 1), (130, 131, 3), (130, 165, 1))       # (130 rows: five bands of eight elements do not fit 65 values)
VERT_UNITS = lambda Cf: (1, (Cf + 3) // 4 - 1)                          # the two hidden units on the kink: bias +0.0 and -0.0
VERT_TAILS = {1: ((45.0,), (0.0,)), 3: ((45.0, 45.0, 45.0), (12.0, -12.0, 0.0))}  # K: (deviation, centre) of the final pre-activation's columns
VERT_TAILS_SEED = {(130, 131, 1): 50, (130, 131, 3): 50, (130, 165, 1): 50}
VERT_FIELDS = ("out", "grad_x", "grad_pts")
# the edge rows' seeds where the first one tried puts a unit within mean_reach of its kink
VERT_LN_SEED = {(130, 131, 1, 0): 7000, (130, 131, 1, 1): 7013, (130, 131, 1, 2): 7004, (130, 131, 3, 1): 7016, (130, 131, 3, 2): 7005,
                (65, 165, 3, 1): 7011, (65, 165, 3, 2): 7002}
VERT_KINK_ROWS_SEED = {(130, 131, 1): 7501, (130, 131, 3): 7568, (65, 165, 3): 7509}


def _vert(P, Cf, K, seed):
    inputs, cot = VM.make_inputs("cpu", P, Cf, K, seed=seed)
    return {"inputs": inputs, "cot": cot, "P": P, "Cf": Cf, "K": K, "groups": {"tame": torch.ones(P, dtype=torch.bool)}}


def _vert_set_rows(c, rows, z):
    c["inputs"][0][list(rows)], c["inputs"][1][list(rows)] = z[:, :c["Cf"]], z[:, c["Cf"]:]


def vert_z64(c):
    return torch.cat([c["inputs"][0], c["inputs"][1]], dim=1).double()


def vert_run(mode, c, device="cpu"):
    return VM.run(mode, [t.to(device) for t in c["inputs"]], c["cot"].to(device), c["K"])


@functools.lru_cache(maxsize=None)
def vert_ln_case(P, Cf, K, kind):
    c = _vert(P, Cf, K, seed=20 + kind)
    m, s = LN_KINDS[kind]
    rows = edge_rows(P)
    _vert_set_rows(c, rows, m + s * torch.randn(len(rows), Cf + 3, generator=_gen(VERT_LN_SEED.get((P, Cf, K, kind), 6000 + kind + Cf))))
    c.update(rows=rows, groups=row_groups(P, rows), kind=kind)
    return c


def vert_ln_conditions(c):
    tag = f"vert LN P={c['P']} Cf={c['Cf']} K={c['K']}"
    assert_row_kind(tag, vert_z64(c)[list(c["rows"])], *LN_KINDS[c["kind"]])
    mean_reach(tag, vert_z64(c)[list(c["rows"])], c["inputs"][2], c["inputs"][4], vert_pre1(c)[list(c["rows"])])
    ref = vert_run("f64", c)
    assert_reaches(tag, ref["out"], c["rows"])
    g = ref["grad_x"][list(c["rows"])]
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


@functools.lru_cache(maxsize=None)
def vert_dominant_case(P, Cf, K):
    c = _vert(P, Cf, K, seed=30)
    rows, cols = edge_rows(P), dominant_columns(Cf + 3)
    z = vert_z64(c)[list(rows)].float()
    at = tuple(cols[i % len(cols)] for i in range(len(rows)))
    z[torch.arange(len(rows)), list(at)] = BIG
    _vert_set_rows(c, rows, z)
    c.update(rows=rows, cols=at, groups=row_groups(P, rows, "dominant"))
    return c


def vert_dominant_conditions(c):
    tag = f"vert dominant P={c['P']} Cf={c['Cf']} K={c['K']}"
    assert set(c["cols"]) == set(dominant_columns(c["Cf"] + 3))
    assert_dominant(tag, vert_z64(c)[list(c["rows"])], c["cols"])
    assert_reaches(tag, vert_run("f64", c)["out"], c["rows"])


VERT_KINK_SEED = {(130, 131, 1): 41, (130, 131, 3): 40, (65, 165, 3): 40}


@functools.lru_cache(maxsize=None)
def vert_kink_case(P, Cf, K, cut=False):
    """fc1's units VERT_UNITS have a zero weight row and the biases +0.0 and -0.0; the edge rows are LN_KINDS[1]'s. cut: fc2's
    columns for those units are zero as well."""
    c = _vert(P, Cf, K, seed=VERT_KINK_SEED[(P, Cf, K)])
    rows, units = edge_rows(P), VERT_UNITS(Cf)
    m, s = LN_KINDS[1]
    _vert_set_rows(c, rows, m + s * torch.randn(len(rows), Cf + 3, generator=_gen(VERT_KINK_ROWS_SEED.get((P, Cf, K), 6100 + Cf))))
    c["inputs"][4][list(units)] = 0.0
    c["inputs"][5][units[0]], c["inputs"][5][units[1]] = 0.0, -0.0
    if cut:
        c["inputs"][6][:, list(units)] = 0.0
    c.update(rows=rows, units=units, groups=row_groups(P, rows))
    return c


def vert_pre1(c):
    """fc1's float64 pre-activation: the block's first two statements."""
    g, b, w1, b1 = (t.double() for t in c["inputs"][2:6])
    z = vert_z64(c)
    return F.linear(F.layer_norm(z, (z.shape[1],), g, b, 1e-6), w1, b1)


def vert_kink_conditions(c):
    tag = f"vert kink P={c['P']} Cf={c['Cf']} K={c['K']}"
    assert bool(torch.equal(c["inputs"][5][list(c["units"])].signbit(), torch.tensor([False, True])))
    mean_reach(tag, vert_z64(c)[list(c["rows"])], c["inputs"][2], c["inputs"][4], vert_pre1(c)[list(c["rows"])])
    return kink_margin(tag, vert_pre1(c), c["units"])


def vert_pre_out(c):
    """The float64 pre-activation of the epilogue, from the restatement itself: with fc's weight and bias times 2^-10 (exact) its
    sigmoid stays near 1/2, where the logit gives the scaled pre-activation back to float64 rounding."""
    p = [t.double() for t in c["inputs"][2:]]
    p[6], p[7] = p[6] * 2.0 ** -10, p[7] * 2.0 ** -10
    return torch.logit(V._vert_block_ref(c["inputs"][0], c["inputs"][1], p, act="sigmoid", eps=1e-6, acc=F64)) * 2.0 ** 10


@functools.lru_cache(maxsize=None)
def vert_tails_case(P, Cf, K):
    """LayerNorm takes a row's scale away, so the epilogue is driven through the head alone: each row of fc is scaled, and fc_bias set,
    so that its column of the float64 pre-activation has VERT_TAILS' deviation and centre over the P rows, which spreads it over +-12,
    +-40 and +-100. Groups: out by the band of its own element; the gradients by the band of the row's column nearest 0, whose
    derivative (1 - s) s or 1 - t^2 is the row's largest — with its sign where there is one column, without where there are three."""
    c = _vert(P, Cf, K, seed=VERT_TAILS_SEED[(P, Cf, K)])
    c["inputs"][9].zero_()
    u = vert_pre_out(c)
    sd, centre = (torch.tensor(t, dtype=F64) for t in VERT_TAILS[K])
    a = sd / u.std(0)
    c["inputs"][8] *= a.float()[:, None]
    c["inputs"][9].copy_((centre - a * u.mean(0)).float())
    v = vert_pre_out(c)
    near = v.gather(1, v.abs().argmin(dim=1, keepdim=True))[:, 0]
    b = bands(near)
    rows = b if K == 1 else {"mid": b["mid"], "far": b["far+"] | b["far-"], "deep": b["deep+"] | b["deep-"]}
    c.update(pre=v, groups_out=bands(v), groups=rows)
    return c


def vert_tails_conditions(c):
    tag = f"vert tails P={c['P']} Cf={c['Cf']} K={c['K']}"
    v = c["pre"]
    print(f"{tag}: float64 pre-activation {float(v.min()):.4g} .. {float(v.max()):.4g}")
    assert float(v.min()) < -89 and float(v.max()) > 89          # expf overflows float32 past 88.7
    assert_bands(tag + " out", c["groups_out"])
    return assert_bands(tag + " rows", c["groups"], tuple(c["groups"]))


# ---- cond -------------------------------------------------------------------------------------------------------------------------------
# B = 2, N = 65: the second tile holds row 64 of batch element 0 and rows 0 .. 62 of batch element 1
COND_B, COND_N = 2, 65
COND_LN = tuple(("full", k) for k in range(4)) + (("de1", 1), ("l8", 1))
COND_COMBOS = ("zero", "m64", "d50", "de1_100", "xyz1_l8")
COND_UNITS = (1, 50)
COND_FIELDS = ("out", "grad_code")


def _cond(layout, seed):
    t, params, cot, L = CM.make_case("cpu", COND_B, COND_N, layout, seed=seed)
    P = COND_B * COND_N
    return {"t": t, "params": params, "cot": cot, "L": L, "layout": layout, "P": P, "rows": edge_rows(P), "groups": row_groups(P, edge_rows(P))}


def cond_run(mode, c, device="cpu"):
    t = {k: (None if v is None else v.to(device)) for k, v in c["t"].items()}
    res = CM.run(mode, (t, [p.to(device) for p in c["params"]], c["cot"].to(device), c["L"]))
    return {k: v.reshape(c["P"], -1) for k, v in res.items()}


def _code_rows(c):
    return c["t"]["code"].view(c["P"], -1)


def cond_dense64(c):
    """The rows as the reference's torch.cat gives them, in float64 (P, Dv + De), and Dv."""
    rows = CM.point_rows(c["t"], c["L"])
    return rows.dense(F64).reshape(c["P"], -1), rows.Dv


@functools.lru_cache(maxsize=None)
def cond_ln_case(layout, kind):
    """The code columns of the edge rows, and both batch elements' broadcast vectors, have LN_KINDS[kind]'s mean and deviation. The
    encodings' columns stay within +-1, so the whole row's deviation is of the mean's order: what is large is every sum the kernel forms.
    This family cannot tell a one-pass m2 (sum x^2 - n mean^2) from the centred one: ghr_moments sees the row's own Dv columns only,
    of which 51 to 91 are those encodings, so their mean^2 / variance never passes 0.64 and the one-pass form loses two or three ulp,
    not the variance. It holds the pairwise combination with (m_e, M_e) and the sums' sizes; vert and the attention block hold m2."""
    c = _cond(layout, seed=20 + kind)
    m, s = LN_KINDS[kind]
    gen = _gen(6200 + kind + len(layout))
    _code_rows(c)[list(c["rows"])] = m + s * torch.randn(len(c["rows"]), _code_rows(c).shape[1], generator=gen)
    c["t"]["e"] = m + s * torch.randn(c["t"]["e"].shape, generator=gen)
    c["kind"] = kind
    return c


def cond_pre1(c):
    g, b, w1, b1 = (t.double() for t in c["params"][:4])
    z, _ = cond_dense64(c)
    return z, F.linear(F.layer_norm(z, (z.shape[1],), g, b, 1e-6), w1, b1)


def cond_ln_conditions(c):
    tag = f"cond LN {c['layout']}"
    z, pre = cond_pre1(c)
    mean_reach(tag, z[list(c["rows"])], c["params"][0], c["params"][2], pre[list(c["rows"])])
    m, s = LN_KINDS[c["kind"]]
    assert_row_kind(tag + " code", _code_rows(c)[list(c["rows"])].double(), m, s)
    if c["t"]["e"].shape[-1] > 1:
        assert_row_kind(tag + " broadcast", c["t"]["e"].reshape(COND_B, -1).double(), m, s)
    z, _ = cond_dense64(c)
    z = z[list(c["rows"])]
    print(f"{tag}: whole edge rows: mean {float(z.mean(1).min()):.4g} .. {float(z.mean(1).max()):.4g}, deviation "
          f"{float(z.std(1, unbiased=False).min()):.4g} .. {float(z.std(1, unbiased=False).max()):.4g}")
    assert_reaches(tag, cond_run("f64", c)["out"], c["rows"])


@functools.lru_cache(maxsize=None)
def cond_combo_case(kind):
    """The broadcast vector of COND_COMBOS against rows whose code columns have mean 8 (the edge rows) and mean 0 (the others).
    xyz1_l8: the edge rows' |xyz| reach 1 at L = 8 instead, so that the sines' arguments reach pi 2^7 = 402."""
    layout = {"de1_100": "de1", "xyz1_l8": "l8"}.get(kind, "full")
    c = _cond(layout, seed=30 + COND_COMBOS.index(kind))
    gen = _gen(6300 + COND_COMBOS.index(kind))
    e = c["t"]["e"]
    if kind == "xyz1_l8":
        xyz = c["t"]["xyz"].view(c["P"], 3)
        xyz[list(c["rows"])] = 2 * torch.rand(len(c["rows"]), 3, generator=gen) - 1
        xyz[c["rows"][0], 0], xyz[c["rows"][-1], 2] = 1.0, -1.0
    else:
        _code_rows(c)[list(c["rows"])] += 8.0
        if kind == "zero":
            e.zero_()
        elif kind == "m64":
            e.copy_(64.0 + 1e-3 * torch.randn(e.shape, generator=gen))
        elif kind == "d50":
            d = 50.0 * torch.randn(e.shape, generator=gen, dtype=F64)
            e.copy_((d - d.mean(-1, keepdim=True)).float())
        else:
            e.fill_(100.0)
    c["kind"] = kind
    return c


def cond_delta_share(c):
    """Per row, from the float64 moments of the row's own columns (m_v, M_v) and of its batch element's broadcast vector (m_e, M_e):
    the share of delta^2 Dv De / D, delta = m_e - m_v, in M = M_v + M_e + delta^2 Dv De / D."""
    z, Dv = cond_dense64(c)
    v, e = z[:, :Dv], z[:, Dv:]
    De = e.shape[1]
    m_v, m_e = v.mean(1), e.mean(1)
    M_v, M_e = (v - m_v[:, None]).square().sum(1), (e - m_e[:, None]).square().sum(1)
    cross = (m_e - m_v).square() * (Dv * De / (Dv + De))
    M = M_v + M_e + cross
    assert float(((z - z.mean(1, keepdim=True)).square().sum(1) / M - 1).abs().max()) < 1e-12      # (the combination is the row's own m2)
    return cross / M, M_e


def cond_combo_conditions(c):
    kind, tag = c["kind"], f"cond combination {c['kind']}"
    share, M_e = cond_delta_share(c)
    edge = share[list(c["rows"])]
    print(f"{tag}: share of the delta^2 term in M: all rows {float(share.min()):.3e} .. {float(share.max()):.3e}, edge rows "
          f"{float(edge.min()):.3e} .. {float(edge.max()):.3e}; rows below 1e-6: {int((share < 1e-6).sum())}; M_e {float(M_e.min()):.4g} .. {float(M_e.max()):.4g}")
    if kind == "zero":
        assert float(M_e.max()) == 0.0
    if kind == "m64":
        assert float(share.min()) > 0.99
    if kind == "d50":
        assert int((share < 1e-6).sum()) >= MIN_BAND
    if kind == "xyz1_l8":
        xyz = c["t"]["xyz"].view(c["P"], 3)[list(c["rows"])]
        arg = float(xyz.abs().max()) * math.pi * 2 ** (c["L"] - 1)
        print(f"{tag}: largest |xyz| of the edge rows {float(xyz.abs().max()):.4g}, largest sine argument {arg:.4g}")
        assert c["L"] == 8 and float(xyz.abs().max()) == 1.0 and arg > 400
    assert_reaches(tag, cond_run("f64", c)["out"], c["rows"])
    return share


COND_KINK_SEED = 40


@functools.lru_cache(maxsize=None)
def cond_kink_case(cut=False):
    c = _cond("full", seed=COND_KINK_SEED)
    m, s = LN_KINDS[1]
    _code_rows(c)[list(c["rows"])] = m + s * torch.randn(len(c["rows"]), _code_rows(c).shape[1], generator=_gen(6400))
    u = COND_UNITS
    c["params"][2][list(u)] = 0.0
    c["params"][3][u[0]], c["params"][3][u[1]] = 0.0, -0.0
    if cut:
        c["params"][4][:, list(u)] = 0.0
    c["units"] = u
    return c


def cond_kink_conditions(c):
    z, pre = cond_pre1(c)
    mean_reach("cond kink", z[list(c["rows"])], c["params"][0], c["params"][2], pre[list(c["rows"])])
    return kink_margin("cond kink", pre, c["units"])


# ---- the attention block ----------------------------------------------------------------------------------------------------------------
# two batch elements of V = 65: the second tile of the 130 rows holds row 64 of the first and rows 0 .. 62 of the second
ATTN_SHAPES = ((131, None, 4), (37, 50, 1))                            # (F, hid, heads); hid = 50 is no multiple of the mask's 32-bit word
ATTN_BS, ATTN_V = 2, 65
ATTN_FIELDS = ("out", "grad_x")
ATTN_NAN = dict(V=80, listed=65, b=0, pos=64, col=5)


def _attn(f_dim, hid, heads, seed, V=ATTN_V):
    m = AC.make_module(f_dim, hid=hid, n_heads=heads, seed=seed)
    x, cot = AC.make_input(ATTN_BS, V, f_dim, seed=seed)
    P = ATTN_BS * V
    return {"params": [p.detach().clone() for p in AB.module_params(m)], "x": x, "cot": cot, "heads": heads, "F": f_dim, "hid": m.ff.fc1.out_features,
            "P": P, "rows": edge_rows(P), "groups": row_groups(P, edge_rows(P))}


def attn_run(mode, c, device="cpu", idx=None, x=None, cot=None):
    """{out, grad_x} as (BS V, F) rows. mode: 'f64' | 'torch32' (attn_block_ref) | 'kernel' (attn_block)."""
    P, H = [p.to(device) for p in c["params"]], c["heads"]
    idx = None if idx is None else idx.to(device)
    fn = {"kernel": lambda t: AB.attn_block(t, P, n_heads=H, idx=idx), "torch32": lambda t: AB.attn_block_ref(t, P, n_heads=H, idx=idx),
          "f64": lambda t: AB.attn_block_ref(t, P, n_heads=H, idx=idx, acc=F64)}[mode]
    y, g = AC.grad_run(fn, (c["x"] if x is None else x).to(device), (c["cot"] if cot is None else cot).to(device), F64 if mode == "f64" else None)
    return {"out": y.reshape(-1, c["F"]), "grad_x": g.reshape(-1, c["F"])}


def attn_y64(c):
    """The float64 y = x + fc(attention), the input of the second LayerNorm: the restatement with ff.fc2 zeroed returns y + 0."""
    P = list(c["params"])
    P[14], P[15] = torch.zeros_like(P[14]), torch.zeros_like(P[15])
    return AB.attn_block_ref(c["x"], P, n_heads=c["heads"], acc=F64).reshape(c["P"], -1)


def _x_rows(c):
    return c["x"].view(c["P"], -1)


@functools.lru_cache(maxsize=None)
def attn_ln_case(shape, kind):
    c = _attn(*shape, seed=20 + kind)
    m, s = LN_KINDS[kind]
    _x_rows(c)[list(c["rows"])] = m + s * torch.randn(len(c["rows"]), c["F"], generator=_gen(6500 + kind + c["F"]))
    c["kind"] = kind
    return c


def attn_ln_conditions(c):
    """LN1 sees x's rows as they are. LN2 sees y = x + fc(attention): the mean is x's, the deviation is the attention's output's, and
    the condition there is that |mean| / deviation of the float64 y stays at or above 4 (mean 8) and 32 (mean +-64)."""
    tag = f"attn LN F={c['F']} hid={c['hid']}"
    m, s = LN_KINDS[c["kind"]]
    assert_row_kind(tag + " x", _x_rows(c)[list(c["rows"])].double(), m, s)
    y = attn_y64(c)[list(c["rows"])]
    ratio = float((y.mean(1).abs() / y.std(1, unbiased=False)).min())
    print(f"{tag}: y rows: mean {float(y.mean(1).min()):.5g} .. {float(y.mean(1).max()):.5g}, deviation {float(y.std(1, unbiased=False).min()):.4g} .. "
          f"{float(y.std(1, unbiased=False).max()):.4g}, smallest |mean| / deviation {ratio:.4g}")
    assert ratio >= abs(m) / 2
    yy, pre = attn_pre1(c)
    mean_reach(tag + " LN2", yy[list(c["rows"])], c["params"][10], c["params"][12], pre[list(c["rows"])])
    assert_reaches(tag, attn_run("f64", c)["out"], c["rows"])


@functools.lru_cache(maxsize=None)
def attn_dominant_case(shape):
    c = _attn(*shape, seed=30)
    cols = dominant_columns(c["F"])
    at = tuple(cols[i % len(cols)] for i in range(len(c["rows"])))
    _x_rows(c)[list(c["rows"]), list(at)] = BIG
    c.update(cols=at, groups=row_groups(c["P"], c["rows"], "dominant"))
    return c


def attn_dominant_conditions(c):
    tag = f"attn dominant F={c['F']} hid={c['hid']}"
    assert set(c["cols"]) == set(dominant_columns(c["F"]))
    assert_dominant(tag + " x", _x_rows(c)[list(c["rows"])].double(), c["cols"])
    assert_dominant(tag + " y", attn_y64(c)[list(c["rows"])], c["cols"])
    assert_reaches(tag, attn_run("f64", c)["out"], c["rows"])


ATTN_KINK_SEED = {(131, None, 4): 40, (37, 50, 1): 40}


@functools.lru_cache(maxsize=None)
def attn_kink_case(shape, cut=False):
    """ff.fc1's units 3 and hid - 1 (the last bit of the mask's last word) sit on the kink; cut: ff.fc2's columns for them are zero."""
    c = _attn(*shape, seed=ATTN_KINK_SEED[shape])
    m, s = LN_KINDS[1]
    _x_rows(c)[list(c["rows"])] = m + s * torch.randn(len(c["rows"]), c["F"], generator=_gen(6600 + c["F"]))
    u = (3, c["hid"] - 1)
    c["params"][12][list(u)] = 0.0
    c["params"][13][u[0]], c["params"][13][u[1]] = 0.0, -0.0
    if cut:
        c["params"][14][:, list(u)] = 0.0
    c["units"] = u
    return c


def attn_pre1(c):
    """(y, ff.fc1's pre-activation) in float64."""
    g2, b2, w1, c1 = (t.double() for t in c["params"][10:14])
    y = attn_y64(c)
    return y, F.linear(F.layer_norm(y, (y.shape[1],), g2, b2, 1e-6), w1, c1)


def attn_kink_conditions(c):
    tag = f"attn kink F={c['F']} hid={c['hid']}"
    y, pre = attn_pre1(c)
    mean_reach(tag + " LN2", y[list(c["rows"])], c["params"][10], c["params"][12], pre[list(c["rows"])])
    return kink_margin(tag, pre, c["units"])


@functools.lru_cache(maxsize=None)
def attn_nan_case(shape):
    """BS = 2, V = 80, 65 listed rows: the second tile of the 130 listed rows holds the last listed row of batch element 0 — the one
    that takes the NaN — and the first 63 of batch element 1."""
    a = ATTN_NAN
    c = _attn(*shape, seed=60, V=a["V"])
    c["idx"] = torch.sort(torch.randperm(a["V"], generator=_gen(6700))[:a["listed"]])[0].to(torch.int32)
    return c


def check_attn_containment(run, c, eq):
    """run(x) -> {out, grad_x} (BS V, F). A NaN in one listed row of batch element 0 leaves every row of batch element 1 and every
    unlisted row of batch element 0 unchanged, forward and backward, and reaches its own row."""
    a, V = ATTN_NAN, ATTN_NAN["V"]
    clean = run(c["x"])
    assert all(bool(torch.isfinite(clean[f]).all()) for f in ATTN_FIELDS)
    x = c["x"].clone()
    row = int(c["idx"][a["pos"]])
    x[a["b"], row, a["col"]] = NAN
    got = run(x)
    keep = torch.ones(ATTN_BS * V, dtype=torch.bool)
    keep[c["idx"].long()] = False                                # batch element 0's unlisted rows ...
    keep[V:] = True                                              # ... and all of batch element 1
    for f in ATTN_FIELDS:
        k = keep.to(got[f].device)
        assert eq(got[f][k], clean[f][k]), f
        assert not bool(torch.isfinite(got[f][row]).all()), f


# ---- the trunk and the head -------------------------------------------------------------------------------------------------------------
# P = 129: one full tile of 128 rows, four waves of 32, and a last row alone in its workgroup
TRUNK_P = 129
TRUNK_SILU = tuple((TRUNK_P, 131, 128, 128, w, "silu", w == 3, None, 7) for w in (3, 48))
TRUNK_RELU_SEED = {3: 1, 48: 0}
TRUNK_RELU = tuple((TRUNK_P, 3, 32, 32, w, "relu", w == 3, None, TRUNK_RELU_SEED[w]) for w in (3, 48))
TRUNK_HEAD_SEED = {"silu": 1, "relu": 3}
TRUNK_HEAD = ((TRUNK_P, 131, 128, 128, 3, "silu", True, None, TRUNK_HEAD_SEED["silu"]), (TRUNK_P, 3, 32, 32, 48, "relu", True, None, TRUNK_HEAD_SEED["relu"]))
TRUNK_UNITS = (1, 31)
TRUNK_LIVE_UNITS = (5, 20)
TRUNK_ZERO_ROWS = (31, 32, 128)                                         # a wave's last row, the next one's first, the tail's
TRUNK_NAN_ROWS = (31, 32)
LADDER_T = (0.25, 64.0)
QUAT_SCALES = (1e-6, 1e-3, 1.0, 1e2, 1e4)
HEAD_SD = 45.0                                                          # the deviation of a driven raw column over the P rows
HEAD_CENTRE = {0: 12.0, 1: -12.0, 2: 0.0, 10: 0.0, 11: -12.0, 12: 12.0, 13: 0.0}    # raw column: its centre


def trunk_to(c, device):
    mv = lambda t: t.to(device)
    return SimpleNamespace(x=mv(c.x), pts=mv(c.pts), trunk=[mv(t) for t in c.trunk], Wh=mv(c.Wh), bh=mv(c.bh), kw=c.kw,
                              cot={k: mv(v) for k, v in c.cot.items()})


def trunk_run(mode, c, device="cpu", x=None):
    d = trunk_to(c, device)
    return TC.run(d, mode, x=None if x is None else x.to(device))


@functools.lru_cache(maxsize=None)
def trunk_kink_case(case, cut=None):
    """Two kinds of unit of W1 on the kink. TRUNK_UNITS have a zero weight row and the biases +0.0 and -0.0: their v1 is 0 on every
    row, but whatever their gate lets through meets the zero row before it reaches grad_x, and the trunk has no parameter gradient.
    TRUNK_LIVE_UNITS keep their weight rows and have the biases +0.0 and -0.0, and the rows TRUNK_ZERO_ROWS of x are exactly zero: v1
    is 0 there on those rows alone, and a gate that opens at 0 adds d W1[u, :] to those rows of grad_x. cut="units": W2's columns
    for TRUNK_UNITS are zero (every row keeps its bits); cut="live": those for TRUNK_LIVE_UNITS too (the zero rows keep theirs)."""
    c = TC.make(case)
    u, live = TRUNK_UNITS, TRUNK_LIVE_UNITS
    c.trunk[0][list(u)] = 0.0
    c.trunk[1][u[0]], c.trunk[1][u[1]] = 0.0, -0.0
    c.trunk[1][live[0]], c.trunk[1][live[1]] = 0.0, -0.0
    c.x[list(TRUNK_ZERO_ROWS)] = 0.0
    if cut is not None:
        c.trunk[2][:, list(u if cut == "units" else u + live)] = 0.0
    c.units, c.live, c.zero_rows, c.groups = u, live, TRUNK_ZERO_ROWS, row_groups(case[0], TRUNK_ZERO_ROWS, "zero")
    return c


def trunk_kink_conditions(c, tag="trunk kink"):
    """v1 is exactly 0 at TRUNK_UNITS on every row and at TRUNK_LIVE_UNITS on the zero rows, where their weight rows are not zero;
    every other v1, and every v2, keeps the project's margin."""
    v1, v2, _ = TC.layers64(c)
    on = torch.zeros_like(v1, dtype=torch.bool)
    on[:, list(c.units)] = True
    for r in c.zero_rows:
        on[r, list(c.live)] = True
    assert bool((v1[on] == 0).all()) and float(c.trunk[0][list(c.live)].abs().min()) > 0 and float(c.x[list(c.zero_rows)].abs().max()) == 0
    assert bool(torch.equal(c.trunk[1][list(c.units + c.live)].signbit(), torch.tensor([False, True, False, True])))
    w = v1[~on]
    m, both = float(w.abs().min() / w.abs().max()), bool((w > 0).any() and (w < 0).any())
    print(f"{tag} v1: units {c.units} are exactly 0, units {c.live} on the rows {c.zero_rows}; the others' relu margin {m:.3e} "
          f"(guard {GUARD:.3e}), both sides: {both}")
    assert m > GUARD and both, (tag, m)
    return kink_margin(tag + " v2", v2, ())


@functools.lru_cache(maxsize=None)
def trunk_ladder_case(case):
    """Row i of x times t_i, the P values of t geometric from 0.25 to 64 in a seeded order. Groups: the rows by the band of their
    largest float64 |v1|."""
    c = TC.make(case)
    P = case[0]
    t = torch.logspace(math.log10(LADDER_T[0]), math.log10(LADDER_T[1]), P, dtype=F64)[torch.randperm(P, generator=_gen(6800))].float()
    c.x = c.x * t[:, None]
    top = TC.layers64(c)[0].abs().amax(1)
    c.groups = {"mid": top <= 4, "far": (top > 4) & (top <= 20), "deep": top > 20}
    return c


def trunk_ladder_conditions(c, tag="trunk silu ladder"):
    v1, v2, _ = TC.layers64(c)
    v = torch.cat([v1.reshape(-1), v2.reshape(-1)])
    print(f"{tag}: hidden pre-activations {float(v.min()):.4g} .. {float(v.max()):.4g}")
    assert float(v.min()) < -89 and float(v.max()) > 89          # expf(-v) overflows float32 past 88.7
    assert_bands(tag + " hidden", bands(v))
    n = {k: int(m.sum()) for k, m in c.groups.items()}
    print(f"{tag}: rows per band of their largest |v1|: {n}")
    assert all(k >= MIN_BAND for k in n.values()), n


def head_raw64(c):
    _, _, y = TC.layers64(c)
    return F.linear(y, c.Wh.double(), c.bh.double())


@functools.lru_cache(maxsize=None)
def trunk_head_case(case, qscale):
    """Wh's rows and bh for the restricted offset (0 .. 2), the opacity (10) and, with use_rgb, the colour (11 .. 13) are scaled and
    set so that each of those columns of the float64 raw values has the deviation HEAD_SD and the centre HEAD_CENTRE over the P rows:
    they pass +-20 and +-100. The rotation's rows and biases are multiplied by qscale, and the raw rotation with them, exactly. Element
    groups per field: the bands of its own raw value."""
    c = TC.make(case)
    cols = [o for o in HEAD_CENTRE if o <= 10 or c.kw["use_rgb"]]
    u = head_raw64(c)[:, cols]
    a = HEAD_SD / u.std(0)
    c.Wh[cols] *= a.float()[:, None]
    c.bh[cols] = (torch.tensor([HEAD_CENTRE[o] for o in cols], dtype=F64) + a * (c.bh[cols].double() - u.mean(0))).float()
    c.Wh[6:10] *= qscale
    c.bh[6:10] *= qscale
    raw = head_raw64(c)
    c.raw, c.qscale = raw, qscale
    c.bands = {"xyz": bands(raw[:, 0:3]), "opacity": bands(raw[:, 10:11])}
    if c.kw["use_rgb"]:
        c.bands["shs"] = bands(raw[:, 11:14].reshape(-1, 1, 3))
    return c


def trunk_head_conditions(c, tag="head tails"):
    raw, q = c.raw, c.qscale
    norm = raw[:, 6:10].norm(dim=1)
    print(f"{tag} qscale {q:g}: quaternion norms {float(norm.min()):.4g} .. {float(norm.max()):.4g}, largest raw scaling {float(raw[:, 3:6].max()):.4g}")
    assert q / 30 < float(norm.min()) and float(norm.max()) < 30 * q
    assert not bool(((norm > 1e-13) & (norm < 1e-11)).any()) and float(raw[:, 3:6].max()) < 15
    assert c.kw["restrict_offset"]
    for f, b in c.bands.items():
        # one opacity per row: its three bands as two groups per sign would ask 40 of 129 rows of each; both signs of "far" and "deep" are
        # asked of the three-column fields, and of the opacity the bands whole
        if f == "opacity":
            whole = {"mid": b["mid"], "far": b["far+"] | b["far-"], "deep": b["deep+"] | b["deep-"]}
            assert_bands(f"{tag} {f}", whole, tuple(whole))
            assert all(int(b[k].sum()) >= 1 for k in BANDS)
        else:
            assert_bands(f"{tag} {f}", b)
        v = {"xyz": raw[:, 0:3], "opacity": raw[:, 10:11], "shs": raw[:, 11:14]}[f]
        assert float(v.min()) < -89 and float(v.max()) > 89, f       # expf overflows float32 past 88.7


def check_trunk_containment(run, c, eq):
    """run(x) -> TC.OUT's fields. A NaN in row 31, and in row 32, of x: every other row of every output and of grad_x is unchanged."""
    clean = run(c.x)
    assert all(bool(torch.isfinite(clean[f]).all()) for f in TC.OUT)
    for r in TRUNK_NAN_ROWS:
        x = c.x.clone()
        x[r, 1] = NAN
        got = run(x)
        keep = torch.arange(c.x.shape[0]) != r
        for f in TC.FIELDS + ("grad_x",):
            k = keep.to(got[f].device)
            assert eq(got[f][k], clean[f][k]), (r, f)
        assert not bool(torch.isfinite(got["grad_x"][r]).all()) and not bool(torch.isfinite(got["rotation"][r]).all()), r


def zero_cotangents(c):
    """The trunk case c with every cotangent zero."""
    d = trunk_to(c, "cpu")
    d.cot = {k: torch.zeros_like(v) for k, v in c.cot.items()}
    return d


def is_plus_zero(t):
    """Every element is +0.0, bit for bit."""
    from tests.fit_cases import bits
    return bool((bits(t.float()) == 0).all())


if __name__ == "__main__":                                   # every condition, printed: how the seeds were chosen
    for s in VERT_SHAPES:
        for k in range(len(LN_KINDS)):
            vert_ln_conditions(vert_ln_case(*s, k))
        vert_dominant_conditions(vert_dominant_case(*s))
        vert_kink_conditions(vert_kink_case(*s))
    for s in VERT_TAIL_SHAPES:
        vert_tails_conditions(vert_tails_case(*s))
    for layout, k in COND_LN:
        cond_ln_conditions(cond_ln_case(layout, k))
    for k in COND_COMBOS:
        cond_combo_conditions(cond_combo_case(k))
    cond_kink_conditions(cond_kink_case())
    for s in ATTN_SHAPES:
        for k in range(len(LN_KINDS)):
            attn_ln_conditions(attn_ln_case(s, k))
        attn_dominant_conditions(attn_dominant_case(s))
        attn_kink_conditions(attn_kink_case(s))
    for case in TRUNK_RELU:
        trunk_kink_conditions(trunk_kink_case(case), TC.case_id(case))
    for case in TRUNK_SILU:
        trunk_ladder_conditions(trunk_ladder_case(case), TC.case_id(case))
    for case in TRUNK_HEAD:
        for q in QUAT_SCALES:
            trunk_head_conditions(trunk_head_case(case, q), TC.case_id(case))
