"""Shared by tests/test_pool_cpu.py, tests/test_gpu_pool.py and tests/test_gpu_pool_edges.py: the fixture, the rounding bound of a
float32 sum, a per-cell loop in float64 that shares no code with guassianhand_amd.pool (`loop_pool`), and the generator of the
edge cases both the CPU and the GPU tests draw (`SWEEP`, `make_case`).

The bound. A float32 sum of n terms, added in any order, lies within gamma_(n-1) * sum|terms| of the exact sum, and
gamma_(n-1) = (n-1) u / (1 - (n-1) u) <= n u for n <= 4096 with u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2). Dividing by the count scales that error and adds one rounding of the quotient, u * |result|. So an
element computed as (sum of n terms) / count is within

    n * u * sum|terms| / count + u * |result|

of the exact value (count = 1 where nothing is divided). `sum|terms| / count` is the same reduction applied to |terms|, so the
tests get it from the float64 restatement run on the absolute values."""
import os

import numpy as np
import torch

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_fixture.npz")


def load_fixture():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def fixture_weights(fx):
    return {k[2:]: v for k, v in fx.items() if k.startswith("w.")}


def fixture_cfg(fx, kind):
    T, D, hid, cdim, plane, blocks = (int(v) for v in fx["dims"])
    return dict(input_channels=D, c_dim=cdim, hidden_dim=hid, scatter_type=kind, plane_size=plane, n_blocks=blocks,
                radius=float(fx["radius"]))


def assert_within(got, exact, bound, what, slack=1.0):
    """|got - exact| <= slack * bound elementwise (exact, bound: float64). Prints the worst ratio before asserting."""
    got, exact, bound = got.detach().double().cpu(), exact.detach().double().cpu(), bound.detach().double().cpu()
    err = (got - exact).abs()
    ratio = (err / (slack * bound).clamp(min=1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max |err| {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    bad = err > slack * bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, worst err / bound {ratio:.3f}"


def mean_pool_bound(absx_pooled64, result64, counts_per_point):
    """pool 'mean' forward / backward: n = the cell's population, terms = the cell's rows."""
    return counts_per_point.double().unsqueeze(1) * U * absx_pooled64 + U * result64.abs()


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()


# ---- the independent yardstick: a per-cell loop in float64 ---------------------------------------------------------------------------
# Shares no code with guassianhand_amd.pool. The rules are those of include/gh_pool.h: ties of a maximum go to the lowest point
# index; a NaN never wins, and a cell of NaNs alone is empty for that channel (value 0, argmax T, no gradient); -inf is an ordinary
# value; means propagate NaN and infinities; a point whose index is outside [0, n_cells) contributes nothing and receives zeros.
def loop_pool(x, index, n_cells, reduce="max", cot=None, plane_cot=None):
    """x (T,C), index (T,), on the CPU -> a namespace of float64 / int64 tensors:
         pooled (T,C)          every point's row is its cell's max / mean         abs_pooled (T,C)   the same mean over |x| (mean only)
         plane (C,n_cells)     the mean per cell, 0 for empty cells               abs_plane (C,n_cells)
         argmax (n_cells,C)    lowest point index attaining the maximum, T for an empty cell (max only)
         lands (T,C) bool      where a max gradient lands (max only)
         grad (T,C)            exact gradient of sum(pooled * cot)                abs_grad (T,C)     sum|cot| (/ count) where it lands
         plane_grad (T,C)      exact gradient of sum(plane * plane_cot)
         counts (n_cells,), count_pt (T,): a point's cell population, 0 without a cell
         cell_start (n_cells+1,), order (T,): the plan, int32"""
    from types import SimpleNamespace
    assert reduce in ("max", "mean")
    T, C = x.shape
    x64, idx = x.detach().double().cpu(), index.detach().cpu().long().reshape(-1)
    has = (idx >= 0) & (idx < n_cells)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    r = SimpleNamespace(pooled=z(T, C), abs_pooled=z(T, C), plane=z(C, n_cells), abs_plane=z(C, n_cells),
                        argmax=torch.full((n_cells, C), T, dtype=torch.int64), lands=torch.zeros(T, C, dtype=torch.bool),
                        grad=None, abs_grad=None, plane_grad=None, counts=torch.zeros(n_cells, dtype=torch.int64),
                        count_pt=torch.zeros(T, dtype=torch.int64))
    if cot is not None:
        cot = cot.detach().double().cpu()
        r.grad, r.abs_grad = z(T, C), z(T, C)
    if plane_cot is not None:
        plane_cot = plane_cot.detach().double().cpu()
        r.plane_grad = z(T, C)
    chans = torch.arange(C)
    lists = []
    for c in torch.unique(idx[has]).tolist():
        pts = torch.nonzero(idx == c).flatten()                             # ascending point index
        lists.append(pts)
        rows, k = x64[pts], pts.numel()
        r.counts[c], r.count_pt[pts] = k, k
        r.plane[:, c], r.abs_plane[:, c] = rows.sum(0) / k, rows.abs().sum(0) / k
        if plane_cot is not None:
            r.plane_grad[pts] = (plane_cot[:, c] / k).expand(k, C)
        if reduce == "mean":
            r.pooled[pts], r.abs_pooled[pts] = (rows.sum(0) / k).expand(k, C), (rows.abs().sum(0) / k).expand(k, C)
            if cot is not None:
                r.grad[pts], r.abs_grad[pts] = (cot[pts].sum(0) / k).expand(k, C), (cot[pts].abs().sum(0) / k).expand(k, C)
            continue
        nan = torch.isnan(rows)
        seen = torch.where(nan, torch.full_like(rows, float("-inf")), rows)
        top = torch.max(seen, dim=0).values
        hit = (seen == top) & ~nan
        first = torch.where(hit, torch.arange(k).unsqueeze(1).expand(k, C), torch.full((k, C), k)).min(dim=0).values
        live = first < k                                                    # channels in which the cell holds something but NaN
        arg = pts[first.clamp(max=k - 1)]
        r.argmax[c] = torch.where(live, arg, torch.full_like(arg, T))
        r.pooled[pts] = torch.where(live, top, torch.zeros_like(top)).expand(k, C)
        r.lands[arg[live], chans[live]] = True
        if cot is not None:
            r.grad[arg[live], chans[live]] = cot[pts].sum(0)[live]
            r.abs_grad[arg[live], chans[live]] = cot[pts].abs().sum(0)[live]
    out_of_range = torch.nonzero(~has).flatten()
    r.order = torch.cat(lists + [out_of_range]).to(torch.int32)
    r.cell_start = torch.cat([torch.zeros(1, dtype=torch.int64), r.counts.cumsum(0)]).to(torch.int32)
    return r


def assert_within_or_same_nonfinite(got, exact, bound, what, slack=1.0):
    """assert_within where the exact value is finite; where it is NaN or +-inf (a cell that holds one) `got` must be the same
    NaN / the same infinity. `err > bound` is false for a NaN, so assert_within alone would let those elements through."""
    got, exact, bound = got.detach().double().cpu(), exact.detach().double().cpu(), bound.detach().double().cpu()
    fin = torch.isfinite(exact)
    assert torch.equal(torch.isnan(got), torch.isnan(exact)), f"{what}: NaNs in other places than the float64 loop's"
    inf = torch.isinf(exact)
    assert torch.equal(got[inf], exact[inf]), f"{what}: infinities differ from the float64 loop's"
    zero = torch.zeros((), dtype=torch.float64)
    assert_within(torch.where(fin, got, zero), torch.where(fin, exact, zero), torch.where(fin, bound, zero), what, slack)


# ---- the case generator ----------------------------------------------------------------------------------------------------------------
LADDER = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300)      # cell c of the "ladder" population holds exactly LADDER[c] points
INT32_MIN = -(1 << 31)
BLOCK = 256                                                      # the plan's points per workgroup


def _bad_positions(T):
    """Either side of the plan's block boundaries, and both ends."""
    at = {0, T - 1}
    for b in range(BLOCK, T, BLOCK):
        at |= {b - 1, b, b + 1}
    return sorted(p for p in at if 0 <= p < T)


def make_index(pop, T, n_cells, dtype=torch.int64, bad=False, seed=0):
    """index (T,) of `dtype` for a named population pattern:
         random        uniform over the cells                       own_cell     every point its own cell, shuffled (n_cells >= T)
         all_in_first  every point in cell 0                        all_in_last  every point in cell n_cells - 1
         ladder        cells 0..12 hold exactly LADDER[c] points, shuffled so that a cell's points are spread over the 256-point
                       blocks; the rest go to the cells from 13 on at random (n_cells >= 14 when there is a rest)
         all_bad       every index out of range
       bad=True replaces the index around every block boundary and at both ends by out-of-range values (-1, n_cells, and 1 << 40
       for int64 / INT32_MIN for int32); the population pattern is laid over the remaining points."""
    g = torch.Generator().manual_seed(1000 + seed)
    outside = [-1, n_cells, (1 << 40) if dtype == torch.int64 else INT32_MIN]
    if pop == "all_bad":
        return torch.tensor([outside[i % 3] for i in range(T)], dtype=dtype)
    bad_at = _bad_positions(T) if bad else []
    assert len(bad_at) < T
    good = torch.ones(T, dtype=torch.bool)
    good[bad_at] = False
    Tg = int(good.sum())
    if pop == "random":
        cells = torch.randint(0, n_cells, (Tg,), generator=g)
    elif pop == "own_cell":
        assert n_cells >= Tg
        cells = torch.randperm(n_cells, generator=g)[:Tg]
    elif pop == "all_in_first":
        cells = torch.zeros(Tg, dtype=torch.int64)
    elif pop == "all_in_last":
        cells = torch.full((Tg,), n_cells - 1, dtype=torch.int64)
    elif pop == "ladder":
        rest = Tg - sum(LADDER)
        assert rest >= 0 and n_cells >= len(LADDER) + (rest > 0), (Tg, n_cells)
        cells = torch.cat([torch.full((k,), c, dtype=torch.int64) for c, k in enumerate(LADDER)] +
                          [torch.randint(len(LADDER), max(n_cells, len(LADDER) + 1), (rest,), generator=g)])
        cells = cells[torch.randperm(Tg, generator=g)]
    else:
        raise ValueError(pop)
    index = torch.empty(T, dtype=torch.int64)
    index[good] = cells
    index[bad_at] = torch.tensor([outside[i % 3] for i in range(len(bad_at))], dtype=torch.int64)
    return index.to(dtype)


def _cell_lists(index, n_cells):
    idx = index.long()
    return [torch.nonzero(idx == c).flatten() for c in torch.unique(idx[(idx >= 0) & (idx < n_cells)]).tolist()]


def _quarter(k, w):
    """[lo, hi) of quarter w of a list of k entries: the kernels' cut."""
    return k * w // 4, k * (w + 1) // 4


def make_values(values, index, n_cells, C, seed=0):
    """x (T,C) float32 for a named value pattern over the cells of `index`:
         normal      random normal                              grid        randint(-3, 4) / 4: ties in nearly every cell and channel
         const_col   normal, first and last column constant     dup_rows    two identical rows hold every channel's maximum of a cell,
         inf         column 0: -inf throughout the even cells,              either side of a quarter cut or (cells over 256 points) of a
                     sprinkled elsewhere; last column: +inf                 64-entry chunk inside a quarter, cell by cell in turn
                     sprinkled (a cell with both means NaN)
         nan_first / nan_middle / nan_last   a NaN at that place of every cell's list, in the even channels
         nan_q0 .. nan_q3   a NaN at the first entry of that quarter of every cell's list in the even channels, and at the middle
                     entry of the quarter in the channels 1, 5, 9, ...
         nan_all     the even channels of every third cell are NaN in all its rows
         nan_bad     normal, every point without a cell is NaN (and +inf in the last column)
       The odd channels (3, 7, ... for nan_q*) stay free of NaN as the control."""
    g = torch.Generator().manual_seed(2000 + seed)
    T = index.numel()
    x = torch.randn(T, C, generator=g)
    even = torch.arange(0, C, 2)
    if values == "normal":
        return x
    if values == "grid":
        return torch.randint(-3, 4, (T, C), generator=g).float() / 4
    if values == "const_col":
        x[:, 0], x[:, C - 1] = 1.5, -0.25
        return x
    if values == "nan_bad":
        idx = index.long()
        out = (idx < 0) | (idx >= n_cells)
        assert out.any()
        x[out] = float("nan")
        x[out, C - 1] = float("inf")
        return x
    for i, pts in enumerate(_cell_lists(index, n_cells)):
        k = pts.numel()
        if values == "dup_rows":
            if k < 2:
                continue
            pairs = [(_quarter(k, w)[0] - 1, _quarter(k, w)[0]) for w in (1, 2, 3) if 0 < _quarter(k, w)[0] < k]
            pairs += [(_quarter(k, w)[0] + 63, _quarter(k, w)[0] + 64) for w in range(4) if _quarter(k, w)[1] - _quarter(k, w)[0] > 64]
            a, b = pairs[i % len(pairs)]
            x[pts[a]] = x[pts[b]] = x[pts].max(dim=0).values + 1.0
        elif values == "inf":
            x[pts[torch.rand(k, generator=g) < 0.2], 0] = float("-inf")
            if i % 2 == 0:
                x[pts, 0] = float("-inf")
            x[pts[torch.rand(k, generator=g) < 0.1], C - 1] = float("inf")
        elif values in ("nan_first", "nan_middle", "nan_last"):
            x[pts[{"nan_first": 0, "nan_middle": k // 2, "nan_last": k - 1}[values]], even] = float("nan")
        elif values in ("nan_q0", "nan_q1", "nan_q2", "nan_q3"):
            lo, hi = _quarter(k, int(values[-1]))
            if hi > lo:
                x[pts[lo], even] = float("nan")
                x[pts[(lo + hi) // 2], torch.arange(1, C, 4)] = float("nan")
        elif values == "nan_all":
            if i % 3 == 0:
                x[pts.unsqueeze(1), even.unsqueeze(0)] = float("nan")
        else:
            raise ValueError(values)
    return x


NAN_VALUES = ("nan_first", "nan_middle", "nan_last", "nan_q0", "nan_q1", "nan_q2", "nan_q3", "nan_all", "nan_bad")
TIE_VALUES = ("grid", "dup_rows", "const_col")

# (T, C, n_cells, population, values, index dtype, out-of-range points mixed in). Not the product of the axes: every T of
# 1, 3, 255, 256, 257, 700, 3000, every C of 1, 16, 63, 64, 65, 100, 130, every n_cells of 1, 7, 8, 9, 1023, 1024, 1025, 2500, 8192,
# every population, both index types and every value pattern appear at least once, and every case runs every kernel.
I32, I64 = torch.int32, torch.int64
SWEEP = (
    (1, 1, 1, "all_in_first", "normal", I64, False),
    (1, 65, 9, "all_in_last", "normal", I32, False),
    (3, 16, 7, "random", "grid", I32, False),
    (255, 63, 8, "random", "grid", I64, True),
    (256, 64, 9, "random", "normal", I32, True),
    (257, 65, 1023, "random", "const_col", I64, True),
    (700, 100, 1024, "own_cell", "normal", I32, False),
    (700, 130, 7, "random", "dup_rows", I64, True),
    (3000, 130, 1025, "ladder", "dup_rows", I64, True),
    (3000, 16, 2500, "ladder", "grid", I32, True),
    (3000, 65, 8192, "own_cell", "normal", I64, False),
    (3000, 16, 8192, "all_in_last", "grid", I32, True),
    (3000, 64, 1, "all_in_first", "normal", I64, False),
    (3000, 1, 2500, "all_in_first", "grid", I32, False),
    (3000, 100, 8, "all_in_last", "dup_rows", I64, True),
    (700, 16, 9, "all_bad", "normal", I64, False),
    (257, 65, 1025, "all_bad", "normal", I32, False),
    (1000, 65, 16, "ladder", "inf", I64, True),
    (1000, 1, 14, "ladder", "inf", I32, False),
) + tuple((1000, 16 if i % 2 else 65, 20, "ladder", v, I32 if i % 2 else I64, True) for i, v in enumerate(NAN_VALUES))


def case_id(case):
    T, C, n, pop, values, dtype, bad = case
    return f"T{T}-C{C}-n{n}-{pop}-{values}-{'i64' if dtype == torch.int64 else 'i32'}{'-bad' if bad else ''}"


def make_case(case, seed=0):
    """(index, x) of one SWEEP entry, on the CPU."""
    T, C, n, pop, values, dtype, bad = case
    index = make_index(pop, T, n, dtype, bad, seed)
    return index, make_values(values, index, n, C, seed)


def permute_within_cells(index, x, n_cells, seed=0):
    """The same cloud with the rows of every cell shuffled among that cell's points: index is unchanged."""
    g = torch.Generator().manual_seed(3000 + seed)
    y = x.clone()
    for pts in _cell_lists(index, n_cells):
        y[pts] = x[pts[torch.randperm(pts.numel(), generator=g)]]
    return y


_SWEEP_CACHE = {}


def sweep_case(case):
    """One SWEEP entry with everything the CPU and the GPU tests compare against, computed once and shared (treat as read-only):
    index, x, cot (T,C), left (T,C: the cat buffer's left-half cotangent), plane_cot (C,n_cells), and loop_pool's results for
    both reductions under .max and .mean."""
    from types import SimpleNamespace
    if case not in _SWEEP_CACHE:
        T, C, n = case[:3]
        index, x = make_case(case)
        g = torch.Generator().manual_seed(4000 + T + C + n)
        cot, left, plane_cot = torch.randn(T, C, generator=g), torch.randn(T, C, generator=g), torch.randn(C, n, generator=g)
        _SWEEP_CACHE[case] = SimpleNamespace(T=T, C=C, n=n, index=index, x=x, cot=cot, left=left, plane_cot=plane_cot,
                                             max=loop_pool(x, index, n, "max", cot, plane_cot),
                                             mean=loop_pool(x, index, n, "mean", cot, plane_cot))
    return _SWEEP_CACHE[case]


def pool_bounds(loop, kind, left=None):
    """The derived bounds of one reduction from loop_pool's quantities: (forward, backward, cat backward) — forward None for the
    maximum, which is exact."""
    cnt = loop.count_pt.double().unsqueeze(1)
    if kind == "mean":
        fwd = cnt * U * loop.abs_pooled + U * loop.pooled.abs()
        bwd = cnt * U * loop.abs_grad + U * loop.grad.abs()
    else:
        fwd, bwd = None, cnt * U * loop.abs_grad
    cat = None if left is None else (cnt + 1) * U * (left.double().abs() + loop.abs_grad)
    return fwd, bwd, cat


def plane_bounds(loop):
    return loop.counts.double() * U * loop.abs_plane + U * loop.plane.abs(), 2 * U * loop.plane_grad.abs()
