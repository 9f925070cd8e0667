"""gh_knn_indices / gh_knn_mismatch_mask at the shapes tests/test_gpu_knn.py leaves out (tests/knn_cases.py), against the brute-force
oracle (oracle/gh_oracle.c:gho_knn, itself pinned at the same shapes by tests/test_knn_oracle.py). Every comparison is torch.equal on
index lists and squared distances: K around the two 64-entry halves of the candidate list, N from one point up, around a wave and around
the four queries of a workgroup, K = N, signed / dyadic / far-from-origin / degenerate clouds, exact power-of-two scalings, B > 1, other
input forms, non-finite points (containment), the 128-cells-per-axis clamp at 1.25 M points, the mask kernel on hand-built lists and
the argument checks of both entry points.

The exactness contract ends where squared distances between distinct points stop being normal float32 numbers (guassianhand_amd/knn.py);
test_below_the_domain asserts only what holds there and prints how far the lists are from the brute-force ones."""
import time

import pytest
import torch

from oracle import oracle_c
from tests.knn_cases import CLOUDS, PAIRS, case_cloud, cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def device_knn(points, K, dev):
    """(idx (N, K) int32, squared distances (N, K)) of one (N, 3) cloud, on the host."""
    from guassianhand_amd import knn
    idx, d = knn.knn_indices(points[None].to(dev), K, return_dists=True)
    return idx[0].cpu(), d[0].cpu()


def same_bits(a, b):
    """torch.equal on the bit patterns of two float32 tensors (tells -0.0 from +0.0, and equal NaNs are equal)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rows_in_range_and_unique(idx, N):
    srt = idx.sort(dim=1).values
    return bool((idx >= 0).all()) and bool((idx < N).all()) and bool((srt[:, 1:] != srt[:, :-1]).all())


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CLOUDS)
def test_sweep_equals_oracle(dev, name):
    bad = []
    for N, K in PAIRS:
        p = case_cloud(name, N)
        idx, d = device_knn(p, K, dev)
        want_idx, want_d = oracle_c.knn(p, K)
        if not (torch.equal(idx, want_idx) and same_bits(d, want_d)):
            rows = int(((idx != want_idx).any(1) | (d.view(torch.int32) != want_d.view(torch.int32)).any(1)).sum())
            bad.append((N, K, rows))
    assert not bad, f"{name}: (N, K, rows that differ from the oracle) = {bad}"


# ---- power-of-two scaling ------------------------------------------------------------------------------------------------------------

SCALED = ("uniform", "signed", "dyadic")


@pytest.mark.parametrize("K", [65, 100])
@pytest.mark.parametrize("name", SCALED)
def test_power_of_two_scaling_is_exact(dev, name, K):
    """Inside the normal range a scaling by 2^k changes no rounding: same lists, distances times 4^k, both equal to the oracle's."""
    p = cloud(name, 300, 7)
    idx, d = device_knn(p, K, dev)
    want_idx, want_d = oracle_c.knn(p, K)
    assert torch.equal(idx, want_idx) and same_bits(d, want_d)
    for k in (-40, 40):
        q = p * 2.0 ** k
        idx_k, d_k = device_knn(q, K, dev)
        assert torch.equal(idx_k, idx), k
        assert same_bits(d_k, d * 4.0 ** k), k
        o_idx, o_d = oracle_c.knn(q, K)
        assert torch.equal(idx_k, o_idx) and same_bits(d_k, o_d), k


@pytest.mark.parametrize("name", SCALED)
def test_below_the_domain(dev, name):
    """At 2^-100 every squared distance underflows to 0 and the stop rule ends the walk as soon as K candidates exist (0 <= 0), before the
    lowest indices are seen: outside the stated domain. Guaranteed there: the call returns, rows are in range and unique, distances are 0.
    The number of rows that still equal the brute-force list arange(K) is printed, not asserted."""
    p = cloud(name, 300, 7) * 2.0 ** -100
    for K in (65, 100):
        idx, d = device_knn(p, K, dev)
        assert rows_in_range_and_unique(idx, 300)
        assert bool((d == 0).all())
        rows = int((idx == torch.arange(K, dtype=torch.int32)).all(1).sum())
        print(f"below the domain: {name} x 2^-100, K = {K}: {rows} of 300 rows equal arange(K)")


# ---- batch ---------------------------------------------------------------------------------------------------------------------------

def test_batch_elements_equal_solo_calls_and_oracle(dev):
    from guassianhand_amd import knn
    clouds = [cloud(n, 300, 21) for n in ("uniform", "offset", "two_clusters")]
    batch = torch.stack(clouds).to(dev)
    idx, d = knn.knn_indices(batch, 65, return_dists=True)
    idx2, d2 = knn.knn_indices(batch, 65, return_dists=True)
    assert idx.shape == (3, 300, 65) and d.shape == (3, 300, 65)
    assert torch.equal(idx, idx2) and same_bits(d, d2)
    for b, p in enumerate(clouds):
        solo_idx, solo_d = device_knn(p, 65, dev)
        want_idx, want_d = oracle_c.knn(p, 65)
        assert torch.equal(idx[b].cpu(), solo_idx) and same_bits(d[b].cpu(), solo_d), b
        assert torch.equal(solo_idx, want_idx) and same_bits(solo_d, want_d), b


def test_interaction_mask_batch_of_two(dev):
    from guassianhand_amd import knn
    posed = [cloud("uniform", 300, 21), cloud("two_clusters", 300, 21)]
    noise = cloud("signed", 300, 22) * 0.025
    t_pose = [posed[0] + noise, posed[1] + noise * 0.01]                 # moved by a fraction of the point spacing: some lists survive
    got = knn.interaction_mask(torch.stack(posed).to(dev), torch.stack(t_pose).to(dev), K=65, min_same=10)
    assert got.shape == (2, 300, 1) and got.dtype == torch.bool
    for b in range(2):
        want = oracle_c.interaction_mask(posed[b], t_pose[b], K=65, min_same=10)
        assert 0.05 < float(want.float().mean()) < 0.95                  # the case is not trivial
        assert torch.equal(got[b, :, 0].cpu(), want), b


# ---- input forms ---------------------------------------------------------------------------------------------------------------------

def both(points, K=65):
    from guassianhand_amd import knn
    return knn.knn_indices(points, K, return_dists=True)


def test_input_forms_equal_the_float32_contiguous_form(dev):
    g = torch.Generator().manual_seed(31)
    forms = {
        "float64": torch.rand(2, 300, 3, generator=g, dtype=torch.float64).to(dev),
        "float16": torch.rand(2, 300, 3, generator=g).half().to(dev),                    # 11 bits per coordinate: ties
        "window": torch.rand(2, 300, 5, generator=g).to(dev)[:, :, 1:4],
        "requires_grad": torch.rand(2, 300, 3, generator=g).to(dev).requires_grad_(True),
    }
    assert not forms["window"].is_contiguous()
    for name, x in forms.items():
        plain = x.detach().float().contiguous()
        idx, d = both(x)
        want_idx, want_d = both(plain)
        assert torch.equal(idx, want_idx) and same_bits(d, want_d), name
        assert not idx.requires_grad and not d.requires_grad, name
        o_idx, o_d = oracle_c.knn(plain[1].cpu(), 65)
        assert torch.equal(idx[1].cpu(), o_idx) and same_bits(d[1].cpu(), o_d), name


def test_knn_points_refuses_a_second_point_set(dev):
    from guassianhand_amd import knn
    g = torch.Generator().manual_seed(32)
    p = torch.rand(1, 100, 3, generator=g).to(dev)
    with pytest.raises(NotImplementedError):
        knn.knn_points(p, torch.rand(1, 100, 3, generator=g).to(dev), K=4)
    with pytest.raises(NotImplementedError):
        knn.knn_points(p, p.clone(), K=4)
    d, idx, none = knn.knn_points(p, p, K=4)                                             # the form that is provided
    assert none is None and idx.dtype == torch.int64 and idx.shape == (1, 100, 4) and d.shape == (1, 100, 4)


# ---- non-finite points: containment --------------------------------------------------------------------------------------------------

BAD_ROWS = (3, 77, 400)


@pytest.fixture(scope="module")
def finite_subset():
    """The 500-point cloud, the indices of the 497 rows that stay finite, and the oracle's lists on those rows alone (indices mapped
    back): K = 100 <= 497 finite points and a non-finite key exceeds every finite one, so no non-finite point enters a finite row's list."""
    p = cloud("signed", 500, 41)
    keep = torch.tensor([i for i in range(500) if i not in BAD_ROWS])
    sub_idx, sub_d = oracle_c.knn(p[keep], 100)
    return p, keep, keep[sub_idx.long()].to(torch.int32), sub_d


@pytest.mark.parametrize("coords", ["all", "one"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_points_are_contained(dev, finite_subset, value, coords):
    """The walk is bounded by the grid (r <= G), so a NaN or infinite point cannot spin it; finite rows must not notice such points."""
    p, keep, want_idx, want_d = finite_subset
    q = p.clone()
    if coords == "all":
        q[list(BAD_ROWS)] = value
    else:
        q[list(BAD_ROWS), 1] = value
    idx, d = device_knn(q, 100, dev)
    assert bool((idx >= 0).all()) and bool((idx < 500).all())            # every row, the non-finite ones included
    assert torch.equal(idx[keep], want_idx)
    assert same_bits(d[keep], want_d)


# ---- the grid clamp ------------------------------------------------------------------------------------------------------------------

def test_grid_clamp_at_1_25_million_points(dev):
    """int(cbrt(1,250,000) * 1.2) = 129 cells per axis, clamped to 128: 21 key bits (three radix passes with the scan kernel) and
    2,097,153 cell starts. 512 random queries against the oracle and the whole-result properties; the device time is printed."""
    from guassianhand_amd import knn
    N, K = 1_250_000, 8
    g = torch.Generator().manual_seed(51)
    p = torch.rand(N, 3, generator=g)
    qs = torch.randperm(N, generator=g)[:512].to(torch.int32)
    pd = p[None].to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, d = knn.knn_indices(pd, K, return_dists=True)
    torch.cuda.synchronize()
    print(f"knn_indices N = {N}, K = {K}: {time.perf_counter() - t0:.3f} s on the device (allocation included)")
    idx, d = idx[0], d[0]
    want_idx, want_d = oracle_c.knn(p, K, queries=qs)
    assert torch.equal(idx[qs.long().to(dev)].cpu(), want_idx)
    assert same_bits(d[qs.long().to(dev)].cpu(), want_d)
    assert bool((d[:, 1:] >= d[:, :-1]).all())
    assert bool((d[:, 0] == 0).all())
    assert torch.equal(idx[:, 0], torch.arange(N, dtype=torch.int32, device=dev))        # distinct points: each is its own nearest
    assert rows_in_range_and_unique(idx, N)


# ---- the mask kernel alone -----------------------------------------------------------------------------------------------------------

def rank_orders(K):
    """Two orders of the ranks [0, K) from which a row takes its agreeing ranks as a prefix: the ends first (rank 0, rank K - 1), then the
    ranks on both sides of every multiple of 64, then the rest; and the same from its other end, so that a small count lands in the middle
    of a lane stride."""
    first = [0, K - 1] + [r for m in range(64, K + 1, 64) for r in (m - 1, m, m - 2, m + 1)]
    order = []
    for r in first + list(range(K)):
        if 0 <= r < K and r not in order:
            order.append(r)
    return order, order[::-1]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 100, 128, 200])
def test_mismatch_mask_on_hand_built_lists(dev, K):
    from guassianhand_amd._call import launch, ptr
    g = torch.Generator().manual_seed(60 + K)
    orders = rank_orders(K)
    for N in (1, 3, 4, 5, 257):
        for min_same in (0, 1, 10, K, K + 1):
            counts = [min(max(c, 0), K) for c in (0, min_same - 1, min_same, K)]
            a = torch.randint(0, 1000, (N, K), generator=g, dtype=torch.int32)
            b = a + 1                                                                    # no rank agrees ...
            chosen = torch.empty(N, dtype=torch.int64)
            for i in range(N):
                chosen[i] = counts[(i + N + min_same) % 4]
                ranks = orders[(i // 4) % 2][:int(chosen[i])]
                b[i, ranks] = a[i, ranks]                                                # ... but these
            assert torch.equal((a == b).sum(-1), chosen)
            want = (a == b).sum(-1) < min_same
            mask = torch.full((N,), 7, dtype=torch.uint8, device=dev)
            ad, bd = a.to(dev), b.to(dev)
            launch("gh_knn_mismatch_mask", dev, ptr(ad), ptr(bd), N, K, min_same, ptr(mask))
            assert torch.equal(mask.cpu(), want.to(torch.uint8)), (N, K, min_same)


def test_mismatch_mask_argument_checks(dev):
    from guassianhand_amd import _abi, _lib
    from guassianhand_amd._call import ptr, stream
    L = _lib.lib()
    a = torch.zeros(4, 8, dtype=torch.int32, device=dev)
    mask = torch.full((4,), 7, dtype=torch.uint8, device=dev)
    assert L.gh_knn_mismatch_mask(ptr(a), ptr(a), 0, 8, 1, ptr(mask), stream(dev)) == _abi.GH_OK            # N = 0: nothing is written
    assert L.gh_knn_mismatch_mask(None, None, 0, 8, 1, None, stream(dev)) == _abi.GH_OK
    torch.cuda.synchronize()
    assert mask.tolist() == [7, 7, 7, 7]
    assert L.gh_knn_mismatch_mask(ptr(a), ptr(a), 4, 0, 1, ptr(mask), stream(dev)) == _abi.GH_ERR_INVALID_ARG
    assert L.gh_knn_mismatch_mask(ptr(a), ptr(a), -1, 8, 1, ptr(mask), stream(dev)) == _abi.GH_ERR_INVALID_ARG
    assert L.gh_knn_mismatch_mask(ptr(a), None, 4, 8, 1, ptr(mask), stream(dev)) == _abi.GH_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert mask.tolist() == [7, 7, 7, 7]


# ---- C-ABI checks of gh_knn_indices --------------------------------------------------------------------------------------------------

def test_knn_indices_argument_checks(dev):
    from guassianhand_amd import _abi, _lib
    from guassianhand_amd._call import ptr, stream
    L = _lib.lib()
    N, K = 200, 65
    p = cloud("uniform", N, 61)
    pd = p.to(dev)
    nbytes = int(L.gh_knn_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idx = torch.full((N, K), -7, dtype=torch.int32, device=dev)
    d = torch.full((N, K), -7.0, device=dev)
    s = stream(dev)
    assert L.gh_knn_indices(None, 0, K, None, None, None, 0, s) == _abi.GH_OK                                 # N = 0
    assert L.gh_knn_indices(ptr(pd), N, K, ptr(idx), ptr(d), ptr(ws), nbytes - 1, s) == _abi.GH_ERR_WORKSPACE_SMALL
    assert L.gh_knn_indices(ptr(pd), N, K, None, ptr(d), ptr(ws), nbytes, s) == _abi.GH_ERR_INVALID_ARG       # null idx_out
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((d == -7.0).all())                                                # refused calls write nothing
    idx_only = torch.empty(N, K, dtype=torch.int32, device=dev)
    assert L.gh_knn_indices(ptr(pd), N, K, ptr(idx_only), None, ptr(ws), nbytes, s) == _abi.GH_OK             # dist_out = NULL
    assert L.gh_knn_indices(ptr(pd), N, K, ptr(idx), ptr(d), ptr(ws), nbytes, s) == _abi.GH_OK
    torch.cuda.synchronize()
    want_idx, want_d = oracle_c.knn(p, K)
    assert torch.equal(idx_only, idx)
    assert torch.equal(idx.cpu(), want_idx) and same_bits(d.cpu(), want_d)
