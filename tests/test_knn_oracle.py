"""kNN oracle (oracle/gh_oracle.c:gho_knn) against an independent numpy restatement of pytorch3d's knn_points as the
reference calls it (infer_one_shot.py:247-248: self-query, K=100, sorted) and the mask arithmetic of :249."""
import numpy as np
import pytest
import torch

from oracle import oracle_c
from tests.knn_cases import CLOUDS, PAIRS, case_cloud, cloud, dense_knn, float64_knn, numpy_knn


def test_oracle_knn_matches_dense_numpy_restatement():
    g = torch.Generator().manual_seed(5)
    p = torch.rand(700, 3, generator=g)
    p[100:110] = p[0:10]                       # exact duplicates: distance ties, resolved by index
    p[200:300, 2] = 0.5                        # a coplanar patch
    idx, d = oracle_c.knn(p, 100)
    want_idx, want_d = numpy_knn(p.numpy(), 100)
    assert np.array_equal(idx.numpy(), want_idx)
    assert np.array_equal(d.numpy(), want_d)
    assert np.array_equal(idx[:, 0].numpy()[:100], np.arange(100))      # self first (for duplicates: the lower index)
    assert (idx[100:110, 0].numpy() == np.arange(10)).all()


def test_oracle_knn_query_subset_and_mask():
    g = torch.Generator().manual_seed(6)
    p = torch.randn(500, 3, generator=g)
    full, _ = oracle_c.knn(p, 32)
    qs = torch.tensor([3, 499, 17, 3], dtype=torch.int32)
    sub, _ = oracle_c.knn(p, 32, queries=qs)
    assert torch.equal(sub, full[qs.long()])
    # rigid motion keeps every neighbour list -> nothing flagged; a shuffled second set flags nearly everything
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    moved = p.double() @ R.double().T + 0.25
    m_same = oracle_c.interaction_mask(p, p.clone(), K=32, min_same=10)
    assert not m_same.any()
    m_rigid = oracle_c.interaction_mask(p, moved.float(), K=32, min_same=10)
    assert m_rigid.float().mean() < 0.05                                # only rounding-induced rank swaps
    m_diff = oracle_c.interaction_mask(p, torch.randn(500, 3, generator=g), K=32, min_same=10)
    assert m_diff.float().mean() > 0.95


# ---- the oracle itself at the shapes of the edge sweep (tests/knn_cases.py): the device is compared with gho_knn there, so gho_knn is pinned there

@pytest.mark.parametrize("name", CLOUDS)
def test_oracle_knn_equals_restatement_on_the_edge_sweep(name):
    bad = []
    for N, K in PAIRS:
        p = case_cloud(name, N)
        idx, d = oracle_c.knn(p, K)
        want_idx, want_d = dense_knn(name, N)
        # distances are compared as bits: -0.0 / +0.0 and NaN would slip through a float comparison
        if not (np.array_equal(idx.numpy(), want_idx[:, :K]) and np.array_equal(d.numpy().view(np.uint32), want_d[:, :K].view(np.uint32))):
            bad.append((N, K))
    assert not bad, f"{name}: oracle != numpy restatement at (N, K) = {bad}"


def test_signed_cloud_holds_both_zeros():
    p = case_cloud("signed", 700)
    assert bool(torch.signbit(p[::7, 0]).all()) and bool((p[::7, 0] == 0).all())
    assert bool((p[::11, 1] == 0).all()) and not bool(torch.signbit(p[::11, 1]).any())
    assert bool((p < 0).any()) and bool((p > 0).any())


def test_oracle_knn_equals_float64_argsort_where_distances_are_exact():
    """dyadic: coordinates are multiples of 1/64 below 1, so a squared distance is a multiple of 2^-12 below 3: exact in float32 however
    it is accumulated, and the answer is the stable argsort of the float64 distances, with no model of the fused multiply-adds."""
    for N, K in PAIRS:
        p = case_cloud("dyadic", N)
        idx, d = oracle_c.knn(p, K)
        want_idx, want_d = float64_knn(p, K)
        assert torch.equal(idx, want_idx), (N, K)
        assert torch.equal(d.double(), want_d), (N, K)
    assert int((want_d[:, 1:] == want_d[:, :-1]).sum()) > 700 * 5         # (700, 100): several tied neighbour pairs in every row on average


@pytest.mark.parametrize("name", ["uniform", "dyadic"])
def test_oracle_knn_commutes_with_power_of_two_scaling(name):
    """Scaling by 2^k is exact in every operation as long as nothing leaves the normal range: same lists, distances times 4^k."""
    p = cloud(name, 300, 7)
    idx, d = oracle_c.knn(p, 100)
    assert float(d[d > 0].min()) * 4.0 ** -40 > 1e-30                   # well inside the normal range
    for k in (-40, 40):
        idx_k, d_k = oracle_c.knn(p * 2.0 ** k, 100)
        assert torch.equal(idx_k, idx), k
        assert torch.equal(d_k, d * 4.0 ** k), k


@pytest.mark.parametrize("name", ["uniform", "dyadic"])
def test_oracle_knn_below_the_domain_is_the_first_k_indices(name):
    """At 2^-100 every squared distance underflows to 0: all points tie, and the brute-force order is the index order."""
    p = cloud(name, 300, 7) * 2.0 ** -100
    assert bool((p[:, 0] != p[0, 0]).any())                               # the coordinates themselves are still distinct normal numbers
    idx, d = oracle_c.knn(p, 100)
    assert torch.equal(idx, torch.arange(100, dtype=torch.int32).expand(300, 100))
    assert bool((d == 0).all())
