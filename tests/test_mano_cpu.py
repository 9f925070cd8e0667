"""guassianhand_amd.mano without a GPU: the subdivision tables against the reference's recorded edge_subdivide results, the closed-form
counts, the plain-torch restatement against float64 loops and against gradcheck, the CPU convention of ops="fused", and the C-ABI's
symbols and argument checks (the library cross-compiles for gfx950 here; nothing is launched)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi, _lib, scenes
from guassianhand_amd import mano as M
from tests import mano_cases as MC
from tests.helpers import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mano_subdivide_fixture.npz")


def _fixture_model(fx, faces):
    V = fx["vertices"].shape[0]
    return M.HandModel(fx["vertices"], np.zeros((V, 3, 1)), np.zeros((0, 3 * V)), np.full((1, V), 1.0 / V), [-1], np.ones((V, 1)), np.zeros(3),
                       faces, levels=3)


@pytest.mark.parametrize("tag,faces_key", [("a", "faces"), ("b", "faces_b")])
def test_tables_are_the_reference_edge_subdivide(tag, faces_key):
    """Per level, edges and faces exactly; the folded stencil's points within 4 ulp of max|coordinate|: the weights are exact dyadics, the
    stencil rounds at most twice and the reference's level-by-level float64 path rounds once on its way to the recorded float32."""
    fx = np.load(FIXTURE)
    m = _fixture_model(fx, fx[faces_key])
    for l in (1, 2, 3):
        assert np.array_equal(m.edges[l - 1], fx[f"{tag}_l{l}_edges"]), l
        assert np.array_equal(m.faces[l], fx[f"{tag}_l{l}_faces"]), l
    want = fx[f"{tag}_l3_vertices"]
    assert m.n_points == want.shape[0] and tuple(m.faces_subdivided.shape) == (64 * fx["faces"].shape[0], 3)
    got = m.stencil_points(torch.from_numpy(fx["vertices"])).numpy()
    ulp = float(np.abs(want).max()) * 2.0 ** -23
    err = float(np.abs(got.astype(np.float64) - want).max()) / ulp
    print(f"stencil against the recorded vertices: {err:.2f} ulp of max|coordinate|")
    assert err <= 4.0
    assert np.array_equal(got[:20], fx["vertices"])
    # every weight a multiple of 1/8, rows summing to 1, at most three vertices; the transpose holds the same entries
    w = m.stencil_w.numpy()
    assert np.array_equal(w * 8, np.round(w * 8)) and np.array_equal(w.sum(1), np.ones(m.n_points, dtype=np.float32))
    assert int(m.tr_ptr[-1]) == int((w != 0).sum()) == m.tr_point.numel()
    dense = np.zeros((m.n_points, 20))
    np.add.at(dense, (np.repeat(np.arange(m.n_points), 3), m.stencil_idx.numpy().reshape(-1)), w.reshape(-1))
    back = np.zeros_like(dense)
    rows = np.repeat(np.arange(20), np.diff(m.tr_ptr.numpy()))
    back[m.tr_point.numpy(), rows] = m.tr_w.numpy()
    assert np.array_equal(dense, back)
    assert all(np.all(np.diff(m.tr_point.numpy()[a:b]) > 0) for a, b in zip(m.tr_ptr.numpy()[:-1], m.tr_ptr.numpy()[1:]))


def test_the_two_windings_own_different_tables():
    fx = np.load(FIXTURE)
    a, b = _fixture_model(fx, fx["faces"]), _fixture_model(fx, fx["faces_b"])
    assert not np.array_equal(a.edges[0], b.edges[0]) and not torch.equal(a.stencil_idx, b.stencil_idx)


def test_closed_form_counts():
    assert M.point_count(778, 1538, 0) == 778 and M.point_count(778, 1538, 1) == 3093 and M.point_count(778, 1538, 2) == 12337
    assert M.point_count(778, 1538, 3) == 49281 == scenes.P_HAND
    for nx, ny in ((2, 2), (4, 5), (3, 86)):
        for levels in (0, 1, 3):
            m = M.synthetic_model(nx, ny, J=2, NB=1, levels=levels)
            assert m.n_points == M.point_count(nx * ny, 2 * (nx - 1) * (ny - 1), levels) and m.faces_subdivided.shape[0] == 2 * (nx - 1) * (ny - 1) * 4 ** levels


def test_synthetic_model_is_well_conditioned():
    m = M.synthetic_model(3, 4)
    assert m.parents == M.MANO_PARENTS and m.J == 16 and m.NB == 10 and m.V == 12
    assert torch.allclose(m.lbs_weights.sum(1), torch.ones(12)) and torch.allclose(m.J_regressor.sum(1), torch.ones(16))
    assert float(m.pose_mean.abs().max()) > 0
    f, g = M.synthetic_model(3, 4, flip=True).faces[0], m.faces[0]
    assert np.array_equal(f, g[:, [0, 2, 1]])


def test_model_is_validated():
    m = M.synthetic_model(3, 3, J=2, NB=1)
    args = lambda **kw: {**dict(v_template=m.v_template, shapedirs=m.shapedirs, posedirs=m.posedirs, J_regressor=m.J_regressor,
                                parents=[-1, 0], lbs_weights=m.lbs_weights, pose_mean=m.pose_mean, faces=m.faces[0]), **kw}
    M.HandModel(**args())
    for bad in (dict(parents=[-1, 1]), dict(parents=[0, 0]), dict(levels=4), dict(levels=-1), dict(faces=m.faces[0] + 8),
                dict(posedirs=m.posedirs[:, :-1]), dict(lbs_weights=m.lbs_weights.t()), dict(pose_mean=m.pose_mean[:3]),
                dict(v_template=m.v_template[:0]), dict(J_regressor=m.J_regressor[:1])):
        with pytest.raises(ValueError):
            M.HandModel(**args(**bad))

    class Layer:
        pass
    layer = Layer()
    for k, v in args().items():
        setattr(layer, k, v)
    layer.parents = torch.tensor([-1, 0])
    again = M.HandModel.from_layer(layer, levels=1)
    assert again.levels == 1 and again.n_points == M.point_count(9, 8, 1) and torch.equal(again.posedirs, m.posedirs)


@pytest.mark.parametrize("J", [1, 2, 16])
def test_ref_is_the_hand_written_loops(J):
    m = M.synthetic_model(3, 3, J=J, NB=3, levels=2, seed=J)
    go, hp, be, tr = MC.params(2, 1, J, 3, seed=4)
    pts, jts = M.mano_ref(m, go[:, 0], hp[:, 0], be[:, 0], tr[:, 0], acc=torch.float64)
    for b in range(2):
        want_p, want_j = MC.loops(m, go[b, 0], hp[b, 0], be[b, 0], tr[b, 0])
        for got, want in ((pts[b].numpy(), want_p), (jts[b].numpy(), want_j)):
            assert got.shape == want.shape
            assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max())


@pytest.mark.parametrize("zero", [False, True])
def test_ref_passes_gradcheck(zero):
    """float64 autograd of mano_ref against finite differences; zero pose with a zero pose_mean is the |1e-8| branch of the rotation."""
    m = M.synthetic_model(2, 3, J=3, NB=2, levels=1, seed=5)
    if zero:
        m.pose_mean.zero_()
    ps = [p[:, 0].double() for p in MC.params(1, 1, 3, 2, seed=6)]
    if zero:
        ps[0], ps[1] = torch.zeros_like(ps[0]), torch.zeros_like(ps[1])
    ps = [p.requires_grad_(True) for p in ps]
    assert torch.autograd.gradcheck(lambda *a: M.mano_ref(m, *a, acc=torch.float64), ps, eps=1e-6, atol=1e-6, rtol=1e-4)


def test_cpu_tensors_take_the_torch_statements():
    ms = MC.models(4, 2, 1, 1, 2)
    ps = [p.requires_grad_(True) for p in MC.params(3, 2, 2, 1)]
    out = M.pose_hands(ms, *ps)
    ref = M.pose_hands(ms, *ps, ops="torch")
    assert torch.equal(out.points, ref.points) and torch.equal(out.joints, ref.joints)
    assert tuple(out.points.shape) == (3, sum(m.n_points for m in ms), 3) and tuple(out.joints.shape) == (3, 4, 3)
    one = M.mano_ref(ms[1], *(p[:, 1] for p in ps))
    assert torch.equal(out.points[:, ms[0].n_points:], one[0]) and torch.equal(out.joints[:, 2:], one[1])
    (out.points.sum() + out.joints.sum()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in ps)
    empty = M.pose_hands(ms, *(p[:0].detach() for p in ps))
    assert tuple(empty.points.shape) == (0, out.points.shape[1], 3) and tuple(empty.joints.shape) == (0, 4, 3)
    assert M.pose_hands(ms[0], *(p[:, :1].detach().double() for p in ps)).points.dtype == torch.float64
    with pytest.raises(ValueError):
        M.pose_hands(ms, *ps, ops="triton")
    with pytest.raises(ValueError):
        M.pose_hands(ms[:1], *ps)
    with pytest.raises(ValueError):
        M.pose_hands((ms[0], MC.model(4, 2, 10, 1)), *ps)


def test_library_exports_the_mano_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.MANO_SYMBOLS:
        assert hasattr(L, sym), sym
    assert sorted(_abi.MANO_SYMBOLS) == header_symbols("gh_mano.h") and set(_abi.MANO_SYMBOLS) <= set(_abi.ALL_SYMBOLS)
    assert not set(_abi.MANO_SYMBOLS) & set(_abi.EXPORTED_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    assert any(s.endswith("gh_mano.hip") for s in _lib.SOURCES) and any(h.endswith("gh_mano.h") for h in _lib.HEADERS)
    h = open(os.path.join(ROOT, "include", "gh_mano.h")).read()
    for name in ("GH_MANO_MAX_H", "GH_MANO_MAX_J", "GH_MANO_MAX_NB", "GH_MANO_MAX_LEVELS", "GH_MANO_MAX_V", "GH_MANO_MAX_P", "GH_MANO_MAX_B",
                 "GH_MANO_CHUNK"):
        assert f"#define {name} {getattr(_abi, name)} " in h, name


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes in the header's order (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare(L)
    one, odd = 1 << 20, (1 << 20) + 2
    INV, UNS, OK, SMALL = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED, _abi.GH_OK, _abi.GH_ERR_WORKSPACE_SMALL

    def mk(V=8, P=20, levels=1, nnz=None, parents=(-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14), **ptrs):
        m = _abi.GhManoModel()
        m.V, m.P, m.levels, m.nnz = V, P, levels, (2 * P if nnz is None else nnz)
        for i, p in enumerate(parents):
            m.parents[i] = p
        for n in _abi.MANO_MODEL_ARRAYS:
            setattr(m, n, ptrs.get(n, one))
        return m

    def fwd(B=1, H=1, J=16, NB=10, model=None, points=one, joints=one, ws=one, ws_bytes=1 << 30, params=(one, one, one, one)):
        dims = _abi.GhManoDims(B, H, J, NB)
        arr = (_abi.GhManoModel * max(H, 1))(*[model or mk()] * max(H, 1))
        return L.gh_mano_forward(C.byref(dims), arr, C.byref(_abi.GhManoParams(*params)), points, joints, ws, ws_bytes, None)

    def bwd(B=1, H=1, J=16, NB=10, model=None, dp=one, dj=one, grads=(one, one, one, one), ws=one, ws_bytes=1 << 30):
        dims = _abi.GhManoDims(B, H, J, NB)
        arr = (_abi.GhManoModel * max(H, 1))(*[model or mk()] * max(H, 1))
        return L.gh_mano_backward(C.byref(dims), arr, dp, dj, C.byref(_abi.GhManoGrads(*grads)), ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(B=-1) == call(H=0) == call(J=0) == call(NB=0) == INV
        assert call(J=17) == call(NB=17) == call(H=5) == call(B=65536) == UNS
        assert call(model=mk(V=0, P=0)) == call(model=mk(P=7)) == call(model=mk(levels=-1)) == call(model=mk(nnz=19)) == INV
        assert call(model=mk(levels=0)) == INV                                                  # levels = 0 with P != V
        assert call(model=mk(parents=(-1, 1) + (0,) * 14)) == call(model=mk(parents=(-1, 0, 2) + (0,) * 13)) == INV     # parents[i] >= i
        assert call(model=mk(parents=(0,) * 16)) == call(model=mk(parents=(-1, -1) + (0,) * 14)) == INV
        assert call(model=mk(levels=4)) == call(model=mk(V=65537, P=65537)) == call(model=mk(V=8, P=4194305)) == UNS
        assert call(ws=None) == call(ws=odd) == call(model=mk(lbs_weights=None)) == call(model=mk(pose_mean=odd)) == INV
        assert call(B=0) == OK                                                                  # empty: nothing launched
        assert call(ws_bytes=64) == SMALL
    assert fwd(points=None) == fwd(joints=None) == fwd(points=odd) == INV                      # a null output
    assert fwd(params=(None, one, one, one)) == fwd(params=(one, None, one, one)) == fwd(params=(one, one, one, odd)) == INV
    assert fwd(model=mk(st_idx=None)) == INV and bwd(model=mk(tr_ptr=None)) == INV
    assert fwd(B=0, J=1, params=(one, None, one, one), model=mk(V=8, P=8, levels=0, posedirs=None, st_idx=None, st_w=None)) == OK
    assert bwd(grads=(None, None, None, None)) == OK and bwd(grads=(one, odd, one, one)) == INV
    assert bwd(B=0, dp=None, dj=None) == OK
    dims = _abi.GhManoDims(2, 1, 16, 10)
    assert L.gh_mano_workspace_bytes(C.byref(dims), C.byref(mk())) > 2 * (624 + 3 * 3 * 8) * 4
    assert L.gh_mano_workspace_bytes(C.byref(_abi.GhManoDims(2, 1, 17, 10)), C.byref(mk())) == 0
    assert L.gh_mano_workspace_bytes(C.byref(dims), C.byref(mk(levels=4))) == 0
