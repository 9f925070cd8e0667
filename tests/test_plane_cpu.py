"""The plane fetch on the host (guassianhand_amd/plane.py): its plain-torch restatement and the bound query_triplane_texture against
outputs and gradients CAPTURED from the reference's own method (tests/golden/make_plane_fixture.py -> plane_fixture.npz), the index
contract against uvmap.ActiveTexels, the C-ABI's symbols and host-side argument checks, and the opt-in renderer names. No GPU
compute is launched here."""
import ctypes as C
import os
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import _abi, uvmap
from guassianhand_amd import plane as P
from tests.helpers import GoldenNpz, header_symbols

PLANES = ("big", "small")
RADII = (1.0, 0.5)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return GoldenNpz(os.path.join(golden_dir, "plane_fixture.npz"))


def fixture_case(fx, tag, r):
    """(plane (C,Hp,Wp), positions (N,2), cotangent (N,C)) of plane `tag` at radius_texture r."""
    return torch.tensor(fx[f"{tag}_plane_q"]).float() / 4.0, torch.tensor(fx[f"{tag}_r{r}_pos"]), torch.tensor(fx[f"{tag}_cot_q"]).float() / 8.0


def test_fixture_holds_what_it_promises(fx):
    assert [float(r) for r in fx["radii"]] == list(RADII)
    for tag, shape in (("big", (80, 64, 128)), ("small", (3, 5, 7))):
        assert fx[f"{tag}_plane_q"].shape == shape and fx[f"{tag}_uv"].shape == (64, 2)
        uv = torch.tensor(fx[f"{tag}_uv"])
        assert int((uv.abs() == 1.0).all(1).sum()) >= 4                  # the four corners, exactly
        assert 3 <= int((uv.abs() > 1.0).any(1).sum()) <= 8              # a few just outside
        for r in RADII:
            assert fx[f"{tag}_r{r}_batched_grad"].shape == shape and fx[f"{tag}_r{r}_unbatched_out"].shape == (64, shape[0])


@pytest.mark.parametrize("tag", PLANES)
@pytest.mark.parametrize("r", RADII)
def test_restatement_reproduces_the_reference_bit_for_bit(fx, tag, r):
    """plane_sample on CPU tensors (and ops="torch") is the reference's grid_sample call on the same build: outputs and the plane's
    gradient equal the recorded ones bitwise."""
    plane, pos, cot = fixture_case(fx, tag, r)
    uv = (pos - (-r)) / (r - (-r)) * 2 + (-1)
    for kw in ({}, {"ops": "torch"}):
        p = plane.clone().requires_grad_(True)
        out = P.plane_sample(p[None], uv[None], **kw)
        assert out.dtype == torch.float32 and tuple(out.shape) == (1, 64, plane.shape[0])
        (out[0] * cot).sum().backward()
        assert torch.equal(out[0].detach(), torch.tensor(fx[f"{tag}_r{r}_batched_out"]))
        assert torch.equal(p.grad, torch.tensor(fx[f"{tag}_r{r}_batched_grad"]))
    five = P.plane_sample(plane[None, None], uv[None])                     # the (B,1,C,Hp,Wp) form
    assert torch.equal(five[0], torch.tensor(fx[f"{tag}_r{r}_batched_out"]))
    o64 = P._plane_sample_ref(plane[None], uv[None], acc=torch.float64)
    assert o64.dtype == torch.float64
    ref = torch.tensor(fx[f"{tag}_r{r}_batched_out"]).double()
    # float32 rounds the texel coordinate three times (u + 1, * 0.5, * (Wp - 1)) and the weight once: 4 * 2^-24 * (Wp - 1) per axis,
    # and a weight error moves the result by at most the difference of two texels, 2 * max|plane|
    Hp, Wp = plane.shape[1:]
    assert float((o64[0] - ref).abs().max()) <= 2.0 ** -24 * 4 * (Hp + Wp) * 2 * float(plane.abs().max())


@pytest.mark.parametrize("tag", PLANES)
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("form", ["batched", "unbatched"])
def test_bound_method_reproduces_the_reference_bit_for_bit(fx, tag, r, form):
    plane, pos, cot = fixture_case(fx, tag, r)
    me = SimpleNamespace(cfg=SimpleNamespace(radius_texture=r))
    assert P.fuse_plane_fetch(me) is me and me.query_triplane_texture.__func__ is P.query_triplane_texture
    p = plane.clone().requires_grad_(True)
    if form == "batched":
        out = me.query_triplane_texture(pos[None], p[None, None])
        assert tuple(out.shape) == (1, 64, plane.shape[0])
        out = out[0]
    else:
        out = me.query_triplane_texture(pos, p[None])
        assert tuple(out.shape) == (64, plane.shape[0])
    (out * cot).sum().backward()
    assert torch.equal(out.detach(), torch.tensor(fx[f"{tag}_r{r}_{form}_out"]))
    assert torch.equal(p.grad, torch.tensor(fx[f"{tag}_r{r}_{form}_grad"]))


def edge_uvs(n, seed):
    """Uniform in [-1.1, 1.1] with rows at exactly +-1, 0 and just outside."""
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand(n, 2, generator=g) * 2.2 - 1.1
    fixed = torch.tensor([[-1, -1], [1, -1], [-1, 1], [1, 1], [0, 0], [1, 0.3], [-0.4, -1], [1 + 2.0 ** -10, 0.0], [-1.09, -1.09]])
    k = min(n, fixed.shape[0])
    uv[:k] = fixed[:k]
    return uv


def loop_contract(uv, Hp, Wp):
    """The index contract as a loop: pairs e = 4n + corner in ascending e, each appended to the list of its texel when the corner is
    inside the map. float32 arithmetic through torch scalars."""
    lists = [[] for _ in range(Hp * Wp)]
    one, half = torch.tensor(1.0), torch.tensor(0.5)
    for n in range(uv.shape[0]):
        ix = ((uv[n, 0] + one) * half) * torch.tensor(float(Wp - 1))
        iy = ((uv[n, 1] + one) * half) * torch.tensor(float(Hp - 1))
        x0, y0 = int(torch.floor(ix)), int(torch.floor(iy))
        for corner in range(4):
            x, y = x0 + (corner & 1), y0 + (corner >> 1)
            if 0 <= x < Wp and 0 <= y < Hp:
                lists[y * Wp + x].append(4 * n + corner)
    return lists


@pytest.mark.parametrize("n,Hp,Wp", [(9, 1, 1), (40, 2, 3), (200, 5, 7), (300, 16, 9)])
def test_index_contract_equals_active_texels(n, Hp, Wp):
    """index_contract (what PlaneIndex builds on the device): pairs grouped by texel, ascending 4n + corner, out-of-map corners absent
    — equal to the loop statement and to ActiveTexels.pairs / row_ptr once its compact slots are mapped back to texels; weights
    bitwise ActiveTexels.w."""
    uv = edge_uvs(n, seed=n)
    ts, pairs, w = P.index_contract(uv, Hp, Wp)
    assert ts.dtype == pairs.dtype == torch.int32 and w.dtype == torch.float32
    assert tuple(ts.shape) == (Hp * Wp + 1,) and tuple(w.shape) == (4 * n,) and int(ts[0]) == 0 and int(ts[-1]) == pairs.numel()
    lists = loop_contract(uv, Hp, Wp)
    assert [pairs[int(ts[t]):int(ts[t + 1])].tolist() for t in range(Hp * Wp)] == lists
    assert sum(len(l) for l in lists) < 4 * n                             # some corners were outside
    at = uvmap.ActiveTexels(uv, Hp, Wp)
    assert torch.equal(w.reshape(n, 4), at.w)
    active = at.index.tolist()
    assert [t for t in range(Hp * Wp) if lists[t]] == active
    for u, t in enumerate(active):
        assert at.pairs[int(at.row_ptr[u]):int(at.row_ptr[u + 1])].tolist() == lists[t], t
    cpu = P.PlaneIndex(uv, Hp, Wp)                                        # CPU tensors: the same lists
    assert torch.equal(cpu.texel_start, ts) and torch.equal(cpu.pairs, pairs) and torch.equal(cpu.w, w)


def test_library_exports_the_plane_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.PLANE_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_plane(L)
    assert sorted(_abi.PLANE_SYMBOLS) == header_symbols("gh_plane.h")
    assert set(_abi.PLANE_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    ws = L.gh_plane_workspace
    for N, Cc, Hp, Wp in ((-1, 80, 64, 128), (10, 0, 64, 128), (10, 80, 0, 128), (10, 80, 64, 0), (10, -3, 64, 128), (2 ** 30, 80, 64, 128),
                          (10, 80, 65536, 65536)):
        assert ws(N, Cc, Hp, Wp) == 0, (N, Cc, Hp, Wp)
    copy = 80 * 64 * 128 * 4
    assert copy <= ws(0, 80, 64, 128) < copy + 256                       # no points: the channel-last copy alone
    assert ws(98562, 80, 100, 100) == ws(0, 80, 100, 100)                # above the sort's limit: the forward alone
    _abi.declare_pool(L)
    plan = L.gh_pool_plan_workspace(4 * 98562, 64 * 128)
    assert plan > 0 and ws(98562, 80, 64, 128) >= max(copy, 16 * 98562 + 4 + plan)
    assert ws(98562, 1, 64, 128) == ws(98562, 80, 64, 128)               # the index part is the larger one, whatever C
    assert ws(1, 1, 1, 1) > 0 and ws(1, 1, 90, 91) > 0


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for bad sizes, null or misaligned pointers, too many texels and a short workspace (fake addresses: nothing is
    launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_plane(L)
    one, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2)
    bad, big = _abi.GH_ERR_INVALID_ARG, 1 << 40

    def fwd(N=10, Cc=80, Hp=64, Wp=128, plane=one, uv=one, out=one, ws=one, nbytes=big):
        return L.gh_plane_sample_forward(plane, uv, out, N, Cc, Hp, Wp, ws, nbytes, None)

    assert fwd(N=-1) == fwd(Cc=0) == fwd(Hp=0) == fwd(Wp=0) == fwd(Wp=-5) == bad
    assert fwd(plane=None) == fwd(uv=None) == fwd(out=None) == fwd(ws=None) == fwd(plane=odd) == fwd(out=odd) == bad
    assert fwd(ws=C.c_void_p((1 << 20) + 4)) == bad
    assert fwd(nbytes=80 * 64 * 128 * 4 - 1) == _abi.GH_ERR_WORKSPACE_SMALL
    assert fwd(Hp=65536, Wp=65536) == _abi.GH_ERR_UNSUPPORTED
    assert fwd(N=0) == fwd(N=0, plane=None, uv=None, out=None, ws=None, nbytes=0) == _abi.GH_OK      # no points: nothing to launch

    def index(N=10, Hp=64, Wp=128, uv=one, ts=one, pairs=one, w=one, ws=one, nbytes=big):
        return L.gh_plane_index(uv, N, Hp, Wp, ts, pairs, w, ws, nbytes, None)

    assert index(N=-1) == index(Hp=0) == index(Wp=0) == bad
    assert index(uv=None) == index(ts=None) == index(pairs=None) == index(w=None) == index(ws=None) == index(w=odd) == bad
    assert index(Hp=3, Wp=2731) == index(Hp=8193, Wp=1) == index(Hp=100, Wp=100) == _abi.GH_ERR_UNSUPPORTED       # 8193 texels
    assert index(Hp=3, Wp=2731, N=-1) == bad
    assert index(nbytes=16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert index(nbytes=L.gh_plane_workspace(10, 1, 64, 128) - 256) == _abi.GH_ERR_WORKSPACE_SMALL

    def bwd(N=10, Cc=80, Hp=64, Wp=128, g=one, ts=C.c_void_p(1 << 30), pairs=C.c_void_p(1 << 31), w=C.c_void_p(1 << 32), gp=C.c_void_p(1 << 33)):
        return L.gh_plane_sample_backward(g, ts, pairs, w, gp, N, Cc, Hp, Wp, None)

    assert bwd(N=-1) == bwd(Cc=0) == bwd(Hp=0) == bwd(Wp=0) == bad
    assert bwd(g=None) == bwd(ts=None) == bwd(pairs=None) == bwd(w=None) == bwd(gp=None) == bwd(gp=odd) == bad
    assert bwd(gp=one) == bwd(gp=C.c_void_p(1 << 30)) == bwd(gp=C.c_void_p((1 << 31) - 64)) == bad       # the gradient overlaps an input


def test_python_refuses_bad_arguments_on_the_host():
    planes, uv = torch.zeros(1, 3, 5, 7), torch.zeros(1, 6, 2)
    assert tuple(P.plane_sample(planes, uv).shape) == (1, 6, 3)
    assert tuple(P.plane_sample(planes, uv[:, :0]).shape) == (1, 0, 3)
    with pytest.raises(ValueError, match="ops"):
        P.plane_sample(planes, uv, ops="eager")
    with pytest.raises(ValueError, match="planes"):
        P.plane_sample(planes[0], uv)
    with pytest.raises(ValueError, match="planes"):
        P.plane_sample(torch.zeros(1, 2, 3, 5, 7), uv)
    with pytest.raises(ValueError, match="uv"):
        P.plane_sample(planes, uv[0])
    with pytest.raises(ValueError, match="uv"):
        P.plane_sample(planes, torch.zeros(2, 6, 2))
    with pytest.raises(ValueError, match="uv"):
        P.PlaneIndex(torch.zeros(6, 3), 5, 7)
    with pytest.raises(TypeError, match="float32"):
        P.PlaneIndex(torch.zeros(6, 2, dtype=torch.float64), 5, 7)
    with pytest.raises(ValueError, match="8192"):
        P.PlaneIndex(torch.zeros(6, 2), 3, 2731)
    with pytest.raises(ValueError, match="1 x 1"):
        P.PlaneIndex(torch.zeros(6, 2), 0, 7)


def test_uv_gradient_comes_from_torch():
    g = torch.Generator().manual_seed(2)
    planes = torch.randn(1, 3, 5, 7, generator=g)
    uv = (torch.rand(1, 6, 2, generator=g) * 1.8 - 0.9).requires_grad_(True)
    P.plane_sample(planes, uv).sum().backward()
    assert uv.grad is not None and float(uv.grad.abs().max()) > 0


def test_opt_in_renderer_names_resolve_lazily():
    """tgs_renderer's four new names exist beside the old ones and, like them, import nothing of the reference until asked for."""
    import guassianhand_amd.tgs_renderer as T
    assert [T._VARIANTS[s] for s in ("FusedHead", "FusedGate", "FusedAll")] == [("head",), ("gate",), ("gate", "head")]
    assert T._VARIANTS["FusedFetch"] == ("fetch",) and T._VARIANTS["FusedAllFetch"] == ("gate", "head", "fetch")
    assert T._GRAFTS["fetch"][:2] == ("plane", "fuse_plane_fetch")
    with pytest.raises(AttributeError):
        T.GS3DRendererFetch
    for name in ("GS3DRendererFusedFetch", "GS3DRendererEditFusedFetch", "GS3DRendererFusedAllFetch", "GS3DRendererEditFusedAllFetch"):
        try:                                                       # the name is known: resolving it reaches for the reference's classes
            cls = getattr(T, name)
        except ImportError:
            continue
        assert isinstance(cls, type) and callable(cls.configure)
