"""The UV search on the host (guassianhand_amd/uvd.py): its plain-torch restatement against an independent float64 loop
(tests/uvd_cases.py) on the hand template and on a grid, known answers, the tie rule, degenerate and invalid faces, get_uvd's return,
the differentiable path, the livehand shim, the renderer hook, the C-ABI's symbols and refusals. No GPU compute is launched here."""
import ctypes as C
import importlib
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import uvd as U
from tests import uvd_cases as K
from tests.helpers import header_symbols


def _against_the_loop(tag, points, verts, faces, face_uv):
    """closest_uv_ref in float32 and float64 against the loop. The bounds come from the number formats: a closest point is a handful
    of sums of products of quantities no larger than the mesh's extent, each rounded to 2^-24 (2^-53) of it, and the 2 x 2 solve of a
    face whose angles are not small multiplies that by a few tens: 2^-18 (2^-44) of the bounding-box diagonal for (a) and (b). (c)
    compares a three-term sum with itself in float64: 2^-22 (2^-48) of max |face_uv|."""
    d64 = K.loop_reference(points, verts, faces)
    diag, uvmax = K.scales(verts, faces, face_uv)
    for name, acc, ea, ec in (("float32", None, 2.0 ** -18, 2.0 ** -22), ("float64", torch.float64, 2.0 ** -44, 2.0 ** -48)):
        out = U.closest_uv_ref(points, verts, faces, face_uv, acc=acc)
        assert out[0].dtype == out[1].dtype == out[3].dtype == (acc or torch.float32) and out[2].dtype == torch.int64
        m = K.measure(points, verts, faces, face_uv, out, d64)
        print(f"uvd ref {tag} {name}: (a) {m['a'] / diag:.3g} x diag  (b) {m['b'] / diag:.3g} x diag  (c) {m['c']:.3g}  bmin {m['bmin']:.3g}")
        assert m["a"] <= ea * diag and m["b"] <= ea * diag and m["c"] <= ec * uvmax, (tag, name, m, diag)
        assert m["bmin"] >= 0.0 and m["bsum"] <= 2.0 ** -21, (tag, name, m)
    return d64


def test_restatement_against_the_loop_on_the_hand(golden_dir):
    verts, faces, face_uv = K.hand_mesh(golden_dir)
    assert verts.shape == (1810, 3) and faces.shape == (3076, 3) and face_uv.shape == (3076, 3, 2)
    assert float(face_uv[..., 0].max()) <= 1.0 and float(face_uv[..., 1].max()) <= 0.5 and float(face_uv.min()) >= 0.0
    pts = K.surface_points(verts, faces, 1024)
    d64 = _against_the_loop("hand", pts, verts, faces, face_uv)
    assert float(np.nanmax(d64)) > 0 and float(np.nanmin(d64)) < 1e-9           # points on the surface and off it
    f32 = U.closest_uv_ref(pts, verts, faces, face_uv)[2]
    f64 = U.closest_uv_ref(pts, verts, faces, face_uv, acc=torch.float64)[2]
    assert 0.5 < float((f32 == f64).float().mean()) < 1.0                         # ties are the normal case: faces are not compared


def test_restatement_against_the_loop_on_a_grid():
    verts, faces, face_uv = K.grid_mesh(200)
    pts = torch.cat([K.surface_points(verts, faces, 300), K.off_surface_points(verts, faces, 200)[0],
                     4.0 * torch.randn(100, 3, generator=torch.Generator().manual_seed(0))])
    _against_the_loop("grid", pts, verts, faces, face_uv)


def test_known_answers_on_the_octahedron():
    """Points c + h n for interior barycentrics: the face is exact and the UV is the closed form to 2^-20."""
    verts, faces, face_uv = K.octahedron()
    g = np.random.default_rng(0)
    k = np.arange(64) % 8
    b = g.dirichlet([1.0, 1.0, 1.0], 64) * 0.7 + 0.1
    tri = verts.double().numpy()[faces.numpy()[k]]
    c = (b[:, :, None] * tri).sum(1)
    n = tri.mean(1) / np.linalg.norm(tri.mean(1), axis=1, keepdims=True)         # a face's normal points from the origin to its centroid
    h = g.uniform(0.05, 0.5, 64)
    pts = torch.tensor((c + h[:, None] * n).astype(np.float32))
    uv, d, face, bary = U.closest_uv(pts, verts, faces, face_uv)
    assert face.tolist() == k.tolist()
    want = (b[:, :, None] * face_uv.double().numpy()[k]).sum(1)
    assert np.abs(uv.double().numpy() - want).max() <= 2.0 ** -20
    assert np.abs(d.double().numpy() - h).max() <= 2.0 ** -20 and np.abs(bary.double().numpy() - b).max() <= 2.0 ** -20


def test_special_cases_on_the_host():
    K.check_special_cases(lambda p, v, f, t: U.closest_uv(p, v, f, t))
    K.check_special_cases(lambda p, v, f, t: U.closest_uv(p, v, f.int(), t, ops="torch"))


def test_get_uvd_returns_the_reference_triple():
    verts, faces, face_uv = K.grid_mesh(20)
    pts = K.surface_points(verts, faces, 50)
    assert faces.dtype == torch.int64
    uv, d, rest = U.get_uvd(pts, verts, faces, face_uv)
    assert tuple(uv.shape) == (50, 2) and tuple(d.shape) == (50,) and sorted(rest) == ["bary", "face"]
    assert uv.is_contiguous() and uv.dtype == torch.float32 and rest["face"].dtype == torch.int64 and tuple(rest["bary"].shape) == (50, 3)
    again = U.get_uvd(pts, verts, faces.int(), face_uv)
    assert torch.equal(again[0], uv) and again[0].data_ptr() != uv.data_ptr()  # a fresh tensor each call
    keep = uv.clone()
    v = uv.unsqueeze(0)                                                        # the caller's statements (renderer_one_shot.py:484-486)
    v[..., 0] = 2.0 * (v[..., 0] / 1) - 1.0
    v[..., 1] = 2.0 * (v[..., 1] / 0.5) - 1.0
    assert torch.equal(uv[:, 0], 2.0 * keep[:, 0] - 1.0) and float(v.min()) >= -1.0 and float(v.max()) <= 1.0
    assert torch.equal(U.get_uvd(pts, verts, faces, face_uv)[0], keep)
    assert tuple(U.get_uvd(pts[:0], verts, faces, face_uv)[0].shape) == (0, 2)
    with pytest.raises(ValueError, match="ops"):
        U.closest_uv(pts, verts, faces, face_uv, ops="eager")
    with pytest.raises(ValueError, match="split"):
        U.closest_uv(pts, verts, faces, face_uv, split=U.MAX_SPLIT + 1)
    with pytest.raises(ValueError, match="face_uv"):
        U.closest_uv(pts, verts, faces, face_uv[:5])
    with pytest.raises(ValueError, match="points"):
        U.closest_uv(pts[None], verts, faces, face_uv)
    with pytest.raises(TypeError, match="faces"):
        U.closest_uv(pts, verts, faces.float(), face_uv)
    with pytest.raises(ValueError, match="at least one"):
        U.closest_uv(pts, verts, faces[:0], face_uv[:0])


# ---- the differentiable path ---------------------------------------------------------------------------------------------------------
def _region_cases():
    """One triangle (and a far one) with points of every region, each at least 1 % of an edge length off the region's boundaries:
    (points, region) with region 0 = interior, 1..3 = the edges ab, bc, ca, 4..6 = the vertices a, b, c."""
    verts = torch.tensor([[0.1, 0.2, 0.0], [1.3, 0.1, 0.2], [0.4, 1.1, -0.1], [5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [5.0, 6.0, 5.0]], dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]])
    a, b, c = verts[0], verts[1], verts[2]
    n = torch.linalg.cross(b - a, c - a)
    n = n / n.norm()
    out = lambda p, q, r: torch.linalg.cross(q - p, n) / (q - p).norm()        # in the plane, away from r's side of pq
    pts = [0.3 * a + 0.3 * b + 0.4 * c + 0.2 * n, 0.6 * a + 0.25 * b + 0.15 * c - 0.1 * n,
           0.4 * a + 0.6 * b + 0.3 * out(a, b, c) + 0.1 * n, 0.5 * b + 0.5 * c + 0.2 * out(b, c, a) - 0.2 * n,
           0.7 * c + 0.3 * a + 0.25 * out(c, a, b),
           a + 0.3 * (a - b) / (a - b).norm() + 0.3 * (a - c) / (a - c).norm() + 0.1 * n,
           b + 0.3 * (b - a) / (b - a).norm() + 0.3 * (b - c) / (b - c).norm(),
           c + 0.3 * (c - a) / (c - a).norm() + 0.3 * (c - b) / (c - b).norm() - 0.1 * n]
    return verts, faces, torch.stack(pts), [0, 0, 1, 2, 3, 4, 5, 6]


def _by_region(p, verts, face_uv, region):
    """(uv, d) of one point against the triangle 0-1-2 by the formulas of its KNOWN region, independent of uvd.py's."""
    a, b, c = verts[0], verts[1], verts[2]
    t = face_uv[0]
    if region == 0:
        n = torch.linalg.cross(b - a, c - a)
        q = p - n * ((p - a) @ n) / (n @ n)
        area = lambda x, y, z: torch.linalg.cross(y - x, z - x) @ n / (n @ n)
        bary = torch.stack([area(q, b, c), area(a, q, c), area(a, b, q)])
    elif region <= 3:
        i, j = [(0, 1), (1, 2), (2, 0)][region - 1]
        x, y = verts[i], verts[j]
        s = (p - x) @ (y - x) / ((y - x) @ (y - x))
        q = x + s * (y - x)
        bary = torch.zeros(3, dtype=p.dtype).index_put((torch.tensor([i, j]),), torch.stack([1 - s, s]))
    else:
        q = verts[region - 4]
        bary = torch.zeros(3, dtype=p.dtype)
        bary[region - 4] = 1.0
    return bary @ t, (p - q).norm()


def test_differentiable_path_against_autograd_of_the_region_formulas():
    verts, faces, pts, regions = _region_cases()
    face_uv = torch.rand(2, 3, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    leaves = [x.clone().requires_grad_(True) for x in (pts, verts, face_uv)]
    uv, d, face, bary = U.closest_uv(leaves[0], leaves[1], faces, leaves[2])
    assert uv.requires_grad and d.requires_grad and face.tolist() == [0] * 8
    w = torch.randn(8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    got = torch.autograd.grad((uv * w[:, :2]).sum() + (d * w[:, 2]).sum(), leaves)
    ref = [x.clone().requires_grad_(True) for x in (pts, verts, face_uv)]
    total = 0.0
    for i, r in enumerate(regions):
        uv_i, d_i = _by_region(ref[0][i], ref[1], ref[2], r)
        assert float((uv_i - uv[i]).detach().abs().max()) < 1e-12 and abs(float((d_i - d[i]).detach())) < 1e-12, (i, r)
        total = total + (uv_i * w[i, :2]).sum() + d_i * w[i, 2]
    want = torch.autograd.grad(total, ref)
    for name, g, h in zip(("points", "verts", "face_uv"), got, want):
        assert float(h.abs().max()) > 0 and float((g - h).abs().max()) <= 1e-10 * max(1.0, float(h.abs().max())), name
    fn = lambda p, v, t: tuple(U.closest_uv(p, v, faces, t)[:2])
    assert torch.autograd.gradcheck(fn, [x.detach().clone().requires_grad_(True) for x in (pts, verts, face_uv)], eps=1e-7, atol=1e-6)
    # float32 and no_grad: the plain outputs, no graph
    with torch.no_grad():
        assert not U.closest_uv(leaves[0], leaves[1], faces, leaves[2])[0].requires_grad
    p32 = pts.float().requires_grad_(True)
    uv32, d32, _, _ = U.closest_uv(p32, verts.float(), faces, face_uv.float())
    assert torch.equal(uv32.detach(), U.closest_uv(pts.float(), verts.float(), faces, face_uv.float())[0])
    (uv32.sum() + d32.sum()).backward()
    assert bool(torch.isfinite(p32.grad).all()) and float(p32.grad.abs().max()) > 0
    on = (0.2 * verts[0] + 0.3 * verts[1] + 0.5 * verts[2])[None].clone().requires_grad_(True)     # on the surface: d = 0, no NaN
    uv0, d0, _, _ = U.closest_uv(on, verts, faces, face_uv)
    (uv0.sum() + d0.sum()).backward()
    assert float(d0.detach()) < 1e-15 and bool(torch.isfinite(on.grad).all())


# ---- the livehand shim and the renderer hook ------------------------------------------------------------------------------------------
@pytest.fixture
def no_livehand(monkeypatch):
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "livehand" or k.startswith("livehand.")}
    yield
    for k in [k for k in sys.modules if k == "livehand" or k.startswith("livehand.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    importlib.invalidate_caches()


def test_shim_registers_get_uvd_where_livehand_is_absent(no_livehand):
    if importlib.util.find_spec("livehand") is not None:             # a real livehand is installed here: the refusal is what applies
        assert U.install_livehand_shim() is False
        return
    assert U.install_livehand_shim() is True
    from livehand.input_encoder import get_uvd, read_mano_uv_obj, save_obj_for_debugging
    assert get_uvd is U.get_uvd and sys.modules["livehand"].input_encoder is sys.modules["livehand.input_encoder"]
    for stub in (read_mano_uv_obj, save_obj_for_debugging):
        with pytest.raises(NotImplementedError, match=stub.__name__):
            stub("hand.obj")
    assert U.install_livehand_shim() is True and sys.modules["livehand.input_encoder"].get_uvd is U.get_uvd      # idempotent


def test_shim_does_not_replace_an_importable_package(no_livehand, tmp_path, monkeypatch):
    pkg = tmp_path / "livehand"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "input_encoder.py").write_text("def get_uvd(*a):\n    return 'theirs'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    importlib.invalidate_caches()
    assert U.install_livehand_shim() is False and "livehand" not in sys.modules
    from livehand.input_encoder import get_uvd
    assert get_uvd() == "theirs"
    assert U.install_livehand_shim() is False                                 # imported by now: still theirs
    assert U.install_livehand_shim(force=True) is True
    assert sys.modules["livehand.input_encoder"].get_uvd is U.get_uvd


def test_fuse_get_uvd_sets_the_hook_forward_single_batch_reads():
    r = SimpleNamespace(other=1)
    assert U.fuse_get_uvd(r) is r and r.get_uvd is U.get_uvd and r.other == 1
    verts, faces, face_uv = K.grid_mesh(8)
    pts = K.surface_points(verts, faces, 10)
    U.fuse_get_uvd(r, ops="torch", split=2)
    uv, d, rest = r.get_uvd(pts, verts, faces, face_uv)
    assert torch.equal(uv, U.get_uvd(pts, verts, faces, face_uv)[0]) and sorted(rest) == ["bary", "face"]
    src = open(sys.modules["guassianhand_amd.renderer"].__file__).read() if "guassianhand_amd.renderer" in sys.modules else \
        open(importlib.import_module("guassianhand_amd.renderer").__file__).read()
    assert src.count('getattr(self, "get_uvd", None)') == 2                    # forward_single_batch and forward_single_batch_edit


def test_opt_in_renderer_names_resolve_lazily(no_livehand):
    import guassianhand_amd.tgs_renderer as T
    assert T._VARIANTS["FusedUvd"] == ("uvd",) and T._VARIANTS["FusedAllFetchAttnUvd"] == T._VARIANTS["FusedAllFetchAttn"] + ("uvd",)
    assert T._GRAFTS["uvd"][:2] == ("uvd", "fuse_get_uvd")
    with pytest.raises(AttributeError):
        T.GS3DRendererFusedGateUvd
    have_reference = importlib.util.find_spec("tgs") is not None
    for name in ("GS3DRendererFusedUvd", "GS3DRendererEditFusedUvd", "GS3DRendererFusedAllFetchAttnUvd", "GS3DRendererEditFusedAllFetchAttnUvd"):
        if not have_reference:                                     # the name is known: resolving it reaches for the reference's classes
            with pytest.raises(ImportError) as e:
                getattr(T, name)
            assert (e.value.name or "").split(".")[0] == "tgs"      # and for nothing else that is missing
            continue
        cls = getattr(T, name)
        assert isinstance(cls, type) and callable(cls.configure)


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_uvd_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.UVD_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_uvd(L)
    assert sorted(_abi.UVD_SYMBOLS) == header_symbols("gh_uvd.h")
    assert set(_abi.UVD_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    hdr = open(gh_lib_path.replace("guassianhand_amd/libgh_raster.so", "include/gh_uvd.h")).read()
    for name in ("GH_UVD_MAX_SPLIT", "GH_UVD_REC_BYTES", "GH_UVD_TARGET_WGS", "GH_UVD_MIN_CHUNK"):
        assert f"#define {name} {getattr(_abi, name)}" in hdr, name
    from guassianhand_amd import _lib
    assert any(s.endswith("gh_uvd.hip") for s in _lib.SOURCES) and any(h.endswith("gh_uvd.h") for h in _lib.HEADERS)
    ws, auto = L.gh_uvd_workspace_bytes, L.gh_uvd_auto_split
    # the rule of the header, restated
    for N, F in ((98562, 3076), (1, 1), (1000, 200), (64, 3076), (4099, 3076), (1 << 30, 1 << 20), (300000, 127), (256, 128), (257, 256)):
        want = max(1, min(_abi.GH_UVD_TARGET_WGS // ((N + 255) // 256), F // _abi.GH_UVD_MIN_CHUNK, _abi.GH_UVD_MAX_SPLIT))
        assert auto(N, F) == want, (N, F)
    assert auto(1000, 200) == 1 and auto(0, 5) == auto(5, 0) == 1 and 1 < auto(98562, 3076) <= _abi.GH_UVD_MAX_SPLIT
    rec = 256 * ((3076 * _abi.GH_UVD_REC_BYTES + 255) // 256)
    assert ws(98562, 3076, 1) == rec and ws(98562, 3076, 0) == ws(98562, 3076, auto(98562, 3076))
    assert rec + 2 * 4 * 4 * 98562 <= ws(98562, 3076, 4) < rec + 2 * 4 * 4 * 98562 + 512
    assert ws((1 << 31) - 1, 10, 16) > 2 * 16 * 4 * ((1 << 31) - 1)             # 64-bit sizes
    assert ws(0, 5, 1) > 0
    for bad in ((-1, 5, 1), (5, 0, 1), (5, 5, -1), (5, 5, _abi.GH_UVD_MAX_SPLIT + 1)):
        assert ws(*bad) == 0, bad


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for bad sizes, null or misaligned pointers and a short workspace (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_uvd(L)
    one, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2)
    bad = _abi.GH_ERR_INVALID_ARG

    def fwd(N=10, V=4, F=3, split=1, points=one, verts=one, faces=one, face_uv=one, uv=one, dist=one, face=one, bary=one, ws=one, nbytes=1 << 20):
        return L.gh_uvd_forward(points, N, verts, V, faces, face_uv, F, split, uv, dist, face, bary, ws, nbytes, None)

    assert fwd(N=-1) == fwd(V=0) == fwd(F=0) == fwd(split=-1) == fwd(split=_abi.GH_UVD_MAX_SPLIT + 1) == bad
    assert fwd(points=None) == fwd(verts=None) == fwd(faces=None) == fwd(face_uv=None) == fwd(uv=None) == fwd(ws=None) == bad
    assert fwd(points=odd) == fwd(uv=odd) == fwd(dist=odd) == fwd(face=odd) == fwd(bary=odd) == bad
    assert fwd(ws=C.c_void_p((1 << 20) + 4)) == bad
    assert fwd(nbytes=16) == fwd(split=4, nbytes=256) == _abi.GH_ERR_WORKSPACE_SMALL
    assert fwd(N=0) == fwd(N=0, points=None, uv=None, ws=None, nbytes=0) == _abi.GH_OK          # no points: nothing to launch
    assert fwd(N=0, F=0) == fwd(N=0, V=0) == bad                                                   # the sizes are judged first
