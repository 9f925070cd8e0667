"""What the UV search's tests share (tests/test_uvd_cpu.py, tests/test_gpu_uvd.py): the meshes, the points, an independent float64
reference and the three criteria.

The float32 and the float64 search agree on the winning FACE for only about nine on-surface points in ten — ties between faces that
share an edge or a vertex are the normal case, the points being subdivided mesh vertices — so neither the face nor the UV is compared
for equality. A result is checked for being a valid answer instead, for every point, with no exclusions:

    (a) |d - d64| <= tol_a                                  d64: the float64 minimum distance of `loop_reference`
    (b) |p - sum b_i verts[faces[face]]| <= d64 + tol_b     in float64 from the returned face and bary; b_i >= 0, |sum b - 1| <= 2^-21
    (c) |uv - sum b_i face_uv[face]| <= tol_c               in float64

with tol = 4 x (the same quantity measured for closest_uv_ref in float32 on the same inputs) + 2^-20 x scale, scale being the mesh's
bounding-box diagonal for (a) and (b) and max |face_uv| for (c).

`loop_reference` is not closest_uv_ref: per face, the projection onto the plane if it falls inside the triangle, else the best of the
three clamped segments, in numpy float64, one face at a time."""
import functools
import os

import numpy as np
import torch

HAND_OFFSET = (-0.06, 0.0, 0.02)
N_HAND = 4099


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_mesh(golden_dir):
    """The two-hand UV-topology mesh (V = 1810, F = 3076) from the one-hand fixture: the copy is mirrored in x, its winding reversed,
    it is offset by HAND_OFFSET and uses the UV table's second half. -> (verts float32, faces int64, face_uv float32 (F,3,2))."""
    fx = np.load(os.path.join(golden_dir, "uvd_hand_fixture.npz"), allow_pickle=False)
    v, f, table = fx["verts"], fx["faces"].astype(np.int64), fx["uv_table"]
    assert v.shape == (905, 3) and f.shape == (1538, 3) and table.shape == (1810, 2)
    other = v * np.array([-1.0, 1.0, 1.0], np.float32) + np.array(HAND_OFFSET, np.float32)
    verts = np.concatenate([v, other.astype(np.float32)])
    faces = np.concatenate([f, f[:, ::-1] + 905])
    return torch.tensor(verts), torch.tensor(faces), torch.tensor(table[faces])


def grid_mesh(F, seed=0):
    """The first F faces of a jittered height-field grid (cells of 1 x 1, heights and positions jittered by up to 0.3), with a UV per
    corner that is the corner's grid position scaled into [0, 1] x [0, 0.5]."""
    g = np.random.default_rng(seed)
    nx = max(2, int(np.ceil(np.sqrt(F / 2.0))) + 1)
    ii, jj = np.meshgrid(np.arange(nx), np.arange(nx), indexing="ij")
    xy = np.stack([ii, jj], -1).reshape(-1, 2).astype(np.float64)
    verts = np.concatenate([xy + g.uniform(-0.3, 0.3, xy.shape), g.uniform(-0.3, 0.3, (xy.shape[0], 1))], 1).astype(np.float32)
    faces = []
    for i in range(nx - 1):
        for j in range(nx - 1):
            a, b, c, d = i * nx + j, (i + 1) * nx + j, i * nx + j + 1, (i + 1) * nx + j + 1
            faces += [(a, b, c), (c, b, d)]
    faces = np.array(faces[:F], np.int64)
    assert faces.shape[0] == F
    uv = (xy / (nx - 1) * np.array([1.0, 0.5])).astype(np.float32)
    return torch.tensor(verts), torch.tensor(faces), torch.tensor(uv[faces])


def octahedron():
    """The regular octahedron: 6 vertices on the axes, 8 faces, and corner UVs that differ per face."""
    verts = torch.tensor([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    faces = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    g = torch.Generator().manual_seed(4)
    return verts, faces, torch.rand(8, 3, 2, generator=g) * torch.tensor([1.0, 0.5])


# ---- points -------------------------------------------------------------------------------------------------------------------------
def surface_points(verts, faces, n, seed=1, jitter=0.002):
    """n points on and near the mesh: vertices, edge midpoints, centroids, and the same points jittered by `jitter` of the extent, in
    equal shares drawn with a fixed seed."""
    g = np.random.default_rng(seed)
    v, f = verts.numpy().astype(np.float64), faces.numpy()
    tri = v[f]
    pool = np.concatenate([v, (tri[:, 0] + tri[:, 1]) / 2, (tri[:, 1] + tri[:, 2]) / 2, (tri[:, 2] + tri[:, 0]) / 2, tri.mean(1)])
    extent = float(np.linalg.norm(v.max(0) - v.min(0)))
    pick = pool[g.integers(0, pool.shape[0], n)]
    pick[n // 2:] += g.normal(0.0, jitter * extent, (n - n // 2, 3))
    return torch.tensor(pick.astype(np.float32))


def off_surface_points(verts, faces, n, seed=2, lift=0.2, lift_abs=None):
    """n points at a face's interior (barycentrics at least 0.15) lifted along its normal by `lift` of the face's shortest edge, or by
    the length `lift_abs`. -> (points, the faces they were lifted from, the barycentrics)."""
    g = np.random.default_rng(seed)
    v, f = verts.numpy().astype(np.float64), faces.numpy()
    k = g.integers(0, f.shape[0], n)
    b = g.dirichlet([1.0, 1.0, 1.0], n) * 0.55 + 0.15
    tri = v[f[k]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    edge = np.minimum(np.minimum(np.linalg.norm(tri[:, 1] - tri[:, 0], axis=1), np.linalg.norm(tri[:, 2] - tri[:, 0], axis=1)),
                      np.linalg.norm(tri[:, 2] - tri[:, 1], axis=1))
    p = (b[:, :, None] * tri).sum(1) + nrm * (lift * edge if lift_abs is None else np.full(n, lift_abs))[:, None]
    return torch.tensor(p.astype(np.float32)), k, b


# ---- the independent float64 reference -----------------------------------------------------------------------------------------------
def _segment(p, a, b):
    ab = b - a
    dd = float(ab @ ab)
    t = np.zeros(p.shape[0]) if dd == 0.0 else np.clip((p - a) @ ab / dd, 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)


def loop_reference(points, verts, faces):
    """d64 (N,): the float64 distance of every point to the mesh, one face at a time. A face with an index outside [0, V) or a
    non-finite coordinate is skipped; a point with a non-finite coordinate gets NaN, as does every point of a mesh without a face."""
    p = points.detach().cpu().numpy().astype(np.float64)
    v = verts.detach().cpu().numpy().astype(np.float64)
    best = np.full(p.shape[0], np.inf)
    for face in faces.detach().cpu().numpy():
        if face.min() < 0 or face.max() >= v.shape[0] or not np.isfinite(v[face]).all():
            continue
        a, b, c = v[face]
        d = np.minimum(np.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, c, a))
        n = np.cross(b - a, c - a)
        nn = float(n @ n)
        if nn > 0.0:
            h = (p - a) @ n / nn
            q = p - h[:, None] * n                       # the projection onto the plane; inside when the three sub-areas are >= 0
            inside = (np.cross(b - a, q - a) @ n >= 0) & (np.cross(c - b, q - b) @ n >= 0) & (np.cross(a - c, q - c) @ n >= 0)
            d = np.where(inside, np.abs(h) * np.sqrt(nn), d)
        with np.errstate(invalid="ignore"):
            best = np.where(d < best, d, best)
    best[~np.isfinite(p).all(1) | np.isinf(best)] = np.nan
    return best


# ---- the criteria -------------------------------------------------------------------------------------------------------------------
def scales(verts, faces, face_uv):
    v = verts.detach().cpu().numpy().astype(np.float64)
    f = faces.detach().cpu().numpy()
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    used = v[np.unique(f[ok])]
    used = used[np.isfinite(used).all(1)]
    return float(np.linalg.norm(used.max(0) - used.min(0))), float(np.abs(face_uv.detach().cpu().numpy()[ok]).max())


def measure(points, verts, faces, face_uv, out, d64):
    """The three quantities of (a), (b), (c) for one result `out` = (uv, d, face, bary), as maxima over the points that have a winner
    in the float64 reference, and the smallest barycentric and largest |sum b - 1|. Points without one must report face = -1 and NaNs."""
    uv, d, face, bary = (t.detach().cpu().numpy() for t in out)
    p = points.detach().cpu().numpy().astype(np.float64)
    v, f, t = verts.detach().cpu().numpy().astype(np.float64), faces.detach().cpu().numpy(), face_uv.detach().cpu().numpy().astype(np.float64)
    won = ~np.isnan(d64)
    assert np.array_equal(face >= 0, won), "the points with a winner differ from the float64 reference's"
    assert np.isnan(uv[~won]).all() and np.isnan(d[~won]).all() and np.isnan(bary[~won]).all() and (face[~won] == -1).all()
    if not won.any():
        return dict(a=0.0, b=0.0, c=0.0, bmin=0.0, bsum=0.0)
    face, b = face[won], bary[won].astype(np.float64)
    assert face.max() < f.shape[0] and ((f[face] >= 0) & (f[face] < v.shape[0])).all(), "an invalid face won"
    q = (b[:, :, None] * v[f[face]]).sum(1)
    uv_want = (b[:, :, None] * t[face]).sum(1)
    return dict(a=float(np.abs(d[won].astype(np.float64) - d64[won]).max()),
                b=float(np.maximum(np.linalg.norm(p[won] - q, axis=1) - d64[won], 0.0).max()),
                c=float(np.abs(uv[won].astype(np.float64) - uv_want).max()),
                bmin=float(b.min()), bsum=float(np.abs(b.sum(1) - 1.0).max()))


def check(tag, points, verts, faces, face_uv, out, ref32, d64):
    """Assert (a)-(c) for `out` with the tolerances built from `ref32` (closest_uv_ref in float32 on the same inputs); print the three
    errors and the share of each bound that was used. -> the three shares."""
    diag, uvmax = scales(verts, faces, face_uv)
    got, ref = measure(points, verts, faces, face_uv, out, d64), measure(points, verts, faces, face_uv, ref32, d64)
    tol = dict(a=4 * ref["a"] + 2.0 ** -20 * diag, b=4 * ref["b"] + 2.0 ** -20 * diag, c=4 * ref["c"] + 2.0 ** -20 * uvmax)
    share = {k: got[k] / tol[k] for k in "abc"}
    print(f"uvd {tag}: " + "  ".join(f"({k}) {got[k]:.3g} of {tol[k]:.3g} = {share[k]:.2f} [ref {ref[k]:.3g}]" for k in "abc") +
          f"  bmin {got['bmin']:.3g}  |sum b - 1| {got['bsum']:.3g}")
    assert got["bmin"] >= 0.0 and got["bsum"] <= 2.0 ** -21, (tag, got)
    for k in "abc":
        assert got[k] <= tol[k], (tag, k, got[k], tol[k])
    return share


# ---- the special cases (the host and the device run the same checks) --------------------------------------------------------------------
def special_mesh():
    """Two proper triangles, the first listed twice with other corner UVs (faces 0 and 1), a collinear and a coincident face, a face
    with the index -1 and one with the index V, all over nine vertices of dyadic coordinates."""
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 1], [3, 0, 1], [2, 1, 1],
                          [0, 0, 2], [0.5, 0.5, 2], [1.5, 1.5, 2]])
    faces = torch.tensor([[0, 1, 2], [0, 1, 2], [3, 4, 5], [6, 7, 8], [7, 7, 7], [0, 1, -1], [0, 9, 2]])
    face_uv = torch.rand(7, 3, 2, generator=torch.Generator().manual_seed(1))
    return verts, faces, face_uv


def special_points():
    g = torch.Generator().manual_seed(2)
    near = torch.tensor([[0.25, 0.25, 0.1], [0.25, 0.25, 0.0], [0.0, 0.0, 0.0], [2.5, 0.2, 1.3], [0.25, 0.25, 2.2], [1.0, 1.0, 2.5],
                         [0.5, 0.5, 2.0], [2.0, 2.0, 2.0], [-1.0, -1.0, 3.0]])
    return torch.cat([near, 1.5 * torch.randn(55, 3, generator=g) + torch.tensor([1.0, 0.5, 1.0])])


def check_special_cases(run):
    """`run(points, verts, faces, face_uv) -> (uv, d, face, bary)`: the tie, zero-area, bad-index and NaN cases (shared with the GPU file)."""
    verts, faces, face_uv = special_mesh()
    pts = special_points()
    out = run(pts, verts, faces, face_uv)
    from guassianhand_amd.uvd import closest_uv_ref
    ref32 = closest_uv_ref(pts, verts, faces, face_uv)
    check("special", pts, verts, faces, face_uv, out, ref32, loop_reference(pts, verts, faces))
    uv, d, face, bary = out
    assert bool(torch.isfinite(uv).all()) and bool(torch.isfinite(d).all())
    assert not bool((face == 1).any()) and int((face == 0).sum()) >= 3          # the tie: the lower index wins, with its UVs
    assert not bool((face >= 5).any())                                          # an index -1 and an index V: ignored
    assert int((face == 3).sum()) >= 3 and int((face == 4).sum()) == 0          # the collinear face wins as its edges; the coincident
    assert float(d[6]) == 0.0 and int(face[6]) == 3                              # vertex lies on it and has the higher index
    first = uv[face == 0]
    want = (bary[face == 0, :, None] * face_uv[0]).sum(1)
    assert float((first - want).abs().max()) <= 2.0 ** -22
    assert float((want - (bary[face == 0, :, None] * face_uv[1]).sum(1)).abs().max()) > 0.01
    # a mesh whose only proper face is invalid: the degenerate faces answer; a mesh without a valid face: no winner
    only = run(pts, verts, faces[3:], face_uv[3:])
    assert bool((only[2] >= 0).all()) and bool((only[2] <= 1).all()) and bool(torch.isfinite(only[1]).all())
    none = run(pts, verts, faces[5:], face_uv[5:])
    assert bool((none[2] == -1).all()) and bool(torch.isnan(none[0]).all()) and bool(torch.isnan(none[1]).all()) and bool(torch.isnan(none[3]).all())
    # non-finite points: face = -1 and NaNs for them, nothing changes for the others
    bad = pts.clone()
    bad[3, 1], bad[10, 0], bad[20, 2] = float("nan"), float("inf"), float("-inf")
    b = run(bad, verts, faces, face_uv)
    rows = torch.tensor([3, 10, 20])
    keep = torch.ones(pts.shape[0], dtype=torch.bool)
    keep[rows] = False
    assert b[2][rows].tolist() == [-1, -1, -1] and bool(torch.isnan(b[0][rows]).all()) and bool(torch.isnan(b[1][rows]).all())
    for got, want in zip(b, out):
        assert torch.equal(got[keep], want[keep])
    nan_vert = verts.clone()
    nan_vert[4, 0] = float("nan")                                              # face 2 loses its validity, the others keep theirs
    c = run(pts, nan_vert, faces, face_uv)
    assert not bool((c[2] == 2).any()) and bool(torch.isfinite(c[1]).all())
