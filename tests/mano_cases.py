"""What tests/test_mano_cpu.py and tests/test_gpu_mano.py share: the case generators, a float64 restatement of include/gh_mano.h's
mathematics in per-vertex, per-joint Python loops that shares no code with guassianhand_amd.mano.mano_ref, and the error criterion.

The criterion. The yardstick is mano_ref in float64 on the same inputs. An output of the kernels passes when its largest absolute
error against the yardstick, divided by the yardstick's largest magnitude, is at most MARGIN = 4 times what mano_ref in float32 on
the CPU shows against the same float64 values. The margin is 4 because the kernels sum the blend terms and the joint terms in another
fixed order than torch does; it is not widened per case."""
import math

import numpy as np
import torch

from guassianhand_amd import mano as M

MARGIN = 4.0
GRIDS = {4: (2, 2), 63: (7, 9), 64: (8, 8), 65: (5, 13), 256: (16, 16), 258: (3, 86)}
NAMES = ("global_orient", "hand_pose", "betas", "transl")


def sweep():
    """(V, J, NB, levels, B, H): every V x J pair, the other axes cycling so that each of their values meets each V and each J, then
    the corners the cycle leaves out. NB = 1 is never paired with (B, H) = (1, 1): d_betas would be one number, and the criterion
    cannot judge one number — a correctly rounded float32 result is up to 2^-24 of it away from the yardstick, which is already more
    than 4 times the float32 reference's error whenever that reference lands within an eighth of an ulp, as one draw in four does.
    (The first device run had that pairing at V = 63, J = 2, levels = 3: kernel 3.348e-07, float32 mano_ref 8.680e-09.)"""
    out, i = [], 0
    for V in GRIDS:
        for J in (1, 2, 16):
            bh = ((1, 1), (3, 2))[(i // 2) % 2]
            out.append((V, J, 10 if bh == (1, 1) else (1, 10)[i % 2], (0, 1, 3)[(i + i // 3) % 3], bh))
            i += 1
    out += [(4, 16, 10, 3, (3, 2)), (65, 16, 10, 3, (3, 2)), (256, 16, 10, 3, (3, 2)), (258, 16, 1, 3, (3, 2)), (258, 2, 10, 0, (3, 2)),
            (64, 1, 1, 3, (3, 2)), (63, 16, 1, 1, (3, 2)), (258, 16, 10, 3, (1, 1))]
    return [(V, J, NB, lv, B, H) for V, J, NB, lv, (B, H) in out]


_MODELS = {}


def model(V, J=16, NB=10, levels=3, flip=False, seed=0):
    key = (V, J, NB, levels, flip, seed)
    if key not in _MODELS:
        nx, ny = GRIDS[V] if V in GRIDS else V
        _MODELS[key] = M.synthetic_model(nx, ny, J=J, NB=NB, seed=seed, levels=levels, flip=flip)
    return _MODELS[key]


def models(V, J, NB, levels, H):
    """H models of one call: the second is the mirrored hand (faces turned over, arrays of its own)."""
    return tuple(model(V, J, NB, levels, flip=bool(h % 2), seed=h) for h in range(H))


def params(B, H, J, NB, seed=1, pose_scale=0.6):
    g = torch.Generator().manual_seed(seed)
    return (pose_scale * torch.randn(B, H, 3, generator=g), pose_scale * torch.randn(B, H, 3 * (J - 1), generator=g),
            torch.randn(B, H, NB, generator=g), 0.3 * torch.randn(B, H, 3, generator=g))


def cotangents(ms, B, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, sum(m.n_points for m in ms), 3, generator=g), torch.randn(B, len(ms) * ms[0].J, 3, generator=g)


def reference(ms, ps, cot, dtype):
    """(points, joints, grads of the four inputs) of mano_ref per hand on the CPU in `dtype`; cot = (g_points, g_joints), either None."""
    leaves = [p.detach().to(dtype).clone().requires_grad_(True) for p in ps]
    per = [M.mano_ref(m, *(t[:, h] for t in leaves), acc=dtype) for h, m in enumerate(ms)]
    pts, jts = torch.cat([p for p, _ in per], 1), torch.cat([j for _, j in per], 1)
    loss = 0
    if cot[0] is not None:
        loss = loss + (pts * cot[0].to(dtype)).sum()
    if cot[1] is not None:
        loss = loss + (jts * cot[1].to(dtype)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return pts.detach(), jts.detach(), [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]


def ratio(name, got, ref32, ref64, say=print):
    """The criterion's two figures for one output, printed before anything is asserted: (error of `got`, error of float32 mano_ref),
    both over the yardstick's largest magnitude."""
    if ref64.numel() == 0:
        return 0.0, 0.0
    scale = float(ref64.abs().max())
    err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    base = float((ref32.double() - ref64).abs().max()) / scale
    say(f"    {name:14s} kernel {err:.3e}  float32 mano_ref {base:.3e}  ratio {err / base if base > 0 else float('inf') if err > 0 else 0.0:.2f}")
    return err, base


def inside(name, got, ref32, ref64, say=print):
    err, base = ratio(name, got, ref32, ref64, say)
    assert math.isfinite(err) and err <= MARGIN * base, f"{name}: kernel error {err:.3e} > {MARGIN} x float32 mano_ref's {base:.3e}"
    return err / base if base > 0 else 0.0


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------
def subdivide_loops(vertices, faces):
    """One level by the rule of the module docstring of guassianhand_amd.mano, with a dict of edges and a loop over faces."""
    nv, seen, edges, out = len(vertices), {}, [], []
    for f in faces:
        mids = []
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            key = (min(a, b), max(a, b))
            if key not in seen:
                seen[key] = len(edges)
                edges.append(key)
            mids.append(nv + seen[key])
        a, b, c = f
        ab, bc, ca = mids
        out += [(a, ab, ca), (ab, b, bc), (ca, ab, bc), (ca, bc, c)]
    verts = list(vertices) + [0.5 * (vertices[a] + vertices[b]) for a, b in edges]
    return verts, out, edges


def loops(m, go, hp, be, tr):
    """One parameter set of one model in float64 numpy, 4 x 4 homogeneous transforms, loops over joints and vertices."""
    d = lambda t: np.asarray(t, dtype=np.float64)
    vt, sd, pd, jr, w, pm = d(m.v_template), d(m.shapedirs), d(m.posedirs), d(m.J_regressor), d(m.lbs_weights), d(m.pose_mean)
    go, hp, be, tr = d(go), d(hp), d(be), d(tr)
    pose = np.concatenate([go, hp]) + pm
    V, J = m.V, m.J
    Rs = []
    for j in range(J):
        r = pose[3 * j:3 * j + 3]
        a = math.sqrt(sum((x + 1e-8) ** 2 for x in r))
        x, y, z = r / a
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        Rs.append(np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K))
    v_shaped = np.array([[vt[v, c] + sum(sd[v, c, n] * be[n] for n in range(m.NB)) for c in range(3)] for v in range(V)], dtype=np.float64)
    Jt = np.array([sum(jr[j, v] * v_shaped[v] for v in range(V)) for j in range(J)])
    feat = np.concatenate([(Rs[j] - np.eye(3)).reshape(9) for j in range(1, J)]) if J > 1 else np.zeros(0)
    v_posed = np.array([[v_shaped[v, c] + sum(feat[k] * pd[k, 3 * v + c] for k in range(feat.size)) for c in range(3)] for v in range(V)])
    hom = lambda R, t: np.block([[R, t.reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
    G = []
    for j in range(J):
        p = m.parents[j]
        G.append(hom(Rs[j], Jt[j]) if p < 0 else G[p] @ hom(Rs[j], Jt[j] - Jt[p]))
    A = [G[j] @ hom(np.eye(3), -Jt[j]) for j in range(J)]
    verts = []
    for v in range(V):
        T = sum(w[v, j] * A[j] for j in range(J))
        verts.append((T @ np.append(v_posed[v], 1.0))[:3] + d(tr))
    faces = [tuple(int(i) for i in f) for f in m.faces[0]]
    for _ in range(m.levels):
        verts, faces, _ = subdivide_loops(verts, faces)
    return np.array(verts), np.array([G[j][:3, 3] + d(tr) for j in range(J)])
