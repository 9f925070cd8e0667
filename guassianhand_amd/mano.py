"""The hand points: MANO-style linear blend skinning and the dataset's edge subdivision on the device (include/gh_mano.h), in place of
the reference's per-frame CPU work (dataset_one_shot.py:299-325: an smplx MANO layer per hand, mis_utils.edge_subdivide three times,
98,562 x 3 floats copied to the device), with a gradient back to the pose inputs.

    HandModel(v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose_mean, faces, levels=3)
    HandModel.from_layer(layer, levels=3)                  the same-named attributes of an smplx MANO layer, duck-typed
    synthetic_model(nx, ny, J=16, NB=10, seed=0, levels=3, flip=False)   a grid-mesh disc with random, well-conditioned arrays
    mano_ref(model, global_orient, hand_pose, betas, transl, acc=None)   -> (points (B, P, 3), joints (B, J, 3)), plain torch
    pose_hands(models, global_orient, hand_pose, betas, transl, *, ops="fused") -> HandPoints(points, joints)
    subdivide_faces(faces, n_vertices)                     one level: (edges (E, 2), faces (4 F, 3)), vectorised
    point_count(V, F, levels, E=None)                      the closed-form vertex count after `levels` subdivisions

The model (V vertices, F faces, J joints, NB shape coefficients): v_template (V, 3), shapedirs (V, 3, NB), posedirs (9 (J - 1), 3 V)
with column 3 v + c, J_regressor (J, V), parents (J) with parents[0] = -1 and parents[i] < i, lbs_weights (V, J), pose_mean (3 J),
faces (F, 3). The mathematics is smplx's lbs with use_pca=False, stated in include/gh_mano.h; `pose_mean` is added to
cat(global_orient, hand_pose), so a zero pose of a non-flat hand mean is still a curled hand.

Subdivision. One level keeps the old vertices, in order, and appends the midpoint of every undirected edge in order of first
appearance walking the faces in order, inside a face (v0, v1), (v1, v2), (v2, v0); face i = (a, b, c) becomes (a, ab, ca), (ab, b, bc),
(ca, ab, bc), (ca, bc, c) at 4 i .. 4 i + 3. That is the result of the reference's mis_utils.edge_subdivide, so the points come in
the reference's order. The topology is constant per model: HandModel builds every level's `edges` and `faces` once, and folds the
levels into one stencil, point = sum of at most three vertices with weights in multiples of 1 / 2^levels (`stencil_idx`, `stencil_w`),
plus that stencil's transpose as a CSR over vertices for the backward. A mirrored hand has the other winding, hence another edge
order: every model owns its tables.

pose_hands takes H models and (B, H, .) parameters and returns points (B, sum_h P_h, 3), hand h's block behind hand h - 1's (the
reference concatenates right, then left: dataset_one_shot.py:371), and joints (B, H J, 3). The first V points of a hand's block are
its skinned vertices. It is an autograd.Function over gh_mano_forward / gh_mano_backward, differentiable in the four parameter
tensors; the model is frozen. The fused path is taken for float32 ROCm tensors with ops="fused"; CPU tensors, other dtypes and
ops="torch" run mano_ref per hand on the tensors' own device. B = 0 launches nothing."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _abi
from ._call import check_ops, cotangent, launch, ptr, workspace

MAX_LEVELS = _abi.GH_MANO_MAX_LEVELS
MANO_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)


class HandPoints(NamedTuple):
    points: torch.Tensor
    joints: torch.Tensor


# ---- topology, on the host, once per model ------------------------------------------------------------------------------------------------
def subdivide_faces(faces: np.ndarray, n_vertices: int) -> Tuple[np.ndarray, np.ndarray]:
    """One level of midpoint subdivision of `faces` (F, 3) over n_vertices vertices: (edges (E, 2) with the smaller index first, in
    order of first appearance; faces (4 F, 3), midpoint e being vertex n_vertices + e). No loop over faces or edges."""
    f = np.asarray(faces, dtype=np.int64)
    half = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2)          # (3 F, 2): face-major, then (01, 12, 20)
    lo, hi = half.min(1), half.max(1)
    key = lo * np.int64(n_vertices) + hi
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                                                  # unique keys by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    edges = np.stack([uniq[order] // n_vertices, uniq[order] % n_vertices], axis=1)
    mid = (n_vertices + rank[inverse.reshape(-1)]).reshape(-1, 3)                               # per face: ab, bc, ca
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    new = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, ab, bc], 1), np.stack([ca, bc, c], 1)], axis=1)
    return edges, new.reshape(-1, 3)


def point_count(V: int, F: int, levels: int, E: Optional[int] = None) -> int:
    """Vertices after `levels` subdivisions of a mesh with V vertices, F faces and E edges (default: a disc, E = V + F - 1, which MANO's
    open-wrist mesh is): a level gives V + E vertices, 2 E + 3 F edges and 4 F faces."""
    E = V + F - 1 if E is None else E
    for _ in range(levels):
        V, E, F = V + E, 2 * E + 3 * F, 4 * F
    return V


def _fold(idx: np.ndarray, w: np.ndarray, edges: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The stencil rows of the midpoints of `edges` over points whose own rows are (idx, w): halves of both rows, equal vertices
    merged, at most three left."""
    i6 = np.concatenate([idx[edges[:, 0]], idx[edges[:, 1]]], axis=1)
    w6 = 0.5 * np.concatenate([w[edges[:, 0]], w[edges[:, 1]]], axis=1)
    for j in range(1, 6):                                                                     # 15 column pairs, not rows
        for i in range(j):
            same = (i6[:, j] == i6[:, i]) & (w6[:, j] != 0) & (w6[:, i] != 0)
            w6[:, i] = np.where(same, w6[:, i] + w6[:, j], w6[:, i])
            w6[:, j] = np.where(same, 0.0, w6[:, j])
    keep = np.argsort(w6 == 0, axis=1, kind="stable")                                        # non-zero weights first, order kept
    i6, w6 = np.take_along_axis(i6, keep, 1), np.take_along_axis(w6, keep, 1)
    if w6.shape[0] and np.abs(w6[:, 3:]).max() != 0:
        raise ValueError("a subdivided point depends on more than three vertices: more levels than the stencil holds")
    i3, w3 = i6[:, :3].copy(), w6[:, :3].copy()
    i3[w3 == 0] = np.broadcast_to(i3[:, :1], i3.shape)[w3 == 0]                               # an unused slot names a valid vertex
    return i3, w3


class HandModel:
    """One frozen hand model with its subdivision tables (module docstring). Arrays are kept as float32 CPU tensors under the
    constructor's names; `edges[l]` / `faces[l + 1]` are level l + 1's tables (faces[0] the model's own), `stencil_idx` / `stencil_w`
    (P, 3) the folded levels, `tr_ptr` / `tr_point` / `tr_w` their transpose. Device copies in the kernels' layouts are made once per
    device."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose_mean, faces, levels: int = 3):
        f32 = lambda t: torch.as_tensor(np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float32)).contiguous()
        self.v_template, self.shapedirs, self.posedirs = f32(v_template), f32(shapedirs), f32(posedirs)
        self.J_regressor, self.lbs_weights, self.pose_mean = f32(J_regressor), f32(lbs_weights), f32(pose_mean).reshape(-1)
        parents = np.asarray(parents.detach().cpu() if isinstance(parents, torch.Tensor) else parents).astype(np.int64).reshape(-1)
        faces = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).astype(np.int64)
        if self.v_template.dim() != 2 or self.v_template.shape[1] != 3 or self.v_template.shape[0] < 1:
            raise ValueError(f"v_template: expected (V, 3) with V >= 1, got {tuple(self.v_template.shape)}")
        V = self.V = int(self.v_template.shape[0])
        if self.shapedirs.dim() != 3 or tuple(self.shapedirs.shape[:2]) != (V, 3) or self.shapedirs.shape[2] < 1:
            raise ValueError(f"shapedirs: expected ({V}, 3, NB) with NB >= 1, got {tuple(self.shapedirs.shape)}")
        self.NB = int(self.shapedirs.shape[2])
        J = self.J = int(parents.size)
        if J < 1 or J > _abi.GH_MANO_MAX_J or self.NB > _abi.GH_MANO_MAX_NB or V > _abi.GH_MANO_MAX_V:
            raise ValueError(f"J = {J}, NB = {self.NB}, V = {V}: the kernels hold 1 <= J <= {_abi.GH_MANO_MAX_J}, NB <= {_abi.GH_MANO_MAX_NB}, "
                             f"V <= {_abi.GH_MANO_MAX_V}")
        if parents[0] != -1 or any(not 0 <= int(parents[i]) < i for i in range(1, J)):
            raise ValueError(f"parents: expected parents[0] = -1 and 0 <= parents[i] < i, got {parents.tolist()}")
        for name, t, shape in (("posedirs", self.posedirs, (9 * (J - 1), 3 * V)), ("J_regressor", self.J_regressor, (J, V)),
                               ("lbs_weights", self.lbs_weights, (V, J)), ("pose_mean", self.pose_mean, (3 * J,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
        if faces.ndim != 2 or faces.shape[1] != 3 or (faces.size and (faces.min() < 0 or faces.max() >= V)):
            raise ValueError(f"faces: expected (F, 3) indices into {V} vertices")
        if not 0 <= int(levels) <= MAX_LEVELS:
            raise ValueError(f"levels: expected 0 .. {MAX_LEVELS}, got {levels}")
        self.parents, self.levels = tuple(int(p) for p in parents), int(levels)
        self.faces, self.edges = [faces], []
        idx = np.repeat(np.arange(V, dtype=np.int64)[:, None], 3, 1)
        w = np.zeros((V, 3))
        w[:, 0] = 1.0
        n = V
        for _ in range(self.levels):
            e, f = subdivide_faces(self.faces[-1], n)
            i3, w3 = _fold(idx, w, e)
            idx, w = np.concatenate([idx, i3]), np.concatenate([w, w3])
            self.edges.append(e)
            self.faces.append(f)
            n += e.shape[0]
        self.n_points = n
        if n > _abi.GH_MANO_MAX_P:
            raise ValueError(f"{n} points: the kernels hold {_abi.GH_MANO_MAX_P}")
        self.stencil_idx, self.stencil_w = torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(w.astype(np.float32))
        # the transpose: entries (vertex, point, weight) of the non-zero weights, sorted by vertex and inside a vertex by point
        pt = np.repeat(np.arange(n, dtype=np.int64), 3)
        vi, ww = idx.reshape(-1), w.reshape(-1)
        nz = ww != 0
        pt, vi, ww = pt[nz], vi[nz], ww[nz]
        order = np.lexsort((pt, vi))
        self.tr_point, self.tr_w = torch.from_numpy(pt[order].astype(np.int32)), torch.from_numpy(ww[order].astype(np.float32))
        self.tr_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(vi, minlength=V))]).astype(np.int32))
        self._device = {}

    @classmethod
    def from_layer(cls, layer, levels: int = 3) -> "HandModel":
        """From an object with an smplx MANO layer's attributes: v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights,
        pose_mean and faces (or faces_tensor)."""
        faces = getattr(layer, "faces_tensor", None)
        faces = getattr(layer, "faces") if faces is None else faces
        return cls(layer.v_template, layer.shapedirs, layer.posedirs, layer.J_regressor, layer.parents, layer.lbs_weights, layer.pose_mean,
                   np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).astype(np.int64), levels=levels)

    @property
    def faces_subdivided(self) -> torch.Tensor:
        """(4^levels F, 3) int64: the faces over the n_points points."""
        return torch.from_numpy(self.faces[-1].copy())

    def stencil_points(self, vertices: torch.Tensor) -> torch.Tensor:
        """(..., V, 3) -> (..., P, 3) through the folded stencil (what the kernel's third stage computes)."""
        idx, w = self.stencil_idx.to(vertices.device).long(), self.stencil_w.to(vertices)
        return (vertices[..., idx, :] * w[..., None]).sum(-2)

    def on(self, dev: torch.device):
        """(GhManoModel, the tensors it points to) on `dev`, in the header's layouts; made once per device."""
        dev = torch.device(dev)
        hit = self._device.get(dev)
        if hit is None:
            V, J, NB = self.V, self.J, self.NB
            t = dict(v_template=self.v_template.t(), shapedirs=self.shapedirs.permute(2, 1, 0),
                     posedirs=self.posedirs.reshape(9 * (J - 1), V, 3).permute(0, 2, 1), lbs_weights=self.lbs_weights.t(),
                     j_template=self.J_regressor.double() @ self.v_template.double(),          # float64: the header's two double arrays
                     j_shapedirs=torch.einsum("jv,vcn->jcn", self.J_regressor.double(), self.shapedirs.double()), pose_mean=self.pose_mean,
                     st_idx=self.stencil_idx, st_w=self.stencil_w, tr_ptr=self.tr_ptr, tr_point=self.tr_point, tr_w=self.tr_w)
            t = {k: v.contiguous().to(dev) for k, v in t.items()}
            m = _abi.GhManoModel()
            m.V, m.P, m.levels, m.nnz = V, self.n_points, self.levels, int(self.tr_point.numel())
            for i in range(_abi.GH_MANO_MAX_J):
                m.parents[i] = self.parents[i] if i < J else -1
            for name in _abi.MANO_MODEL_ARRAYS:
                setattr(m, name, t[name].data_ptr() if t[name].numel() else None)
            hit = self._device[dev] = (m, t)
        return hit


def synthetic_model(nx: int, ny: int, J: int = 16, NB: int = 10, seed: int = 0, levels: int = 3, flip: bool = False) -> HandModel:
    """An nx x ny grid mesh (a disc, as the hand's open wrist leaves MANO's) with random, well-conditioned arrays: lbs_weights and
    J_regressor rows sum to 1, blend shapes are small against the mesh, `parents` is MANO's at J = 16 and a random tree otherwise.
    `flip` turns every face over (the mirrored hand's winding)."""
    g = torch.Generator().manual_seed(seed)
    V = nx * ny
    ii, jj = torch.meshgrid(torch.arange(nx), torch.arange(ny), indexing="ij")
    vt = torch.stack([ii.reshape(-1) / max(nx - 1, 1) - 0.5, jj.reshape(-1) / max(ny - 1, 1) - 0.5, torch.zeros(V)], 1).float() * 0.2
    vt = vt + 0.01 * torch.randn(V, 3, generator=g)
    q = (ii[:-1, :-1] * ny + jj[:-1, :-1]).reshape(-1)
    faces = torch.cat([torch.stack([q, q + ny, q + 1], 1), torch.stack([q + 1, q + ny, q + ny + 1], 1)]).numpy()
    if flip:
        faces = faces[:, [0, 2, 1]]
    parents = list(MANO_PARENTS) if J == 16 else [-1] + [int(torch.randint(0, i, (1,), generator=g)) for i in range(1, J)]
    lbs = torch.rand(V, J, generator=g) ** 4 + 1e-3
    jr = torch.rand(J, V, generator=g)
    return HandModel(vt, 0.01 * torch.randn(V, 3, NB, generator=g), 0.005 * torch.randn(9 * (J - 1), 3 * V, generator=g),
                     jr / jr.sum(1, keepdim=True), parents, lbs / lbs.sum(1, keepdim=True), 0.3 * torch.randn(3 * J, generator=g), faces,
                     levels=levels)


# ---- plain torch (CPU path, fallback, yardstick) --------------------------------------------------------------------------------------------
def _rodrigues(r: torch.Tensor) -> torch.Tensor:
    """smplx's batch_rodrigues on (N, 3): the 1e-8 goes on every component before the norm, the direction divides the raw vector."""
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    d = r / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    z = torch.zeros_like(rx)
    K = torch.cat([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).view(-1, 3, 3)
    return torch.eye(3, dtype=r.dtype, device=r.device)[None] + sin * K + (1 - cos) * torch.bmm(K, K)


def mano_ref(model: HandModel, global_orient: torch.Tensor, hand_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor,
             acc: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The module's mathematics in plain torch ops for one model, subdivision level by level: global_orient (B, 3), hand_pose
    (B, 3 (J - 1)), betas (B, NB), transl (B, 3) -> points (B, P, 3), joints (B, J, 3). In `acc` when given; differentiable."""
    dt = acc or global_orient.dtype
    dev = global_orient.device
    go, hp, be, tr = (t.to(dt) for t in (global_orient, hand_pose, betas, transl))
    m = lambda t: t.to(device=dev, dtype=dt)
    B, J, V = go.shape[0], model.J, model.V
    pose = torch.cat([go, hp], 1) + m(model.pose_mean)
    R = _rodrigues(pose.reshape(-1, 3)).view(B, J, 3, 3)
    v_shaped = m(model.v_template)[None] + torch.einsum("vcn,bn->bvc", m(model.shapedirs), be)
    Jt = torch.einsum("jv,bvc->bjc", m(model.J_regressor), v_shaped)
    feat = (R[:, 1:] - torch.eye(3, dtype=dt, device=dev)).reshape(B, 9 * (J - 1))
    v_posed = v_shaped + (feat @ m(model.posedirs)).view(B, V, 3)
    GR, Gt = [R[:, 0]], [Jt[:, 0]]
    for j in range(1, J):
        p = model.parents[j]
        GR.append(GR[p] @ R[:, j])
        Gt.append((GR[p] @ (Jt[:, j] - Jt[:, p])[..., None])[..., 0] + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                                            # (B, J, 3, 3), (B, J, 3)
    At = Gt - (GR @ Jt[..., None])[..., 0]
    w = m(model.lbs_weights)
    TR, Tt = torch.einsum("vj,bjrc->bvrc", w, GR), torch.einsum("vj,bjr->bvr", w, At)
    pts = (TR @ v_posed[..., None])[..., 0] + Tt + tr[:, None]
    for e in model.edges:
        e = torch.from_numpy(e).to(dev)
        pts = torch.cat([pts, 0.5 * (pts[:, e[:, 0]] + pts[:, e[:, 1]])], 1)
    return pts, Gt + tr[:, None]


# ---- device path -----------------------------------------------------------------------------------------------------------------------
def _structs(models, dev, B: int):
    J, NB = models[0].J, models[0].NB
    dims = _abi.GhManoDims(B, len(models), J, NB)
    arr = (_abi.GhManoModel * len(models))(*[m.on(dev)[0] for m in models])
    return dims, arr


class _PoseHandsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, global_orient, hand_pose, betas, transl, models):
        dev = global_orient.device
        B, H = global_orient.shape[:2]
        go, hp, be, tr = (t.detach().contiguous() for t in (global_orient, hand_pose, betas, transl))
        dims, arr = _structs(models, dev, B)
        points = torch.empty(B, sum(m.n_points for m in models), 3, dtype=torch.float32, device=dev)
        joints = torch.empty(B, H * models[0].J, 3, dtype=torch.float32, device=dev)
        ctx.set_materialize_grads(False)
        ctx.models, ctx.shapes = models, (tuple(hand_pose.shape), dev)
        if B == 0:
            ctx.ws = None
            return points, joints
        nbytes = int(_call_lib().gh_mano_workspace_bytes(C.byref(dims), arr))
        ws = workspace(nbytes, dev)
        params = _abi.GhManoParams(go.data_ptr(), hp.data_ptr() if hp.numel() else None, be.data_ptr(), tr.data_ptr())
        launch("gh_mano_forward", dev, C.byref(dims), arr, C.byref(params), ptr(points), ptr(joints), ptr(ws), nbytes,
               what=f"gh_mano_forward (B={B}, H={H}, J={dims.J}, NB={dims.NB})")
        ctx.ws = ws
        return points, joints

    @staticmethod
    @once_differentiable
    def backward(ctx, g_points, g_joints):
        models, (hp_shape, dev) = ctx.models, ctx.shapes
        B, H, J, NB = hp_shape[0], len(models), models[0].J, models[0].NB
        need = ctx.needs_input_grad[:4]
        shapes = ((B, H, 3), hp_shape, (B, H, NB), (B, H, 3))
        if B == 0 or (g_points is None and g_joints is None):
            return tuple(torch.zeros(s, dtype=torch.float32, device=dev) if n else None for s, n in zip(shapes, need)) + (None,)
        outs = [torch.empty(s, dtype=torch.float32, device=dev) if n else None for s, n in zip(shapes, need)]
        if outs[1] is not None and J == 1:
            outs[1].zero_()
        gp, gj = cotangent(g_points), cotangent(g_joints)
        dims, arr = _structs(models, dev, B)
        grads = _abi.GhManoGrads(*[None if o is None or o.numel() == 0 else o.data_ptr() for o in outs])
        launch("gh_mano_backward", dev, C.byref(dims), arr, ptr(gp), ptr(gj), C.byref(grads), ptr(ctx.ws), int(ctx.ws.numel()),
               what=f"gh_mano_backward (B={B}, H={H}, J={J}, NB={NB})")
        return (*outs, None)


def _call_lib():
    from ._call import lib
    return lib()


def _check(models, global_orient, hand_pose, betas, transl):
    if isinstance(models, HandModel):
        models = (models,)
    models = tuple(models)
    if not 1 <= len(models) or any(not isinstance(m, HandModel) for m in models):
        raise TypeError("models: expected one HandModel or a sequence of them")
    H, J, NB = len(models), models[0].J, models[0].NB
    if any(m.J != J or m.NB != NB for m in models):
        raise ValueError("models: every model of one call has the same J and NB")
    for name, t, last in (("global_orient", global_orient, 3), ("hand_pose", hand_pose, 3 * (J - 1)), ("betas", betas, NB), ("transl", transl, 3)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dim() != 3 or t.shape[1] != H or t.shape[2] != last or t.shape[0] != global_orient.shape[0]:
            raise ValueError(f"{name}: expected (B, {H}, {last}), got {tuple(t.shape)}")
        if t.device != global_orient.device:
            raise ValueError(f"{name} is on {t.device}, global_orient on {global_orient.device}")
    return models


def pose_hands(models: Sequence[HandModel], global_orient: torch.Tensor, hand_pose: torch.Tensor, betas: torch.Tensor,
               transl: torch.Tensor, *, ops: str = "fused") -> HandPoints:
    """H models and (B, H, .) parameters -> HandPoints(points (B, sum_h P_h, 3), joints (B, H J, 3)) (module docstring)."""
    check_ops(ops)
    models = _check(models, global_orient, hand_pose, betas, transl)
    params = (global_orient, hand_pose, betas, transl)
    if ops == "fused" and all(t.is_cuda and t.dtype == torch.float32 for t in params):
        if len(models) > _abi.GH_MANO_MAX_H or global_orient.shape[0] > _abi.GH_MANO_MAX_B:
            raise ValueError(f"pose_hands: the kernels hold {_abi.GH_MANO_MAX_H} models and {_abi.GH_MANO_MAX_B} parameter sets per call")
        return HandPoints(*_PoseHandsFn.apply(*params, models))
    per = [mano_ref(m, *(t[:, h] for t in params)) for h, m in enumerate(models)]
    return HandPoints(torch.cat([p for p, _ in per], 1), torch.cat([j for _, j in per], 1))
