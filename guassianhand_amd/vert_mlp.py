"""The validity gate and the position refinement: the reference's vert_valid and vert_pos_refinement (tgs/models/verts_refinement.py:35-83)
— cat(features, position), LayerNorm(eps=1e-6), fc1 + ReLU, fc2, fc and a sigmoid (K = 1) or `position.detach() + tanh(.) * radius`
(K = 3) — as one HIP pass forward and one backward, through include/gh_vert.h.

    vert_block(x, pts, params, act="sigmoid" | "tanh_offset", radius=0.001, eps=1e-6)  -> (P, K)

`params` are the block's eight tensors in `PARAMS` order: LayerNorm weight and bias (D = Cf + 3), fc1 (Hd, D) with Hd = D // 4, fc2
(Hd, Hd), fc (K, Hd), each followed by its bias. The call is differentiable in x, pts and the parameters. The backward recomputes the
row's forward from x and pts — nothing else is saved; when no parameter needs a gradient it is one launch that writes grad_x and
grad_pts, otherwise the parameter gradients are summed from per-workgroup partials in a fixed order by a second launch. x is read in
place through its row stride; the concatenation is never written. No atomics; a row's output and its grad_x are bitwise the same
alone or among 100,000 rows, and parameter gradients are bitwise reproducible run to run.

CPU tensors, and `ops="torch"` on any device, go through `_vert_block_ref`: F.layer_norm and F.linear over torch.cat, in float64 on
request (the yardstick of the tests). ROCm tensors go through the HIP kernels only.

`VertValid` / `VertPosRefinement` are the modules themselves with the reference's state-dict keys (`ff.layer_norm.*`, `ff.fc1.*`,
`ff.fc2.*`, `fc.*`) and initialisation (Xavier-uniform weights, zero biases), so a reference checkpoint loads unchanged;
`fused_vert_cls(base)` grafts the fused forward onto the reference's own classes, and `fuse_vert_mlps(renderer)` swaps the classes of
`renderer.gs_valid` and `renderer.vert_pos_refinement` for them (parameters untouched) — what the config strings
`guassianhand_amd.tgs_renderer.GS3DRendererFusedGate` / `...FusedAll` (and their `Edit` forms) do in `configure()`.

Dropout. The block holds two nn.Dropout(0.1) layers. The fused forward is taken only when `not self.training` or their p is 0;
otherwise a grafted module calls the reference's own forward unchanged (and VertValid / VertPosRefinement run the same layers in plain
torch): a module in train mode — under Lightning's fit loop, say — keeps the torch path, dropout included."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _abi, _seam
from ._call import check_f32, check_ops, cotangent, launch, lib, ptr, row_stride, rows, struct, workspace
from ._mlp_block import _MLPBlock, block_params, dropout_live, init_linears

PARAMS = _abi.VERT_PARAMS                                        # the order of `params` (GhVertParams)
ACTS = {"sigmoid": _abi.GH_VERT_ACT_SIGMOID, "tanh_offset": _abi.GH_VERT_ACT_TANH_OFFSET}
MAX_CF = _abi.GH_VERT_MAX_CF


def param_shapes(Cf: int, K: int):
    D = int(Cf) + 3
    Hd = D // 4
    return ((D,), (D,), (Hd, D), (Hd,), (Hd, Hd), (Hd,), (int(K), Hd), (int(K),))


def _check(x, pts, params, act, eps) -> int:
    """Everything that can be refused on the host is, before any device work. Returns K."""
    if act not in ACTS:
        raise ValueError(f"act must be one of {tuple(ACTS)}, got {act!r}")
    params = tuple(params)
    if len(params) != len(PARAMS):
        raise ValueError(f"params: expected the {len(PARAMS)} tensors {PARAMS}, got {len(params)}")
    check_f32(x, (("x", x, 2), ("pts", pts, 2)) + tuple((n, p, 2 if n.endswith("weight") and not n.startswith("ln") else 1)
                                                        for n, p in zip(PARAMS, params)))
    Cf = x.shape[1]
    if not 1 <= Cf <= MAX_CF:
        raise ValueError(f"x has {Cf} columns: the block takes 1 to {MAX_CF} features")
    if pts.shape[0] != x.shape[0] or pts.shape[1] != 3:
        raise ValueError(f"pts: expected ({x.shape[0]}, 3) for x {tuple(x.shape)}, got {tuple(pts.shape)}")
    K = params[6].shape[0]
    if K not in (1, 3):
        raise ValueError(f"fc_weight has {K} rows: K must be 1 or 3")
    if act == "tanh_offset" and K != 3:
        raise ValueError(f"act='tanh_offset' adds the position: K must be 3, got {K}")
    for name, p, shape in zip(PARAMS, params, param_shapes(Cf, K)):
        if tuple(p.shape) != shape:
            raise ValueError(f"{name}: expected {shape} for Cf = {Cf} (D = Cf + 3, Hd = D // 4), K = {K}, got {tuple(p.shape)}")
    if not float(eps) >= 0:
        raise ValueError(f"eps must be >= 0, got {eps}")
    return K


# ---- plain-torch restatement (CPU path; the yardstick of the device path) --------------------------------------------------------
def _vert_block_ref(x, pts, params, *, act="sigmoid", radius=0.001, eps=1e-6, acc: Optional[torch.dtype] = None) -> torch.Tensor:
    """The block in plain torch, differentiable, statement for statement the reference's forward in eval mode. acc=torch.float64
    computes (and returns) in double."""
    if acc is not None:
        x, pts = x.to(acc), pts.to(acc)
        params = [p.to(acc) for p in params]
    g, b, w1, b1, w2, b2, w3, b3 = params
    z = torch.cat([x, pts], dim=-1)
    z = F.layer_norm(z, (z.shape[-1],), g, b, eps)
    z = F.linear(F.relu(F.linear(z, w1, b1)), w2, b2)
    o = F.linear(z, w3, b3)
    if act == "sigmoid":
        return torch.sigmoid(o)
    return pts.detach() + torch.tanh(o) * radius


# ---- device path ---------------------------------------------------------------------------------------------------------------
class _VertBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pts, cfg, *params):
        act, radius, eps = cfg
        ctx.set_materialize_grads(False)
        x, pts = rows(x.detach()), pts.detach().contiguous()
        params = [p.detach().contiguous() for p in params]
        P, Cf = x.shape
        K, dev = params[6].shape[0], x.device
        out = torch.empty(P, K, dtype=torch.float32, device=dev)
        if P > 0:
            desc = _abi.GhVertDesc(K, ACTS[act], float(radius), float(eps))
            pstruct = struct(_abi.GhVertParams, params)
            launch("gh_vert_forward", dev, ptr(x), row_stride(x), ptr(pts), P, Cf, C.byref(pstruct), C.byref(desc), ptr(out),
                   what=f"gh_vert_forward (P={P}, Cf={Cf}, K={K})")
        ctx.cfg = cfg
        ctx.save_for_backward(x, pts, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, pts, *params = ctx.saved_tensors
        act, radius, eps = ctx.cfg
        P, Cf = x.shape
        K, dev = params[6].shape[0], x.device
        D, Hd = Cf + 3, (Cf + 3) // 4
        need_pts, need_w = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:])
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        gx = new(P, Cf)
        gpts = new(P, 3) if need_pts else None
        gparams = [new(*p.shape) for p in params] if need_w else None
        if P == 0:
            if need_w:
                for g in gparams:
                    g.zero_()
        else:
            g = cotangent(g_out)
            nbytes = int(lib().gh_vert_workspace_bytes(P, D, Hd, K)) if need_w else 0
            ws = workspace(nbytes, dev) if need_w else None
            desc = _abi.GhVertDesc(K, ACTS[act], float(radius), float(eps))
            pstruct = struct(_abi.GhVertParams, params)
            gstruct = struct(_abi.GhVertGrads, gparams) if need_w else None
            launch("gh_vert_backward", dev, ptr(x), row_stride(x), ptr(pts), P, Cf, C.byref(pstruct), C.byref(desc), ptr(g), ptr(gx), Cf,
                   ptr(gpts), C.byref(gstruct) if need_w else None, ptr(ws), nbytes, what=f"gh_vert_backward (P={P}, Cf={Cf}, K={K})")
        gp = [g if need else None for g, need in zip(gparams, ctx.needs_input_grad[3:])] if need_w else [None] * len(params)
        return (gx if ctx.needs_input_grad[0] else None, gpts, None, *gp)


def vert_block(x: torch.Tensor, pts: torch.Tensor, params: Sequence[torch.Tensor], *, act: str = "sigmoid", radius: float = 0.001,
               eps: float = 1e-6, ops: str = "fused") -> torch.Tensor:
    """x (P,Cf), pts (P,3), params in PARAMS order, all float32 -> (P,K): sigmoid(mlp(cat(x, pts))) for act="sigmoid", or
    pts.detach() + tanh(mlp(cat(x, pts))) * radius for act="tanh_offset" (K = 3). ops="torch" runs the plain-torch restatement on x's
    device instead of the kernels; CPU tensors always take it."""
    check_ops(ops)
    _check(x, pts, params, act, eps)
    if ops == "torch" or not x.is_cuda:
        return _vert_block_ref(x, pts, list(params), act=act, radius=float(radius), eps=float(eps))
    return _VertBlockFn.apply(x, pts, (act, float(radius), float(eps)), *params)


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _module_params(self):
    return block_params(self.ff) + [self.fc.weight, self.fc.bias]


def vert_module_forward(self, verts_f: torch.Tensor, verts_position: torch.Tensor, act: str, ops: Optional[str] = None) -> torch.Tensor:
    """vert_valid.forward / vert_pos_refinement.forward (verts_refinement.py:46-59, :72-83) with dropout inactive, as one vert_block
    call. Reads self.ff.{layer_norm, fc1, fc2}, self.fc, self.verts_f_dim, self.detach and, for the refinement, self.radius."""
    assert verts_f.shape[-1] == self.verts_f_dim
    x, pts = verts_f, verts_position
    if getattr(self, "detach", False):
        x, pts = x.detach(), pts.detach()
    lead = x.shape[:-1]
    out = vert_block(x.reshape(-1, x.shape[-1]), pts.reshape(-1, 3), _module_params(self), act=act,
                     radius=float(getattr(self, "radius", 0.0)), eps=float(self.ff.layer_norm.eps), ops=ops or getattr(self, "vert_ops", "fused"))
    return out.reshape(*lead, out.shape[-1])


class _VertModule(nn.Module):
    ACT, K = "sigmoid", 1

    def __init__(self, verts_f_dim: int, if_detach: bool = False, ops: str = "fused"):
        super().__init__()
        self.verts_f_dim = int(verts_f_dim)
        self.detach = bool(if_detach)
        self.vert_ops = ops
        D = self.verts_f_dim + 3
        self.ff = _MLPBlock(D, D // 4)
        self.fc = nn.Linear(D // 4, self.K)
        init_linears(self)

    def _torch_forward(self, verts_f, verts_position):
        """The reference's forward, layer by layer (dropout included): the train-mode path."""
        assert verts_f.shape[-1] == self.verts_f_dim
        x, pts = (verts_f.detach(), verts_position.detach()) if self.detach else (verts_f, verts_position)
        o = self.fc(self.ff(torch.cat([x, pts], dim=-1)))
        if self.ACT == "sigmoid":
            return torch.sigmoid(o)
        return verts_position.detach() + torch.tanh(o) * self.radius

    def forward(self, verts_f, verts_position):
        if dropout_live(self, self.ff):
            return self._torch_forward(verts_f, verts_position)
        return vert_module_forward(self, verts_f, verts_position, self.ACT)


class VertValid(_VertModule):
    """The reference's vert_valid with its state-dict keys (ff.layer_norm.*, ff.fc1.*, ff.fc2.*, fc.*) and initialisation
    (Xavier-uniform weights, zero biases; LayerNorm's ones and zeros). `if_detach=True` detaches both inputs; the reference's print
    is not reproduced. In train mode with dropout p > 0 the layers run in plain torch, dropout included."""
    ACT, K = "sigmoid", 1


class VertPosRefinement(_VertModule):
    """The reference's vert_pos_refinement, as VertValid is vert_valid: position.detach() + tanh(mlp) * radius."""
    ACT, K = "tanh_offset", 3

    def __init__(self, verts_f_dim: int, radius: float = 0.001, if_detach: bool = False, ops: str = "fused"):
        super().__init__(verts_f_dim, if_detach=if_detach, ops=ops)
        self.radius = radius


_SEAM = (__name__, "fused_vert_cls")


def fused_vert_cls(base):
    """A subclass of the given class (the reference's own tgs.models.verts_refinement.vert_valid or vert_pos_refinement) whose forward
    is vert_module_forward while dropout is inactive, and the base class's own forward, unchanged, in train mode with dropout p > 0.
    The activation follows the head: an `fc` with one output is the gate, with three the refinement."""
    def forward(self, verts_f, verts_position):
        if dropout_live(self, self.ff):
            return base.forward(self, verts_f, verts_position)
        return vert_module_forward(self, verts_f, verts_position, "sigmoid" if self.fc.out_features == 1 else "tanh_offset")

    return _seam.graft(_SEAM, base, {"forward": forward}, "fused MLP block")


def fuse_vert_mlps(renderer):
    """Swap the classes of `renderer.gs_valid` and `renderer.vert_pos_refinement` for fused_vert_cls of their own classes:
    forward_single_batch's gate and refinement then run one HIP pass each. The module objects, their parameters and their state dicts
    are untouched. Returns the renderer."""
    for name in ("gs_valid", "vert_pos_refinement"):
        m = getattr(renderer, name)
        if not isinstance(m, _VertModule):
            _seam.swap(_SEAM, m)
    return renderer
