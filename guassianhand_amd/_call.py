"""What the Python wrappers of the C-ABI share: the loaded library, the ctypes forms of tensors and streams, the rows-in-place rule,
the host-side argument checks, the padded row count and the device test of the convolution blocks (perceptual.py, lpips.py), the
null-cotangent rule and the one way an entry point is called. _raster_launch.py keeps wrappers of its own (its pointers are plain
integers for struct fields, and its stream and device handling were tuned for the render loop)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from ._abi import status_name
from ._lib import lib  # noqa: F401  (the loaded library with every header's argtypes attached)


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def struct(cls, tensors):
    """A ctypes struct of pointers (GhVertParams, GhVertGrads) from tensors in field order."""
    return cls(*[None if t is None else t.data_ptr() for t in tensors])


def workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


def rows(t: torch.Tensor) -> torch.Tensor:
    """A (P,C) float32 tensor the kernels read in place: unit column stride, any row stride >= C; anything else is copied once."""
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def row_stride(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def check_f32(x: torch.Tensor, named) -> None:
    """Every (name, tensor, rank) of `named` is a float32 tensor of that rank on x's device, or the call is refused on the host."""
    for name, t, nd in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
        if t.dim() != nd:
            raise ValueError(f"{name}: expected {nd} dimensions, got {tuple(t.shape)}")
        if t.device != x.device:
            raise ValueError(f"{name} is on {t.device}, x on {x.device}")


def pad_to(c: int, chunk: int) -> int:
    """c rounded up to a multiple of `chunk`: the rows of a packed convolution weight (GH_CONV_CHUNK, GH_LPIPS_CHUNK)."""
    return -(-c // chunk) * chunk


def on_device(x) -> bool:
    """A float32 (N, H, W, C) tensor on a ROCm device: what the convolution, pooling and LPIPS kernels read."""
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def check_ops(ops: str) -> None:
    if ops not in ("fused", "torch"):
        raise ValueError(f"ops must be 'fused' or 'torch', got {ops!r}")


def cotangent(g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """An incoming gradient as the kernels read it: float32, contiguous; None (no gradient arrived) stays None, the entry points'
    null cotangent."""
    return None if g is None else g.float().contiguous()


def launch(name: str, dev,*args, what: Optional[str] = None, detail: str = "") -> None:
    """Call the entry point `name` with dev's current stream appended, dev being the current device; raise on a non-zero status."""
    with torch.cuda.device(dev):
        rc = getattr(lib(), name)(*args, stream(dev))
    if rc != 0:
        raise RuntimeError(f"{what or name} failed: {status_name(rc)}{detail}")
