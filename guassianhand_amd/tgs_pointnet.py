"""`pointcloud_encoder_texture_cls: guassianhand_amd.tgs_pointnet.LocalPoolPointnet` and the same for
`pointcloud_encoder_shade_cls` — the two lines a maintainer changes in config/config_one_shot*.yaml:157,166 (resolved by tgs.find).

The class is built on first access from the reference's own LocalPoolPointnet (pool.fused_pointnet_cls). That module imports
`scatter_mean, scatter_max` from torch_scatter at its top; where no torch_scatter is installed, a module of that name holding
pool.scatter_mean / pool.scatter_max is registered first, so the import succeeds without editing the reference.

`LocalPoolPointnetFolded` is the same construction with block_ops = "folded": the ResNet blocks run with the pooled half folded per
cell (guassianhand_amd.res_block)."""
import importlib
import sys
import types

_cache = {}


def _ensure_torch_scatter():
    try:
        importlib.import_module("torch_scatter")
    except ImportError:
        from . import pool
        shim = types.ModuleType("torch_scatter")
        shim.scatter_max, shim.scatter_mean = pool.scatter_max, pool.scatter_mean
        shim.__doc__ = "guassianhand_amd.pool's scatter_max / scatter_mean under torch_scatter's name"
        sys.modules["torch_scatter"] = shim


def _folded(base):
    from ._seam import graft
    cls = graft((__name__, "_folded"), base, {"block_ops": "folded"}, doc=f"{base.__name__} with the ResNet blocks folded per cell")
    cls.__name__ = cls.__qualname__ = "LocalPoolPointnetFolded"                   # the one made class with a name of its own
    return cls


def __getattr__(name):
    if name == "LocalPoolPointnet":
        if name not in _cache:
            _ensure_torch_scatter()
            from tgs.models.pointclouds.pointnet_texture import LocalPoolPointnet as base
            from .pool import fused_pointnet_cls
            _cache[name] = fused_pointnet_cls(base)
        return _cache[name]
    if name == "LocalPoolPointnetFolded":
        if name not in _cache:
            _cache[name] = _folded(__getattr__("LocalPoolPointnet"))
        return _cache[name]
    raise AttributeError(name)
