"""`backbone_cls: guassianhand_amd.tgs_backbone.Transformer1D` and `backbone_shade_cls: guassianhand_amd.tgs_backbone.Transformer1D` —
the two lines a maintainer changes in config/config_one_shot*.yaml (resolved by tgs.find) to run the backbones' forward in HIP without
editing `_forward`.

The class is built on first access from the reference's own tgs.models.transformers.Transformer1D
(transformer1d.fused_transformer1d_cls): its forward is one gh_xf_forward call where the kernels apply — frozen inference in float32 —
and the base class's forward everywhere else. The one-shot fit, which needs the texture backbone's backward,
is such a case: it runs the reference's statements."""

_cache = {}


def __getattr__(name):
    if name == "Transformer1D":
        if name not in _cache:
            from tgs.models.transformers import Transformer1D as base
            from .transformer1d import fused_transformer1d_cls
            _cache[name] = fused_transformer1d_cls(base)
        return _cache[name]
    raise AttributeError(name)
