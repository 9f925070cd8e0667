"""`backbone_cls: guassianhand_amd.tgs_backbone.Transformer1D` and `backbone_shade_cls: guassianhand_amd.tgs_backbone.Transformer1D` —
the two lines a maintainer changes in config/config_one_shot*.yaml (resolved by tgs.find) to run the backbones' forward in HIP without
editing `_forward`. For the one-shot fit, `backbone_cls: guassianhand_amd.tgs_backbone.Transformer1DGrad` also runs the texture
backbone's backward to its input in HIP.

The classes are built on first access from the reference's own tgs.models.transformers.Transformer1D
(transformer1d.fused_transformer1d_cls): the forward is one gh_xf_forward call where the kernels apply — frozen inference in float32 —
and the base class's forward everywhere else. The one-shot fit trains the identity code through the frozen
texture backbone, so it needs that backbone's gradient with respect to its input: under `Transformer1D` that call runs the
reference's statements, under `Transformer1DGrad` gh_xf_forward_tape and gh_xf_backward. The shade backbone's input depends on no
trainable parameter and keeps `Transformer1D`."""

_cache = {}
_GRAD = {"Transformer1D": "none", "Transformer1DGrad": "input"}


def __getattr__(name):
    if name in _GRAD:
        if name not in _cache:
            from tgs.models.transformers import Transformer1D as base
            from .transformer1d import fused_transformer1d_cls
            _cache[name] = fused_transformer1d_cls(base, grad=_GRAD[name])
        return _cache[name]
    raise AttributeError(name)
