"""`backbone_cls: guassianhand_amd.tgs_backbone.Transformer1D` and `backbone_shade_cls: guassianhand_amd.tgs_backbone.Transformer1D` —
the two lines a maintainer changes in config/config_one_shot*.yaml (resolved by tgs.find) to run the backbones' forward in HIP without
editing `_forward`. For the one-shot fit, `backbone_cls: guassianhand_amd.tgs_backbone.Transformer1DGrad` also runs the texture
backbone's backward to its input in HIP.

The classes are built on first access from the reference's own tgs.models.transformers.Transformer1D
(transformer1d.fused_transformer1d_cls): the forward is one gh_xf_forward call where the kernels apply — frozen inference in float32 —
and the base class's forward everywhere else. The one-shot fit trains the identity code through the frozen
texture backbone, so it needs that backbone's gradient with respect to its input: under `Transformer1D` that call runs the
reference's statements, under `Transformer1DGrad` gh_xf_forward_tape and gh_xf_backward. The shade backbone's input depends on no
trainable parameter and keeps `Transformer1D`.

`Transformer1DTrain` is the third class, for training or fine-tuning the backbones themselves (`freeze_backbone_params: false`): where
a parameter requires a gradient the call is gh_xf_forward_tape and gh_xf_backward_params, which returns the gradient of the input and
of every parameter that wants one; with only the input wanting one it is `Transformer1DGrad`'s pair, with nothing wanted the plain
forward. The mode is opt-in. Measured on an MI355X at the shipped sizes (tools/transformer1d_params_time.py), forward + backward over
torch's statements with SDPA under autograd (over the explicit-softmax statements): 1.11 (1.19) at B = 1 and 1.36 (1.14) at B = 8 with
everything trainable, 0.99 (1.13) and 1.23 (1.01) with the last two layers trainable. Of 25.4 ms of device time a step at B = 1 the
parameter-gradient launches are 6.2 ms, the data-gradient launches 12.5 ms, the taped forward 5.9 ms; at B = 1 a layer's parameter
products take longer than its data products (0.47 against 0.25 ms), every output set being split over T ("The
backbones")."""

_cache = {}
_GRAD = {"Transformer1D": "none", "Transformer1DGrad": "input"}
_TRAIN = {"Transformer1DTrain": "params"}


def __getattr__(name):
    if name in _GRAD or name in _TRAIN:
        if name not in _cache:
            from tgs.models.transformers import Transformer1D as base
            from .transformer1d import fused_transformer1d_cls
            _cache[name] = fused_transformer1d_cls(base, grad=_GRAD.get(name) or _TRAIN[name])
        return _cache[name]
    raise AttributeError(name)
