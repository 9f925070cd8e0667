"""`post_processor_texture_cls: guassianhand_amd.tgs_scene.TriplaneUpsampleNetwork` — the line a maintainer changes in
config/config_one_shot*.yaml (resolved by tgs.find) to run the texture planes' upsample in HIP without editing `_forward`.

The class is built on first access from the reference's own tgs.models.networks_texture.TriplaneUpsampleNetwork
(scene_code.fused_upsample_cls): its forward takes the kernel's per-plane form where the kernels apply and the base class's forward
everywhere else. The `cat`s and the `map_bias` add behind it stay torch; the one-statement edit of `_forward`
(scene_code.scene_code) fuses those too."""

_cache = {}


def __getattr__(name):
    if name == "TriplaneUpsampleNetwork":
        if name not in _cache:
            from tgs.models.networks_texture import TriplaneUpsampleNetwork as base
            from .scene_code import fused_upsample_cls
            _cache[name] = fused_upsample_cls(base)
        return _cache[name]
    raise AttributeError(name)
