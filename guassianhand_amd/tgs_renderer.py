"""`renderer_cls: guassianhand_amd.tgs_renderer.GS3DRenderer` — the one line a maintainer changes in
config/config_one_shot.yaml:175 (the string is resolved by tgs.find, tgs/__init__.py:4-9: import_module + getattr) — and
`renderer_cls: guassianhand_amd.tgs_renderer.GS3DRendererEdit` for the three configs that bind the edit / avatar-drive renderer
(config_one_shot_edit.yaml:179, config_one_shot_avatar_drive.yaml:179, config_one_shot_edit_drive.yaml:180:
tgs.models.renderer_one_shot_edit.GS3DRenderer, whose forward_single_batch takes `render_edit` and per-Gaussian colour weights,
renderer_one_shot_edit.py:440-520).

Either name followed by a suffix of `_VARIANTS` (`GS3DRendererFusedHead`, `GS3DRendererEditFusedHead`, `GS3DRendererFusedGate`,
`GS3DRendererEditFusedGate`, `GS3DRendererFusedAll`, `GS3DRendererEditFusedAll`, ... `GS3DRendererEditFusedAllFetchAttnBlockUvdTrunk`)
is a direct subclass of that class whose `configure()` is the base's and then the listed grafts of `_GRAFTS` on the same object, in
the listed order. All of them are opt-in: the two plain names keep the reference's modules. When each graft's kernels run, and what
it falls back to, is said in its `fuse_*` function's docstring and in INTEGRATION.md. A name with the `uvd` graft registers
`uvd.install_livehand_shim()` before it resolves its base, whose module imports livehand at its top.

The classes are built on first access from the reference's own classes (renderer.fused_renderer_cls / fused_renderer_cls_edit), so
importing this module needs nothing of the reference."""
_cache = {}
_BASES = {"GS3DRenderer": ("tgs.models.renderer_one_shot", "fused_renderer_cls"),            # name -> (the base's module, its graft)
          "GS3DRendererEdit": ("tgs.models.renderer_one_shot_edit", "fused_renderer_cls_edit")}
_GRAFTS = {"gate": ("vert_mlp", "fuse_vert_mlps", "the fused gate and refinement"),           # token -> (module, function, doc phrase)
           "head": ("gs_head", "fuse_gs_head", "the fused Gaussian head"),
           "fetch": ("plane", "fuse_plane_fetch", "the plane fetch"),
           "attn": ("attention", "fuse_self_attn", "the HIP attention core"),
           "block": ("attn_block", "fuse_attn_block", "the fused attention block around it"),
           "uvd": ("uvd", "fuse_get_uvd", "the HIP UV search"),
           "trunk": ("gs_trunk", "fuse_forward_gs", "the fused trunk")}
_VARIANTS = {"FusedHead": ("head",),                                                         # suffix -> what configure() adds, in order
             "FusedGate": ("gate",),
             "FusedAll": ("gate", "head"),
             "FusedFetch": ("fetch",),
             "FusedAllFetch": ("gate", "head", "fetch"),
             "FusedAttn": ("attn",),
             "FusedAllFetchAttn": ("gate", "head", "fetch", "attn"),
             "FusedUvd": ("uvd",),
             "FusedAllFetchAttnUvd": ("gate", "head", "fetch", "attn", "uvd"),
             "FusedAttnBlock": ("attn", "block"),
             "FusedAllFetchAttnBlock": ("gate", "head", "fetch", "attn", "block"),
             "FusedAllFetchAttnBlockUvd": ("gate", "head", "fetch", "attn", "block", "uvd"),
             "FusedTrunk": ("head", "trunk"),
             "FusedAllFetchAttnBlockTrunk": ("gate", "head", "fetch", "attn", "block", "head", "trunk"),
             "FusedAllFetchAttnBlockUvdTrunk": ("gate", "head", "fetch", "attn", "block", "uvd", "head", "trunk")}


def _variant(base, suffix):
    """The subclass of `base` whose configure() adds the grafts of `_VARIANTS[suffix]`: the factory of this module's seam."""
    from importlib import import_module
    from ._seam import graft
    grafts = [_GRAFTS[token] for token in _VARIANTS[suffix]]

    def configure(self, *args, **kwargs):
        base.configure(self, *args, **kwargs)
        for module, function, _ in grafts:
            getattr(import_module(f"{__package__}.{module}"), function)(self)

    return graft((__name__, "_variant"), base, {"configure": configure}, options=(suffix,),
                 doc=f"{base.__doc__}, and {', '.join(phrase for _, _, phrase in grafts)}")


def _build(name):
    from importlib import import_module
    if name in _BASES:
        from . import renderer
        module, graft = _BASES[name]
        return getattr(renderer, graft)(import_module(module).GS3DRenderer)
    for base in _BASES:
        if name[len(base):] in _VARIANTS and name.startswith(base):
            if "uvd" in _VARIANTS[name[len(base):]]:
                import_module(f"{__package__}.uvd").install_livehand_shim()        # the base's module imports livehand.input_encoder at its top
            return _variant(__getattr__(base), name[len(base):])
    raise AttributeError(name)


def __getattr__(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]
