"""`renderer_cls: guassianhand_amd.tgs_renderer.GS3DRenderer` — the one line a maintainer changes in
config/config_one_shot.yaml:175 (the string is resolved by tgs.find, tgs/__init__.py:4-9: import_module + getattr) — and
`renderer_cls: guassianhand_amd.tgs_renderer.GS3DRendererEdit` for the three configs that bind the edit / avatar-drive renderer
(config_one_shot_edit.yaml:179, config_one_shot_avatar_drive.yaml:179, config_one_shot_edit_drive.yaml:180:
tgs.models.renderer_one_shot_edit.GS3DRenderer, whose forward_single_batch takes `render_edit` and per-Gaussian colour weights,
renderer_one_shot_edit.py:440-520).

`GS3DRendererFusedHead` / `GS3DRendererEditFusedHead` are the same two classes whose `configure()` additionally calls
`gs_head.fuse_gs_head(self)`: `forward_gs` then ends in the fused Gaussian head (include/gh_head.h) instead of GSLayer's five
nn.Linear calls and their elementwise launches. Opt-in: the two names above keep the reference's GSLayer.

`GS3DRendererFusedGate` / `GS3DRendererEditFusedGate`: `configure()` additionally calls `vert_mlp.fuse_vert_mlps(self)` — the
validity gate (`gs_valid`) and the position refinement (`vert_pos_refinement`) then run the fused vertex MLP block
(include/gh_vert.h) while their dropout is inactive (eval mode); in train mode they keep the reference's torch forward.
`GS3DRendererFusedAll` / `GS3DRendererEditFusedAll`: gate, refinement and head. All opt-in.

`GS3DRendererFusedFetch` / `GS3DRendererEditFusedFetch`: `configure()` additionally calls `plane.fuse_plane_fetch(self)` — `forward`'s
`query_triplane_texture` (the texture code sampled at every point's UV) then runs the plane fetch (include/gh_plane.h), whose
gradient of the code is summed in a fixed order. `GS3DRendererFusedAllFetch` / `GS3DRendererEditFusedAllFetch`: gate, refinement,
head and fetch. Opt-in as well: every name above keeps its behaviour.

`GS3DRendererFusedAttn` / `GS3DRendererEditFusedAttn`: `configure()` additionally calls `attention.fuse_self_attn(self)` — the
attention core of `self_attn_layer`, which `forward` applies to the points `mink_idxs_inter` flags, then runs the streaming-softmax
kernels (include/gh_attn.h) while its dropout is inactive (eval mode); in train mode it keeps the reference's torch statements.
`GS3DRendererFusedAllFetchAttn` / `GS3DRendererEditFusedAllFetchAttn`: gate, refinement, head, fetch and attention. Opt-in too.

`GS3DRendererFusedUvd` / `GS3DRendererEditFusedUvd`: `configure()` additionally calls `uvd.fuse_get_uvd(self)` — `forward_single_batch`'s
`get_uvd` (every Gaussian's closest point on the UV-topology hand mesh, whose UV drives the `color_b` / `opacity_b` lookups) then runs
the HIP UV search (include/gh_uvd.h) instead of livehand's. `GS3DRendererFusedAllFetchAttnUvd` / `GS3DRendererEditFusedAllFetchAttnUvd`:
gate, refinement, head, fetch, attention and UV search. Opt-in too. The reference's modules import livehand at their top, which
`uvd.install_livehand_shim()` serves where livehand is absent: resolving one of these four names calls it first.

`GS3DRendererFusedAttnBlock` / `GS3DRendererEditFusedAttnBlock`: `GS3DRendererFusedAttn` whose `configure()` additionally calls
`attn_block.fuse_attn_block(self)` — the whole `forward` of `self_attn_layer` (both LayerNorms, the projections, `fc`, the feed-forward
block and the residuals, include/gh_attn_rows.h, around the attention core) is then three launches while its dropout is inactive and
autograd asks none of its parameters for a gradient; otherwise it is what `GS3DRendererFusedAttn` does.
`GS3DRendererFusedAllFetchAttnBlock` / `GS3DRendererEditFusedAllFetchAttnBlock` add the same to `...FusedAllFetchAttn`, and
`GS3DRendererFusedAllFetchAttnBlockUvd` / `GS3DRendererEditFusedAllFetchAttnBlockUvd` the UV search to that. Opt-in too.

`GS3DRendererFusedTrunk` / `GS3DRendererEditFusedTrunk`: `configure()` additionally calls `gs_head.fuse_gs_head(self)` and
`gs_trunk.fuse_forward_gs(self)` — `forward_gs`, the trunk MLP `mlp_net` and the Gaussian head behind it, is then one HIP pass each way
(include/gh_trunk.h) while the trunk has two hidden layers with SiLU or ReLU, the tensors are float32 on the device and autograd asks
no parameter of `mlp_net` or `gs_net` for a gradient; otherwise it is `mlp_net` in torch and then the fused head.
`GS3DRendererFusedAllFetchAttnBlockTrunk` / `GS3DRendererEditFusedAllFetchAttnBlockTrunk` and `...FusedAllFetchAttnBlockUvdTrunk` add
the same to the classes of those names without `Trunk`. Opt-in too.

The classes are built on first access from the reference's own classes (renderer.fused_renderer_cls / fused_renderer_cls_edit), so
importing this module needs nothing of the reference."""
_cache = {}
_BASES = {"GS3DRenderer": ("tgs.models.renderer_one_shot", "fused_renderer_cls"),            # name -> (the base's module, its graft)
          "GS3DRendererEdit": ("tgs.models.renderer_one_shot_edit", "fused_renderer_cls_edit")}
_SUFFIXES = {"FusedHead": (False, True, False, False, "the fused Gaussian head"),              # suffix -> (gate, head, fetch, attn, doc)
             "FusedGate": (True, False, False, False, "the fused gate and refinement"),
             "FusedAll": (True, True, False, False, "the fused gate and refinement and Gaussian head"),
             "FusedFetch": (False, False, True, False, "the plane fetch"),
             "FusedAllFetch": (True, True, True, False, "the fused gate and refinement, Gaussian head and plane fetch"),
             "FusedAttn": (False, False, False, True, "the HIP attention core"),
             "FusedAllFetchAttn": (True, True, True, True, "the fused gate and refinement, Gaussian head, plane fetch and HIP attention core")}
_UVD = {"FusedUvd": "", "FusedAllFetchAttnUvd": "FusedAllFetchAttn"}          # suffix -> the suffix of the class the UV search is added to
# suffix -> (the suffix of the class it is added to, whether it adds the UV search; otherwise the attention block's graft)
_BLOCK = {"FusedAttnBlock": ("FusedAttn", False), "FusedAllFetchAttnBlock": ("FusedAllFetchAttn", False),
          "FusedAllFetchAttnBlockUvd": ("FusedAllFetchAttnBlock", True)}
# suffix -> the suffix of the class the fused trunk (with the fused head behind it) is added to
_TRUNK = {"FusedTrunk": "", "FusedAllFetchAttnBlockTrunk": "FusedAllFetchAttnBlock", "FusedAllFetchAttnBlockUvdTrunk": "FusedAllFetchAttnBlockUvd"}


def _build(name):
    if name in _BASES:
        from importlib import import_module
        from . import renderer
        module, graft = _BASES[name]
        return getattr(renderer, graft)(import_module(module).GS3DRenderer)
    for suffix, (gate, head, fetch, attn, doc) in _SUFFIXES.items():
        if name.endswith(suffix) and name[:-len(suffix)] in _BASES:
            base = __getattr__(name[:-len(suffix)])
            from .attention import fuse_self_attn
            from .gs_head import fuse_gs_head
            from .plane import fuse_plane_fetch
            from .vert_mlp import fuse_vert_mlps

            def configure(self, *args, **kwargs):
                base.configure(self, *args, **kwargs)
                if gate:
                    fuse_vert_mlps(self)
                if head:
                    fuse_gs_head(self)
                if fetch:
                    fuse_plane_fetch(self)
                if attn:
                    fuse_self_attn(self)

            return type(base.__name__, (base,), {"configure": configure, "__module__": __name__, "__doc__": f"{base.__doc__}, and {doc}"})
    for suffix, inner in _UVD.items():
        if name.endswith(suffix) and name[:-len(suffix)] in _BASES:
            from .uvd import fuse_get_uvd, install_livehand_shim
            install_livehand_shim()                            # the base's module imports livehand.input_encoder at its top
            base = __getattr__(name[:-len(suffix)] + inner)

            def configure(self, *args, **kwargs):
                base.configure(self, *args, **kwargs)
                fuse_get_uvd(self)

            return type(base.__name__, (base,), {"configure": configure, "__module__": __name__, "__doc__": f"{base.__doc__}, and the HIP UV search"})
    for suffix, (inner, uvd) in _BLOCK.items():
        if name.endswith(suffix) and name[:-len(suffix)] in _BASES:
            if uvd:
                from .uvd import install_livehand_shim
                install_livehand_shim()
            base = __getattr__(name[:-len(suffix)] + inner)

            def configure(self, *args, **kwargs):
                base.configure(self, *args, **kwargs)
                if uvd:
                    from .uvd import fuse_get_uvd
                    fuse_get_uvd(self)
                else:
                    from .attn_block import fuse_attn_block
                    fuse_attn_block(self)

            doc = "the HIP UV search" if uvd else "the fused attention block around it"
            return type(base.__name__, (base,), {"configure": configure, "__module__": __name__, "__doc__": f"{base.__doc__}, and {doc}"})
    for suffix, inner in _TRUNK.items():
        if name.endswith(suffix) and name[:-len(suffix)] in _BASES:
            base = __getattr__(name[:-len(suffix)] + inner)

            def configure(self, *args, **kwargs):
                base.configure(self, *args, **kwargs)
                from .gs_head import fuse_gs_head
                from .gs_trunk import fuse_forward_gs
                fuse_gs_head(self)
                fuse_forward_gs(self)

            return type(base.__name__, (base,), {"configure": configure, "__module__": __name__, "__doc__": f"{base.__doc__}, and the fused trunk"})
    raise AttributeError(name)


def __getattr__(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]
