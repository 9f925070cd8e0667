"""The class graft (guassianhand_amd/_seam.py) through every factory that uses it, on the CPU: one cached class per (base, options),
an idempotent swap, and pickle / copy.deepcopy that give an instance of the identical class, alone, stacked and in a fresh process."""
import copy
import json
import os
import pickle
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import _seam, attention, attn_block, gs_head, gs_trunk, pool, renderer, scene_code, tgs_pointnet, transformer1d, vert_mlp
from tests import seam_cases as S
from tests import transformer1d_cases as K
from tests.scene_code_cases import PlainUpsample
from tests.self_attn_cases import PlainSelfAttn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _on(attr, fuse):
    """fuse_*(renderer) of a seam that grafts `renderer.<attr>`, as a function of the module."""
    return lambda m: getattr(fuse(SimpleNamespace(**{attr: m})), attr)


def _folded(base):
    return tgs_pointnet._folded(pool.fused_pointnet_cls(base))


# id -> (the factory as f(base), a new ungrafted module, the swap as f(module) or None where the seam has no fuse_* function)
CASES = {
    "self_attn": (attention.fused_self_attn_cls, PlainSelfAttn, _on("self_attn_layer", attention.fuse_self_attn)),
    "attn_block": (attn_block.fused_attn_block_cls, PlainSelfAttn, _on("self_attn_layer", attn_block.fuse_attn_block)),
    "vert": (vert_mlp.fused_vert_cls, S.Plain, _on("gs_valid", lambda r: vert_mlp.fuse_vert_mlps(SimpleNamespace(vert_pos_refinement=S.Plain(), **vars(r))))),
    "gs_layer": (gs_head.fused_gs_layer_cls, S.Plain, _on("gs_net", gs_head.fuse_gs_head)),
    "forward_gs": (gs_trunk.fused_forward_gs_cls, S.Plain, gs_trunk.fuse_forward_gs),
    "upsample": (scene_code.fused_upsample_cls, lambda: PlainUpsample(4, 3, 1), None),
    "transformer1d": (transformer1d.fused_transformer1d_cls, lambda: K.make_module(32, 1, 32, 1), transformer1d.fuse_transformer1d),
    "transformer1d_input": (lambda b: transformer1d.fused_transformer1d_cls(b, "input"), lambda: K.make_module(32, 1, 32, 1),
                            lambda m: transformer1d.fuse_transformer1d(m, grad="input")),
    "transformer1d_params": (lambda b: transformer1d.fused_transformer1d_cls(b, grad="params"), lambda: K.make_module(32, 1, 32, 1),
                             lambda m: transformer1d.fuse_transformer1d(m, "params")),
    "pointnet": (pool.fused_pointnet_cls, S.Plain, None),                  # the three that cached nothing
    "renderer": (renderer.fused_renderer_cls, S.Plain, None),
    "renderer_edit": (renderer.fused_renderer_cls_edit, S.Plain, None),
    "pointnet_folded": (_folded, S.Plain, None),
}


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr() for k in sa)


def _round_trips(m):
    for back in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert type(back) is type(m) and back is not m and _same_state(back, m)


@pytest.mark.parametrize("case", list(CASES))
def test_one_cached_class_an_idempotent_swap_and_round_trips(case):
    factory, new, fuse = CASES[case]
    m = new()
    base = type(m)
    cls = factory(base)
    assert cls is factory(base) and cls is not base and issubclass(cls, base) and cls.__mro__[1] is (base if case != "pointnet_folded" else cls._gh_base)
    assert cls.__name__ == ("LocalPoolPointnetFolded" if case == "pointnet_folded" else base.__name__)
    assert cls.__module__.startswith("guassianhand_amd.") and cls.__module__ == cls._gh_seam[0] and callable(getattr(sys.modules[cls.__module__], cls._gh_seam[1]))
    assert _seam.is_grafted(cls._gh_seam, cls) and not _seam.is_grafted(cls._gh_seam, base)
    assert not _seam.is_grafted(cls._gh_seam, type("Sub", (cls,), {}))             # an exact-type test, not issubclass
    if case != "pointnet_folded":
        assert cls._gh_base is base and cls.__doc__.startswith(f"{base.__module__}.{base.__name__} with the MI355X ")
    if fuse is None:
        m.__class__ = cls
    else:
        before = {k: v.data_ptr() for k, v in m.state_dict().items()}
        assert fuse(m) is m and type(m) is cls and fuse(m) is m and type(m) is cls          # the swap, and again
        assert {k: v.data_ptr() for k, v in m.state_dict().items()} == before
    _round_trips(m)


def test_per_seam_registries_let_grafts_stack():
    r = SimpleNamespace(self_attn_layer=PlainSelfAttn())
    attention.fuse_self_attn(r)
    core = type(r.self_attn_layer)
    assert core is attention.fused_self_attn_cls(PlainSelfAttn)
    attn_block.fuse_attn_block(r)                                                  # the core's class is not "already fused" to the block's seam
    both = type(r.self_attn_layer)
    assert both is attn_block.fused_attn_block_cls(core) and both.__mro__[1] is core and both is not attn_block.fused_attn_block_cls(PlainSelfAttn)
    attn_block.fuse_attn_block(r)
    assert type(r.self_attn_layer) is both
    _round_trips(r.self_attn_layer)


def test_the_fused_trunk_over_a_renderer_variant_round_trips(monkeypatch):
    import guassianhand_amd.tgs_renderer as R
    monkeypatch.setattr(R, "_cache", {"GS3DRenderer": S.Renderer})                 # (nothing built on the stand-in stays cached)
    variant = R.GS3DRendererFusedTrunk
    assert variant.__mro__[1] is S.Renderer and variant._gh_options == ("FusedTrunk",)
    r = gs_trunk.fuse_forward_gs(variant(seed=2))
    assert type(r) is gs_trunk.fused_forward_gs_cls(variant) and type(r).forward_gs is gs_trunk.forward_gs_fused
    _round_trips(r)
    _round_trips(variant(seed=3))


def test_swapping_to_other_options_goes_back_to_the_recorded_base():
    m = transformer1d.fuse_transformer1d(K.make_module(32, 1, 32, 1), grad="input")
    cls = type(transformer1d.fuse_transformer1d(m, grad="params"))
    assert cls is transformer1d.fused_transformer1d_cls(K.StandIn, "params") and cls._gh_base is K.StandIn and cls._gh_grad == "params"


CHILD = """
import pickle, sys
import tests.seam_cases
assert not [m for m in sys.modules if m.startswith("guassianhand_amd")]
with open(sys.argv[1], "rb") as f:
    block, trunk = pickle.load(f)
chain = lambda c: [[c.__module__, c.__name__, *getattr(c, "_gh_seam", ())]] + (chain(c._gh_base) if hasattr(c, "_gh_base") else [])
import json
print(json.dumps({"block": chain(type(block)), "trunk": chain(type(trunk)), "scale": [float(block.scale[0]), float(trunk.scale[0])],
                  "weight": block.fc.weight.tolist()}))
"""


def test_a_stacked_graft_loads_in_a_fresh_process(tmp_path, monkeypatch):
    """The pickle names no made class: a process that has imported the stand-in's module and nothing of this package rebuilds the chain."""
    import guassianhand_amd.tgs_renderer as R
    block = S.Plain(seed=4)
    block.__class__ = attn_block.fused_attn_block_cls(attention.fused_self_attn_cls(S.Plain))
    monkeypatch.setattr(R, "_cache", {"GS3DRenderer": S.Renderer})
    trunk = gs_trunk.fuse_forward_gs(R.GS3DRendererFusedAllFetchAttnBlockTrunk(seed=5))
    path = tmp_path / "stacked.pkl"
    path.write_bytes(pickle.dumps((block, trunk)))
    assert b"fused_attn_block_cls" in path.read_bytes() and b"_rebuild" in path.read_bytes()
    done = subprocess.run([sys.executable, "-c", CHILD, str(path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    got = json.loads(done.stdout.strip().splitlines()[-1])
    plain, rend = ["tests.seam_cases", "Plain"], ["tests.seam_cases", "Renderer"]
    assert got["block"] == [["guassianhand_amd.attn_block", "Plain", "guassianhand_amd.attn_block", "fused_attn_block_cls"],
                            ["guassianhand_amd.attention", "Plain", "guassianhand_amd.attention", "fused_self_attn_cls"], plain]
    assert got["trunk"] == [["guassianhand_amd.gs_trunk", "Renderer", "guassianhand_amd.gs_trunk", "fused_forward_gs_cls"],
                            ["guassianhand_amd.tgs_renderer", "Renderer", "guassianhand_amd.tgs_renderer", "_variant"], rend]
    assert got["scale"] == [5.0, 6.0] and got["weight"] == block.fc.weight.tolist()
