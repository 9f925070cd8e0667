"""guassianhand_amd/tgs_renderer.py: which grafts each opt-in renderer name applies, and in what order. On the CPU, over a stand-in for
the reference's renderer class."""
import importlib
import sys

import pytest

import guassianhand_amd.tgs_renderer as R
from tests import seam_cases as S

# suffix -> the grafts configure() applies after the base's own configure(), in order
TABLE = {
    "FusedHead": ("head",),
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
    "FusedAllFetchAttnBlockUvdTrunk": ("gate", "head", "fetch", "attn", "block", "uvd", "head", "trunk"),
}
FUNCTIONS = {"gate": ("vert_mlp", "fuse_vert_mlps"), "head": ("gs_head", "fuse_gs_head"), "fetch": ("plane", "fuse_plane_fetch"),
             "attn": ("attention", "fuse_self_attn"), "block": ("attn_block", "fuse_attn_block"), "uvd": ("uvd", "fuse_get_uvd"),
             "trunk": ("gs_trunk", "fuse_forward_gs")}
BASES = ("GS3DRenderer", "GS3DRendererEdit")


@pytest.fixture
def no_livehand():
    """The names with the UV search register the livehand shim where livehand is absent: take it out again."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "livehand" or k.startswith("livehand.")}
    yield
    for k in [k for k in sys.modules if k == "livehand" or k.startswith("livehand.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    importlib.invalidate_caches()


def test_the_suffix_table_is_the_one_written_out_here():
    assert R._VARIANTS == TABLE and list(R._VARIANTS) == list(TABLE)
    assert {t: row[:2] for t, row in R._GRAFTS.items()} == FUNCTIONS and all(isinstance(row[2], str) and row[2] for row in R._GRAFTS.values())
    assert tuple(R._BASES) == BASES
    for row in TABLE.values():
        assert "block" not in row or row.index("attn") < row.index("block")
    for name in ("GS3DRendererFusedGateTrunk", "GS3DRendererFusedAttnNothing", "GS3DRendererFusedGateAttnBlock", "GS3DRendererFused",
                 "GS3DRendererEditEditFusedHead", "FusedHead", "GS3DRendererfusedhead"):
        with pytest.raises(AttributeError):
            getattr(R, name)


def test_every_variant_configures_the_base_once_and_then_its_grafts_in_order(monkeypatch):
    """All 30 names over stand-in bases, the seven fuse_* functions replaced by recorders: configure() is the base's, once and with
    the caller's arguments, then exactly the listed grafts on the same object. Building a name caches that name alone, and asks for
    the livehand shim where the UV search is among its grafts."""
    class Edit(S.Renderer):
        """stand-in for the edit renderer"""

    calls = []
    for token, (module, function) in FUNCTIONS.items():
        monkeypatch.setattr(importlib.import_module(f"guassianhand_amd.{module}"), function, lambda r, token=token: calls.append((token, r)) or r)
    monkeypatch.setattr(importlib.import_module("guassianhand_amd.uvd"), "install_livehand_shim", lambda: calls.append(("shim", None)))
    standins = {"GS3DRenderer": S.Renderer, "GS3DRendererEdit": Edit}
    monkeypatch.setattr(R, "_cache", dict(standins))
    seen = set()
    for base, standin in standins.items():
        for suffix, tokens in TABLE.items():
            del calls[:]
            cls = getattr(R, base + suffix)
            assert R._cache.pop(base + suffix) is cls and R._cache == standins          # nothing else was built on the way
            assert calls == ([("shim", None)] if "uvd" in tokens else [])
            assert cls.__mro__[1] is standin and cls.__name__ == standin.__name__ and cls.__module__ == R.__name__ and cls not in seen
            assert cls.__doc__ == f"{standin.__doc__}, and " + ", ".join(R._GRAFTS[t][2] for t in tokens)
            seen.add(cls)
            r = cls()
            del calls[:]
            r.configure(1, two=2)
            assert r.log == [("configure", (1,), {"two": 2})]
            assert [t for t, _ in calls] == list(tokens) and all(obj is r for _, obj in calls)
    assert len(seen) == 30


def test_names_resolve_lazily_and_reach_for_the_reference_alone(monkeypatch, no_livehand):
    import importlib.util
    monkeypatch.setattr(R, "_cache", {})
    have_reference = importlib.util.find_spec("tgs") is not None
    for name in [b + s for b in BASES for s in ("", *TABLE)]:
        if not have_reference:                                     # the name is known: resolving it reaches for the reference's classes
            with pytest.raises(ImportError) as e:
                getattr(R, name)
            assert (e.value.name or "").split(".")[0] == "tgs"      # and for nothing else that is missing
            assert name not in R._cache
            continue
        cls = getattr(R, name)
        assert isinstance(cls, type) and callable(cls.configure)
