"""The attention block on the host (guassianhand_amd/attn_block.py): its plain-torch restatement against attention.SelfAttn, bitwise;
refine_flagged against the reference's loop restated from renderer_one_shot.py:554-574, bitwise; the graft's fall-back rules; the
C-ABI's symbols, struct sizes and host-side argument checks; the opt-in renderer names. No GPU compute is launched here."""
import ctypes as C
import importlib.util
import re
import sys
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import attention as A
from guassianhand_amd import attn_block as AB
from tests.attn_block_cases import grad_run, make_input, make_module, reference_loop_parts, spy_on_launches
from tests.helpers import header_symbols
from tests.self_attn_cases import KEYS, PlainSelfAttn, load_fixture


def test_keys_are_the_state_dict_order():
    m = make_module()
    assert AB.KEYS == KEYS == tuple(m.state_dict().keys())
    assert all(a is b for a, b in zip(AB.module_params(m), m.state_dict(keep_vars=True).values()))
    assert _abi.GhAttnRowsParams._fields_[0][0] == "wq_weight" and len(_abi.ATTN_ROWS_PARAMS) == 16


@pytest.mark.parametrize("BS,V", [(1, 48), (2, 33), (1, 1)])
def test_attn_block_ref_is_the_module_bitwise(BS, V):
    m = make_module(frozen=False)
    x, cot = make_input(BS, V)
    y, g = grad_run(m, x, cot)
    for params in (AB.module_params(m), m.state_dict()):              # a sequence in state-dict order, or a mapping with the keys
        y2, g2 = grad_run(lambda t: AB.attn_block_ref(t, params), x, cot)
        assert torch.equal(y2, y) and torch.equal(g2, g)
    y3, g3 = grad_run(lambda t: AB.attn_block(t, AB.module_params(m)), x, cot)      # CPU tensors take the restatement
    assert torch.equal(y3, y) and torch.equal(g3, g)
    y64 = AB.attn_block_ref(x, AB.module_params(m), acc=torch.float64)
    assert y64.dtype == torch.float64 and float((y64.detach() - y.double()).abs().max()) < 1e-4
    # the restatement differentiates with respect to the parameters as well
    grads = torch.autograd.grad((AB.attn_block_ref(x, AB.module_params(m)) * cot).sum(), list(m.parameters()))
    want = torch.autograd.grad((m(x) * cot).sum(), list(m.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(grads, want))


def test_attn_block_ref_with_a_row_list_and_an_output_tensor():
    m = make_module()
    P = AB.module_params(m)
    x, cot = make_input(2, 20)
    idx = torch.tensor([3, 17, 0, 9], dtype=torch.int32)
    got, g = grad_run(lambda t: AB.attn_block(t, P, idx=idx), x, cot)
    want = x.clone()
    asc = torch.sort(idx.long())[0]                                    # the list is a set: the rows attend in ascending order
    want[:, asc] = m(x[:, asc])
    assert torch.equal(got, want)
    assert torch.equal(AB.attn_block(x, P, idx=asc.to(torch.int32)), got) and torch.equal(AB.attn_block(x, P, idx=idx.flip(0)), got)
    rest = torch.ones(20, dtype=torch.bool)
    rest[idx.long()] = False
    assert torch.equal(g[:, rest], cot[:, rest])                       # a row that is not listed passes its cotangent through
    out = torch.full_like(x, 5.0)
    assert AB.attn_block(x, P, idx=idx, out=out) is out and torch.equal(out[:, idx.long()], want[:, idx.long()]) and bool((out[:, rest] == 5).all())
    with pytest.raises(ValueError, match="out"):
        AB.attn_block(x, P, out=out[:, :3])
    with pytest.raises(ValueError, match="ops"):
        AB.attn_block(x, P, ops="eager")
    with pytest.raises(ValueError, match="expected the 16 tensors"):
        AB.attn_block(x, P[:5])


def _flags(B, N, share, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, generator=g) < share


def _loop_cases():
    f_tail = _flags(2, 1003, 0.3, 1)
    f_tail[:, 1000:] = True                                            # three flagged tail rows: beyond 8 * 125, never refined
    f_single = _flags(2, 1000, 0.3, 2)
    f_one_b = _flags(2, 1003, 0.3, 3)
    f_one_b[1] = False                                                 # a batch element without a flag
    f_range = _flags(2, 1003, 0.3, 4)
    f_range[0, 250:375] = False                                        # a range without a flag
    return {"tail": (1003, 1000, f_tail), "single-range": (1000, 30000, f_single), "empty-element": (1003, 1000, f_one_b),
            "empty-range": (1003, 1000, f_range), "no-flag": (1003, 1000, torch.zeros(2, 1003, dtype=torch.bool))}


@pytest.mark.parametrize("name", ["tail", "single-range", "empty-element", "empty-range", "no-flag"])
def test_refine_flagged_is_the_reference_loop_bitwise(name):
    N, part_rows, flags = _loop_cases()[name]
    m = make_module(seed=1)
    feat, cot = make_input(2, N, seed=3)
    want, gwant = grad_run(lambda t: reference_loop_parts(t, flags, m, part_rows), feat, cot)
    got, ggot = grad_run(lambda t: AB.refine_flagged(t, flags, m, part_rows=part_rows), feat, cot)
    assert got.data_ptr() != feat.data_ptr() and torch.equal(got, want) and torch.equal(ggot, gwant)
    got3, _ = grad_run(lambda t: AB.refine_flagged(t, flags.unsqueeze(-1), m, part_rows=part_rows, ops="torch"), feat, cot)
    assert torch.equal(got3, want)
    if name == "tail":
        assert int(N / 8) == 125 and bool(flags[:, 1000:].all()) and torch.equal(got[:, 1000:], feat[:, 1000:])
        assert not torch.equal(got[:, :1000][flags[:, :1000]], feat[:, :1000][flags[:, :1000]])
    if name == "no-flag":
        assert torch.equal(got, feat) and torch.equal(ggot, cot)
    assert torch.equal(got[~flags], feat[~flags]) and torch.equal(ggot[~flags], cot[~flags])


def _grafted(f_dim=131, over_fused_core=False):
    base = PlainSelfAttn(f_dim)
    r = SimpleNamespace(self_attn_layer=base)
    if over_fused_core:
        A.fuse_self_attn(r)
    before = type(base)
    assert AB.fuse_attn_block(r) is r and r.self_attn_layer is base
    AB.fuse_attn_block(r)                                              # idempotent
    assert type(base) is AB.fused_attn_block_cls(before) and type(base).__name__ == "PlainSelfAttn" and isinstance(base, PlainSelfAttn)
    return base


def test_graft_keeps_the_module_and_falls_back(monkeypatch, golden_dir):
    names = spy_on_launches(monkeypatch)
    _, x, _, st = load_fixture(golden_dir)
    m = _grafted()
    ptrs = [p.data_ptr() for p in m.parameters()]
    m.load_state_dict(st, strict=True)
    assert [p.data_ptr() for p in m.parameters()] == ptrs and sorted(m.state_dict()) == sorted(KEYS)
    plain = PlainSelfAttn()
    plain.load_state_dict(st, strict=True)
    # train mode with p > 0: the base class's forward, dropout included, the same random numbers
    m.train()
    plain.train()
    torch.manual_seed(0)
    a = m(x)
    torch.manual_seed(0)
    assert torch.equal(a, plain(x)) and m.calls == 1
    # a parameter that requires a gradient while grad is enabled
    m.eval()
    plain.eval()
    assert AB._module_kernel_cfg(m, x) is None
    y = m(x)
    assert y.requires_grad and torch.equal(y, plain(x)) and m.calls == 2
    # float64
    m.requires_grad_(False)
    m64 = _grafted().double().eval().requires_grad_(False)
    assert m64(x.double()).dtype == torch.float64 and m64.calls == 1
    # d_q != 32
    m16 = _grafted(f_dim=64).eval().requires_grad_(False)
    assert m16.d_q == 16 and AB._module_cfg(m16) is None and tuple(m16(torch.randn(1, 9, 64)).shape) == (1, 9, 64) and m16.calls == 1
    # over the fuse_self_attn graft the fall-back is that graft's forward: the base's self_attn is not called in eval mode
    both = _grafted(over_fused_core=True).eval().requires_grad_(False)
    both.load_state_dict(st, strict=True)
    assert torch.equal(both(x), plain(x)) and both.calls == 0
    assert names == []
    # what the kernel test of a module rests on, without a device: everything but the device holds here
    cfg = AB._module_cfg(m)
    assert cfg is not None and cfg[1:] == (4, (1e-6, 1e-6), 32 ** 0.5) and AB._shapes_ok(x, cfg[0], 4) and AB._frozen(cfg[0])
    assert not AB._shapes_ok(torch.zeros(1, 3, 193), AB.module_params(make_module(193)), 4)


def test_library_exports_the_attn_rows_symbols(gh_lib_path):
    L = C.CDLL(gh_lib_path)
    for sym in _abi.ATTN_ROWS_SYMBOLS:
        assert hasattr(L, sym), sym
    _abi.declare_attn_rows(L)
    assert sorted(_abi.ATTN_ROWS_SYMBOLS) == header_symbols("gh_attn_rows.h")
    assert set(_abi.ATTN_ROWS_SYMBOLS) <= set(_abi.ALL_SYMBOLS) and len(set(_abi.ALL_SYMBOLS)) == len(_abi.ALL_SYMBOLS)
    hdr = open(gh_lib_path.replace("guassianhand_amd/libgh_raster.so", "include/gh_attn_rows.h")).read()
    for name in ("GH_ATTN_ROWS_MAX_H", "GH_ATTN_ROWS_MAX_F"):
        assert f"#define {name} {getattr(_abi, name)}" in hdr, name


def test_struct_sizes_match_the_header(gh_lib_path):
    """GhAttnRowsDims: 4 int32, 2 floats, 4 int64; GhAttnRowsParams: sixteen pointers in the header's order."""
    assert C.sizeof(_abi.GhAttnRowsDims) == 4 * 4 + 2 * 4 + 4 * 8 and _abi.GhAttnRowsDims.x_stride.offset == 24
    assert C.sizeof(_abi.GhAttnRowsParams) == 16 * 8
    hdr = open(gh_lib_path.replace("guassianhand_amd/libgh_raster.so", "include/gh_attn_rows.h")).read()
    body = hdr[hdr.index("typedef struct GhAttnRowsParams"):hdr.index("} GhAttnRowsParams;")]
    assert tuple(re.findall(r"\*(\w+)", body[body.index("const float"):])) == _abi.ATTN_ROWS_PARAMS
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct GhAttnRowsDims"):hdr.index("} GhAttnRowsDims;")], flags=re.S)
    fields = [f.strip() for decl in re.findall(r"(?:int32_t|float|int64_t)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [n for n, _ in _abi.GhAttnRowsDims._fields_]


def test_c_abi_refuses_bad_arguments_before_any_launch(gh_lib_path):
    """Status codes for unsupported sizes, null pointers and a short workspace (fake addresses: nothing is launched)."""
    L = C.CDLL(gh_lib_path)
    _abi.declare_attn_rows(L)
    one = C.c_void_p(1 << 20)
    pm = _abi.GhAttnRowsParams(*([1 << 20] * 16))
    hole = _abi.GhAttnRowsParams(*([1 << 20] * 15))
    bad, uns, ok = _abi.GH_ERR_INVALID_ARG, _abi.GH_ERR_UNSUPPORTED, _abi.GH_OK
    dims = lambda V=10, F=131, H=4, hid=131, eps=1e-6, xs=131, os_=131, gs=131, ds=131: _abi.GhAttnRowsDims(V, F, H, hid, eps, eps, xs, os_, gs, ds)

    def pre(d, p=pm, X=one, qkv=one, st=one):
        return L.gh_attn_rows_pre_forward(C.byref(d), C.byref(p), X, None, qkv, st, None)

    def post(d, p=pm, y=one):
        return L.gh_attn_rows_post_forward(C.byref(d), C.byref(p), one, None, one, one, y, one, one, None)

    def post_b(d, ws=one, nbytes=1 << 20):
        return L.gh_attn_rows_post_backward(C.byref(d), C.byref(pm), one, None, one, one, one, one, ws, nbytes, None)

    def pre_b(d, ws=one, nbytes=1 << 20, dX=one):
        return L.gh_attn_rows_pre_backward(C.byref(d), C.byref(pm), one, None, one, one, one, one, ws, nbytes, dX, None)

    for call in (pre, post, post_b, pre_b):
        assert call(dims(F=193)) == call(dims(F=0)) == call(dims(hid=193)) == call(dims(hid=0)) == call(dims(H=0)) == call(dims(H=9)) == uns
        assert call(dims(V=(1 << 30) + 1)) == uns and call(dims(V=-1)) == bad and call(dims(eps=-1.0)) == call(dims(eps=float("nan"))) == bad
        assert call(dims(V=0)) == ok                                      # no rows: nothing to launch
        assert call(dims(V=0, F=193)) == uns                              # the sizes are judged first
    assert pre(dims(), p=hole) == post(dims(), p=hole) == bad
    assert pre(dims(), X=None) == pre(dims(), qkv=None) == pre(dims(), st=None) == pre(dims(xs=130)) == bad
    assert post(dims(), y=None) == post(dims(os_=130)) == post(dims(xs=5)) == bad
    assert post_b(dims(gs=130)) == post_b(dims(), ws=None) == post_b(dims(), ws=C.c_void_p((1 << 20) + 4)) == bad
    assert post_b(dims(), nbytes=16) == pre_b(dims(), nbytes=16) == _abi.GH_ERR_WORKSPACE_SMALL
    assert pre_b(dims(ds=130)) == pre_b(dims(), dX=None) == pre_b(dims(), ws=None) == bad
    assert L.gh_attn_rows_pre_forward(None, C.byref(pm), one, None, one, one, None) == bad
    ws = lambda *a, **k: L.gh_attn_rows_workspace_bytes(C.byref(dims(*a, **k)))
    assert 4 * 131 * 12320 <= ws(V=12320) < 4 * 131 * 12320 + 256 and ws(V=0) == ws(F=193) == ws(H=9) == ws(hid=0) == 0


@pytest.fixture
def no_livehand():
    """The two Uvd names register the livehand shim where livehand is absent: take it out again."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "livehand" or k.startswith("livehand.")}
    yield
    for k in [k for k in sys.modules if k == "livehand" or k.startswith("livehand.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    importlib.invalidate_caches()


def test_opt_in_renderer_names_resolve_lazily(no_livehand):
    import guassianhand_amd.tgs_renderer as T
    assert T._VARIANTS["FusedAttnBlock"] == T._VARIANTS["FusedAttn"] + ("block",) == ("attn", "block")
    assert T._VARIANTS["FusedAllFetchAttnBlock"] == T._VARIANTS["FusedAllFetchAttn"] + ("block",)
    assert T._VARIANTS["FusedAllFetchAttnBlockUvd"] == T._VARIANTS["FusedAllFetchAttnBlock"] + ("uvd",)
    assert all(row.index("attn") < row.index("block") for row in T._VARIANTS.values() if "block" in row)      # the block grafts what the core made
    with pytest.raises(AttributeError):
        T.GS3DRendererFusedGateAttnBlock
    have_reference = importlib.util.find_spec("tgs") is not None
    for name in ("GS3DRendererFusedAttnBlock", "GS3DRendererEditFusedAttnBlock", "GS3DRendererFusedAllFetchAttnBlock",
                 "GS3DRendererEditFusedAllFetchAttnBlock", "GS3DRendererFusedAllFetchAttnBlockUvd", "GS3DRendererEditFusedAllFetchAttnBlockUvd"):
        if not have_reference:                                     # the name is known: resolving it reaches for the reference's classes
            with pytest.raises(ImportError) as e:
                getattr(T, name)
            assert (e.value.name or "").split(".")[0] == "tgs"      # and for nothing else that is missing
            continue
        cls = getattr(T, name)
        assert isinstance(cls, type) and callable(cls.configure)
