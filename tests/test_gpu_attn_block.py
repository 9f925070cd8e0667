"""The attention block on the device (include/gh_attn_rows.h and include/gh_attn.h through guassianhand_amd/attn_block.py).

Criterion, per field, printed with its three errors (the project's, from tests/test_gpu_self_attn.py):

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * scale,     scale = max|f64 field| + max|f64 x|

f64 is attn_block_ref with acc=torch.float64, torch32 is attn_block_ref in float32, both on the device.

Shapes are where the row kernels can go wrong: V around a tile's 64 rows (1, 63, 64, 65), several tiles with a partial last (129,
257), two batch elements, and one shape with other widths everywhere (F = 37, hid = 50, H = 1), so that no width is hard-coded.
Bitwise properties (row lists, permutations, positions, strides, run-to-run, graph replay) are asserted as equalities."""
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import attention as A
from guassianhand_amd import attn_block as AB
from tests.attn_block_cases import grad_run, make_input, make_module, reference_loop_parts, spy_on_launches
from tests.self_attn_cases import ROWS, PlainSelfAttn, errors, load_fixture

pytestmark = pytest.mark.gpu

BLOCK = ["gh_attn_rows_pre_forward", "gh_attn_forward", "gh_attn_rows_post_forward", "gh_attn_rows_post_backward", "gh_attn_backward",
         "gh_attn_rows_pre_backward"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def launches(monkeypatch):
    return spy_on_launches(monkeypatch)


@pytest.fixture(scope="module")
def module(dev):
    return make_module(device=dev)


def criterion(label, got, t32, f64, x, bad):
    for name, g, t, f in zip(("out", "grad_x"), got, t32, f64):
        assert g.dtype == torch.float32 and g.shape == f.shape and bool(torch.isfinite(g).all()), name
        s = (float(f.abs().max()) if f.numel() else 0.0) + (float(x.abs().max()) if x.numel() else 0.0)
        errors(f"{label} {name}", g, f, t, lambda e, s=s: 4 * e + 2.0 ** -20 * s, bad)


def check_block(label, m, x, cot, n_heads=4):
    P = AB.module_params(m)
    got = grad_run(lambda t: AB.attn_block(t, P, n_heads=n_heads), x, cot)
    t32 = grad_run(lambda t: AB.attn_block_ref(t, P, n_heads=n_heads), x, cot)
    f64 = grad_run(lambda t: AB.attn_block_ref(t, P, n_heads=n_heads, acc=torch.float64), x, cot, torch.float64)
    bad = []
    criterion(label, got, t32, f64, x, bad)
    assert not bad, bad
    return got


@pytest.mark.parametrize("V", [1, 63, 64, 65, 129, 257])
def test_forward_and_backward_meet_the_criterion(dev, module, launches, V):
    check_block(f"V={V}", module, *make_input(1, V, device=dev))
    assert launches == BLOCK


def test_two_batch_elements(dev, module):
    x, cot = make_input(2, 65, device=dev)
    got = check_block("BS=2 V=65", module, x, cot)
    for b in range(2):                                                 # a batch element alone gives the same bits
        alone = grad_run(lambda t: AB.attn_block(t, AB.module_params(module)), x[b:b + 1], cot[b:b + 1])
        assert torch.equal(alone[0][0], got[0][b]) and torch.equal(alone[1][0], got[1][b])


@pytest.mark.parametrize("f_dim,hid,n_heads", [(37, 50, 1), (192, 192, 8)])
def test_other_widths(dev, launches, f_dim, hid, n_heads):
    """Odd widths everywhere; and the largest ones, at which the two backward kernels' tiles of 64 rows pass 128 KiB of LDS and run 32
    rows per workgroup instead."""
    m = make_module(f_dim, hid=hid, n_heads=n_heads, seed=5, device=dev)
    assert (m.d_q, m.d_v, m.ff.fc1.out_features) == (32, 32, hid)
    check_block(f"F={f_dim} hid={hid} H={n_heads} V=70", m, *make_input(1, 70, f_dim, device=dev), n_heads=n_heads)
    assert launches == BLOCK


# ---- the module ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modules(dev, golden_dir):
    """(fx, x, cot, the grafted module with its parameters frozen, the ungrafted module, the float64 module), all on the device."""
    fx, x, cot, st = load_fixture(golden_dir)
    grafted, plain = PlainSelfAttn().to(dev), PlainSelfAttn().to(dev)
    m64 = PlainSelfAttn().double().to(dev)
    for m in (grafted, plain):
        m.load_state_dict(st, strict=True)
    m64.load_state_dict({k: t.double() for k, t in st.items()}, strict=True)
    for m in (grafted, plain, m64):
        m.eval().requires_grad_(False)
    r = SimpleNamespace(self_attn_layer=grafted)
    assert AB.fuse_attn_block(A.fuse_self_attn(r)).self_attn_layer is grafted
    assert type(grafted) is AB.fused_attn_block_cls(A.fused_self_attn_cls(PlainSelfAttn))
    return fx, x.to(dev), cot.to(dev), grafted, plain, m64


def test_grafted_module_against_the_fixture(dev, modules, launches):
    """The reference's own recorded run (out_r4, grad_x_r4) under the bound test_grafted_module_against_the_fixture of
    tests/test_gpu_self_attn.py applies to recorded values."""
    fx, x, cot, grafted, plain, m64 = modules
    y, gx = grad_run(grafted, x, cot)
    assert launches == BLOCK and grafted.calls == 0
    y32, gx32 = grad_run(plain, x, cot)
    y64, gx64 = grad_run(m64, x, cot, torch.float64)
    xs = float(x.abs().max())
    bad = []
    for name, got, t32, f64, recorded in (("out", y, y32, y64, fx["out_r4"]), ("grad_x", gx, gx32, gx64, fx["grad_x_r4"])):
        got, t32, f64 = got[:, ::ROWS], t32[:, ::ROWS], f64[:, ::ROWS]
        bound = lambda e, s=float(f64.abs().max()) + xs: 4 * e + 2.0 ** -20 * s
        errors(name, got, f64, t32, bound, bad)
        rec = torch.tensor(recorded).to(dev)
        e_rec = float((rec.double() - f64).abs().max())                 # the reference's own run, recorded on the CPU
        e32 = float((t32.double() - f64).abs().max())
        assert float((got.double() - rec.double()).abs().max()) <= bound(e32) + e_rec, name
    assert not bad, bad


def test_trainable_parameters_take_the_core_graft(dev, modules, launches):
    """A parameter that requires a gradient: the block steps aside for what the module did before, here fuse_self_attn's forward."""
    _, x, cot, grafted, plain, _ = modules
    grafted.requires_grad_(True)
    try:
        y, _ = grad_run(grafted, x, cot)
        assert launches == ["gh_attn_forward", "gh_attn_backward"] and y.shape == x.shape
        with torch.no_grad():                                           # no graph is asked for: nothing needs a parameter's gradient
            grafted(x)
        assert launches[2:] == BLOCK[:3]
    finally:
        grafted.requires_grad_(False)


# ---- the loop over the flagged rows ----------------------------------------------------------------------------------------------------
def _flags(B, N, share, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, generator=g) < share).to(dev)


def test_refine_flagged_against_the_loop(dev, module, launches):
    B, N, part_rows = 2, 1003, 1000
    flags = _flags(B, N, 0.3, 11, dev)
    flags[:, 1000:] = True                                             # flagged tail rows: never refined
    flags[1, 125:250] = False                                          # a range without a flag
    feat, cot = make_input(B, N, seed=2, device=dev)
    m64 = make_module(dtype=torch.float64, device=dev)
    got = grad_run(lambda t: AB.refine_flagged(t, flags, module, part_rows=part_rows), feat, cot)
    assert launches == ["gh_attn_rows_pre_forward"] + ["gh_attn_forward"] * 15 + ["gh_attn_rows_post_forward", "gh_attn_rows_post_backward"] + \
        ["gh_attn_backward"] * 15 + ["gh_attn_rows_pre_backward"]
    t32 = grad_run(lambda t: reference_loop_parts(t, flags, lambda r: AB.attn_block_ref(r, AB.module_params(module)), part_rows), feat, cot)
    f64 = grad_run(lambda t: reference_loop_parts(t, flags, m64, part_rows), feat, cot, torch.float64)
    bad = []
    criterion("refine_flagged", got, t32, f64, feat, bad)
    assert not bad, bad
    keep = ~flags
    keep[:, 1000:] = True
    assert 0.25 < float(flags[:, :1000].float().mean()) < 0.35
    assert torch.equal(got[0][keep], feat[keep]) and torch.equal(got[1][keep], cot[keep])   # copies of the input; the cotangent passed through
    assert not bool((got[0][~keep] == feat[~keep]).all(1).any())


def test_refine_flagged_launches_once_around_the_cores(dev, module, launches):
    flags = torch.zeros(1, 1003, dtype=torch.bool, device=dev)
    for p in (0, 3, 7):                                                # three non-empty ranges of 125
        flags[0, 125 * p + 5:125 * p + 70] = True
    feat, _ = make_input(1, 1003, seed=4, device=dev)
    out = AB.refine_flagged(feat, flags, module, part_rows=1000)
    assert launches == ["gh_attn_rows_pre_forward"] + ["gh_attn_forward"] * 3 + ["gh_attn_rows_post_forward"]
    for p in (0, 3, 7):                                                # each range attended among its own rows
        rows = slice(125 * p + 5, 125 * p + 70)
        assert torch.equal(out[:, rows], AB.attn_block(feat[:, rows].contiguous(), AB.module_params(module)))
    del launches[:]
    assert torch.equal(AB.refine_flagged(feat, torch.zeros_like(flags), module, part_rows=1000), feat) and launches == []


# ---- bitwise properties ------------------------------------------------------------------------------------------------------------------
def test_row_lists_permutations_and_positions(dev, module):
    P = AB.module_params(module)
    V = 65
    x, cot = make_input(1, V, seed=6, device=dev)
    base = grad_run(lambda t: AB.attn_block(t, P), x, cot)
    ar = torch.arange(V, dtype=torch.int32, device=dev)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(1)).to(dev).to(torch.int32)
    for idx in (ar, perm):                                             # idx=None is idx=arange; a permutation of the list permutes nothing
        got = grad_run(lambda t: AB.attn_block(t, P, idx=idx), x, cot)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # the same rows in the same order at other positions of a larger tensor: the same bits at their own indices, copies elsewhere
    place = torch.sort(torch.randperm(200, generator=torch.Generator().manual_seed(2))[:V])[0].to(dev)
    big, big_cot = make_input(1, 200, seed=7, device=dev)
    big[:, place], big_cot[:, place] = x, cot
    got = grad_run(lambda t: AB.attn_block(t, P, idx=place.to(torch.int32).flip(0)), big, big_cot)
    assert torch.equal(got[0][:, place], base[0]) and torch.equal(got[1][:, place], base[1])
    rest = torch.ones(200, dtype=torch.bool, device=dev)
    rest[place] = False
    assert torch.equal(got[0][:, rest], big[:, rest]) and torch.equal(got[1][:, rest], big_cot[:, rest])
    # among the same keys at another place of the launch: the second of two equal batch elements (row 64 sits in another tile and lane)
    two = grad_run(lambda t: AB.attn_block(t, P), x.expand(2, V, -1).contiguous(), cot.expand(2, V, -1).contiguous())
    assert torch.equal(two[0][1], base[0][0]) and torch.equal(two[1][1], base[1][0])
    # run to run
    again = grad_run(lambda t: AB.attn_block(t, P), x, cot)
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
    # an output tensor: the listed rows are written, the others stay
    out = torch.full((1, 200, 131), 3.0, device=dev)
    assert AB.attn_block(big, P, idx=place.to(torch.int32), out=out) is out
    assert torch.equal(out[:, place], base[0]) and bool((out[:, rest] == 3).all())


def test_strided_input_is_read_in_place(dev, module):
    """A column window of a wider tensor, row stride 140, gives the bits of its contiguous copy."""
    P = AB.module_params(module)
    g = torch.Generator().manual_seed(8)
    wide = torch.randn(1, 77, 140, generator=g).to(dev)
    cot = torch.randn(1, 77, 131, generator=g).to(dev)
    win = wide[..., 5:136]
    assert win.stride() == (77 * 140, 140, 1) and AB._rows2(win).data_ptr() == win.data_ptr()
    leaf = wide.clone().requires_grad_(True)
    out = AB.attn_block(leaf[..., 5:136], P)
    (gw,) = torch.autograd.grad((out * cot).sum(), leaf)
    want = grad_run(lambda t: AB.attn_block(t, P), win.contiguous(), cot)
    assert torch.equal(out, want[0]) and torch.equal(gw[..., 5:136], want[1]) and float(gw[..., :5].abs().max()) == 0.0
    # a cotangent with a row stride is read in place too
    wide_cot = torch.randn(1, 77, 140, generator=g).to(dev)
    a = grad_run(lambda t: AB.attn_block(t, P), win.contiguous(), wide_cot[..., 3:134].contiguous())
    xx = win.contiguous().requires_grad_(True)
    (b,) = torch.autograd.grad(AB.attn_block(xx, P), xx, wide_cot[..., 3:134])
    assert torch.equal(a[1], b)


def test_empty_inputs_launch_nothing(dev, module, launches):
    P = AB.module_params(module)
    for BS, V in ((1, 0), (0, 5), (0, 0)):
        x, cot = make_input(BS, V, device=dev)
        y, gx = grad_run(lambda t: AB.attn_block(t, P), x, cot)
        assert tuple(y.shape) == tuple(gx.shape) == (BS, V, 131)
    x, cot = make_input(1, 9, device=dev)
    y, gx = grad_run(lambda t: AB.attn_block(t, P, idx=torch.zeros(0, dtype=torch.int32, device=dev)), x, cot)
    assert torch.equal(y, x) and torch.equal(gx, cot)
    assert launches == []


def test_unsupported_sizes_take_the_torch_path(dev, launches):
    m = make_module(193, n_heads=4, device=dev)
    P = AB.module_params(m)
    x, cot = make_input(1, 20, 193, device=dev)
    got = grad_run(lambda t: AB.attn_block(t, P), x, cot)
    want = grad_run(lambda t: AB.attn_block_ref(t, P), x, cot)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    x, cot = make_input(1, 20, device=dev)
    m = make_module(device=dev)
    assert torch.equal(AB.attn_block(x, AB.module_params(m), ops="torch"), AB.attn_block_ref(x, AB.module_params(m)))
    m64 = make_module(dtype=torch.float64, device=dev)
    assert AB.attn_block(x.double(), AB.module_params(m64)).dtype == torch.float64
    assert launches == []


def test_graph_capture_replays_the_eager_bits(dev, modules):
    """The grafted module's forward and backward captured on one stream: one linear chain, no side stream."""
    _, x, cot, grafted, _, _ = modules
    eager = grad_run(grafted, x, cot)
    xl = x.clone().requires_grad_(True)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        out = grafted(xl)                                              # warm-up on the capture stream
        torch.autograd.grad((out * cot).sum(), (xl,))
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = grafted(xl)
        grads = torch.autograd.grad((out * cot).sum(), (xl,))
    for _ in range(2):
        out.zero_()
        grads[0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(grads[0], eager[1])
