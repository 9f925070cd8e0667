"""The Transformer1D backward to the parameters (include/gh_xf.h, transformer1d's grad="params") on the device. The criterion is
tests/fit_cases.three_way: the kernel, torch's float32 autograd and its float64 autograd run on the device on the same inputs, and per
field max|kernel - f64| <= 4 max|torch32 - f64| + 2^-20 max|f64|, no element excluded; the three errors are printed. Bit equality wherever
two paths perform the same float32 operations in the same order.

Fields that are one long float32 sum — dW and db of `linear_wgrad`, dgamma and dbeta of the two norms' single launches — are held through
transformer1d_params_cases.hold: to the three-way rule, and where one misses it only by its summation length, to the sum bound
n U sum|terms| + U |exact| of fit_cases.sum_within with n the documented chain length (plus the roundings inside a term). The whole
stack's fields are held to the three-way rule alone; their ratios are recorded under "xf_params_stack_*"."""
import ctypes as C

import pytest
import torch

from tests import transformer1d_cases as K
from tests import transformer1d_params_cases as P
from tests.fit_cases import bits, misaligned, three_way

pytestmark = pytest.mark.gpu

CASE_ID = lambda c: "C%d_h%d_D%d_L%d_B%d_N%d_%s" % (*c[:6], "attn2" if c[6] else "noattn2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert (_abi.GH_XF_WGRAD_ROWS, _abi.GH_XF_WGRAD_CHUNK, _abi.GH_XF_LNP_ROWS, _abi.GH_XF_GN_CHUNK) == (P.SLAB, P.WGRAD_CHUNK, P.LNP_ROWS, P.GN_CHUNK)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def X():
    from guassianhand_amd import transformer1d
    return transformer1d


def rnd(dev, *shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(17000 + seed)) * scale).to(dev)


# ---- gh_xf_linear_wgrad --------------------------------------------------------------------------------------------------------------------
def wgrad_kernel(X, d, pro, x=None, dy=None, **over):
    kw = {}
    if pro in ("ln", "gn"):
        kw.update(gamma=d["gamma"], beta=d["beta"])
    if pro == "ln":
        kw.update(moments=d["moments"])
    if pro == "gn":
        kw.update(groups=d["G"], eps=P.GN_EPS, moments=X.group_moments(d["x"], d["G"]))
    kw.update(over)
    dw, db = X.linear_wgrad(d["dy"] if dy is None else dy, d["x"] if x is None else x, prologue=pro, **kw)
    return {"dW": dw, "db": db}


@pytest.mark.parametrize("T", P.WGRAD_T)
def test_linear_wgrad(dev, X, T):
    """dW and db of every (K, N_out) x prologue at T rows per batch element against float64; then the same bits with dY channel first,
    with NaN behind the last row of every buffer, with strided and misaligned inputs, and with dW or db asked for alone."""
    for si, (K_, n_out) in enumerate(P.WGRAD_SHAPES):
        for pi, (pro, B) in enumerate(P.WGRAD_PROLOGUES):
            tag = f"wgrad T={T} K={K_} N_out={n_out} {pro} B={B}"
            d = P.wgrad_inputs(T, K_, n_out, pro, B, seed=100 * si + pi, device=dev)
            rows = B * T
            chunk = X.linear_wgrad_chunk(rows, K_, n_out)
            assert chunk == P.WGRAD_CHUNK
            got = wgrad_kernel(X, d, pro)
            f64, t32 = P.wgrad_ref(d, pro, torch.float64), P.wgrad_ref(d, pro, torch.float32)
            sums = {"dW": d["dy"].double().abs().t() @ P.wgrad_px(d, pro, torch.float64).abs(), "db": d["dy"].double().abs().sum(0)}
            P.hold(got, t32, f64, ("dW", "db"), sums, P.wgrad_chain(rows, chunk), tag, name="xf_wgrad")
            assert bool(torch.isfinite(got["dW"]).all()) and bool(torch.isfinite(got["db"]).all())
            same = lambda other, what: [torch.equal(bits(other[k]), bits(got[k])) for k in ("dW", "db")] == [True, True] or pytest.fail(f"{tag}: {what}")
            # dY channel first, as proj_out's cotangent arrives
            dy_cf = P.dy_channel_first(d)
            same(wgrad_kernel(X, d, pro, dy=dy_cf), "dy channel first")
            # NaN behind the last row of x, dy and the row moments: the rows past T are never read
            pad = 40 * max(K_, n_out) + K_ * T
            xn, _bx = P.with_nan_behind(d["x"], pad)
            dyn, _bd = P.with_nan_behind(d["dy"], pad)
            dcn, _bc = P.with_nan_behind(dy_cf, pad)
            over = {"moments": P.with_nan_behind(d["moments"], 128)[0]} if pro == "ln" else {}
            same(wgrad_kernel(X, d, pro, x=xn, dy=dyn, **over), "NaN behind T")
            same(wgrad_kernel(X, d, pro, x=xn, dy=dcn, **over), "NaN behind T, dy channel first")
            # 4-byte-misaligned and strided inputs
            if pro in ("gn", "cf"):
                same(wgrad_kernel(X, d, pro, x=misaligned(d["x"]), dy=K.strided_misaligned(d["dy"])), "misaligned")
            else:
                same(wgrad_kernel(X, d, pro, x=K.strided_misaligned(d["x"]), dy=K.strided_misaligned(d["dy"])), "strided, misaligned")
            same(wgrad_kernel(X, d, pro, dy=misaligned(dy_cf)), "dy channel first, misaligned")
            # either result alone
            only_w, only_b = wgrad_kernel(X, d, pro, want_b=False), wgrad_kernel(X, d, pro, want_w=False)
            assert only_w["db"] is None and only_b["dW"] is None
            assert torch.equal(bits(only_w["dW"]), bits(got["dW"])) and torch.equal(bits(only_b["db"]), bits(got["db"])), tag
            assert all(torch.equal(bits(v), bits(got[k])) for k, v in wgrad_kernel(X, d, pro).items()), tag   # two runs


# ---- the norms' parameter gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", P.WGRAD_T)
def test_layernorm_param_grads(dev, X, T):
    for K_ in P.NORM_K:
        x, dn = rnd(dev, T, K_, seed=T + K_) * 1.5 + 0.3, rnd(dev, T, K_, seed=T + K_ + 1)
        x64 = x.double()
        mom = torch.stack([x64.mean(1), (x64.var(1, unbiased=False) + P.LN_EPS).rsqrt()], dim=1).float()
        dg, db = X.layernorm_param_grads(dn, x, mom)
        got = {"dgamma": dg, "dbeta": db}
        xh = (x64 - x64.mean(1, keepdim=True)) * (x64.var(1, unbiased=False, keepdim=True) + P.LN_EPS).rsqrt()
        sums = {"dgamma": (dn.double() * xh).abs().sum(0), "dbeta": dn.double().abs().sum(0)}
        # a wave's share of a chunk of LNP_ROWS rows, the four waves' join, the chunks' join, three roundings inside a term
        n = P.LNP_ROWS // 4 + 2 + (T + P.LNP_ROWS - 1) // P.LNP_ROWS - 1 + 3
        P.hold(got, P.ln_grads_ref(x, dn, torch.float32), P.ln_grads_ref(x, dn, torch.float64), ("dgamma", "dbeta"), sums, n, f"LN grads T={T} K={K_}",
               name="xf_ln_param_grads")
        xs, dns = K.strided_misaligned(x), K.strided_misaligned(dn)
        dg2, db2 = X.layernorm_param_grads(dns, xs, misaligned(mom))
        assert torch.equal(bits(dg2), bits(dg)) and torch.equal(bits(db2), bits(db))


@pytest.mark.parametrize("N", P.GN_N)
def test_group_norm_param_grads(dev, X, N):
    for C_ in P.NORM_K:
        for B in (1, 2):
            x, dy = rnd(dev, B, C_, N, seed=N + C_ + B) * 1.5 + 0.3, rnd(dev, B, C_, N, seed=N + C_ + B + 1)
            mom = X.group_moments(x, 32)
            dg, db = X.group_norm_param_grads(dy, x, mom, 32)
            got = {"dgamma": dg, "dbeta": db}
            xh = P.group_norm(x.double(), 32)
            sums = {"dgamma": (dy.double() * xh).abs().sum((0, 2)), "dbeta": dy.double().abs().sum((0, 2))}
            # the butterfly's six steps and the four waves' two, the (batch, chunk) join, eight roundings inside a term (rstd from m2)
            n = 8 + B * ((N + P.GN_CHUNK - 1) // P.GN_CHUNK) - 1 + 8
            P.hold(got, P.gn_grads_ref(x, dy, 32, torch.float32), P.gn_grads_ref(x, dy, 32, torch.float64), ("dgamma", "dbeta"), sums, n,
                   f"GN grads N={N} C={C_} B={B}", name="xf_gn_param_grads")
            dg2, db2 = X.group_norm_param_grads(dy, x, mom, 32)
            assert torch.equal(bits(dg2), bits(dg)) and torch.equal(bits(db2), bits(db))


# ---- the whole stack -------------------------------------------------------------------------------------------------------------------------
def fused_grads(X, m, x, dout):
    n = K.StandIn.calls
    got, out = P.module_grads(X.fuse_transformer1d(m, grad="params"), m, x, dout)
    assert K.StandIn.calls == n                                   # the base forward did not run
    return got, out


@pytest.mark.parametrize("case", K.STACKS, ids=CASE_ID)
def test_stack_parameter_gradients(dev, X, case):
    Cc, heads, D, layers, B, N, attn2 = case
    name = "xf_params_stack_" + CASE_ID(case)
    m, x = P.trainable(case, device=dev)
    x.requires_grad_(True)
    dout = rnd(dev, B, Cc, N, seed=N)
    g64, g32 = P.autograd_grads(m, x, dout, torch.float64), P.autograd_grads(m, x, dout, torch.float32)
    got, out = fused_grads(X, m, x, dout)
    fields = ("dx", *[n_ for n_, _ in m.named_parameters()])
    assert set(got) == set(fields) == set(g64)
    three_way(got, g32, g64, fields, tag=name, name=name)
    # the bit equalities: out is the untaped forward, dx is grad="input"'s, two runs agree, and so does the function form
    with torch.no_grad():
        assert torch.equal(bits(out), bits(X.transformer1d(m, x)))
    frozen = K.make_module(Cc, heads, D, layers, attn2=attn2, seed=layers, device=dev).requires_grad_(False)
    dx_in, = torch.autograd.grad(X.transformer1d(frozen, x, grad="input"), x, dout)
    assert torch.equal(bits(got["dx"]), bits(dx_in))
    again, _ = fused_grads(X, m, x, dout)
    assert all(torch.equal(bits(again[k]), bits(got[k])) for k in fields)
    fn, _ = P.module_grads(lambda t: X.transformer1d(X.params_of(m), t, grad="params"), m, x, dout)
    assert all(torch.equal(bits(fn[k]), bits(got[k])) for k in fields)
    # with only x wanting a gradient the mode is grad="input"'s pair, with nothing wanted the plain kernels
    m.requires_grad_(False)
    assert torch.equal(bits(torch.autograd.grad(X.transformer1d(m, x, grad="params"), x, dout)[0]), bits(dx_in))


SMALL = (64, 2, 32, 2, 2, 65, True)


@pytest.fixture(scope="module")
def small(dev, X):
    """(module, x, dout, every gradient with everything wanted, out) of one small stack."""
    m, x = P.trainable(SMALL, device=dev)
    x.requires_grad_(True)
    dout = rnd(dev, 2, 64, 65, seed=3)
    got, out = fused_grads(X, m, x, dout)
    return m, x, dout, got, out


def test_a_gradient_asked_for_alone_has_the_same_bits(dev, X, small):
    m, x, dout, all_, _out = small
    try:
        for alone in ("transformer_blocks.0.attn2.to_k.weight", "transformer_blocks.1.norm1.weight", "proj_in.bias", "norm.weight",
                      "transformer_blocks.1.ff.net.0.proj.bias"):
            m.requires_grad_(False)
            dict(m.named_parameters())[alone].requires_grad_(True)
            got, _ = fused_grads(X, m, x.detach(), dout)
            assert list(got) == [alone] and torch.equal(bits(got[alone]), bits(all_[alone])), alone
    finally:
        m.requires_grad_(True)


def test_subsets(dev, X, small):
    m, x, dout, all_, out_all = small
    names = [n for n, _ in m.named_parameters()]
    try:
        # only the parameters
        got, out = fused_grads(X, m, x.detach(), dout)
        assert list(got) == names and all(torch.equal(bits(got[k]), bits(all_[k])) for k in names) and torch.equal(bits(out), bits(out_all))
        # only the last layer's ff2
        m.requires_grad_(False)
        ff2 = m.transformer_blocks[1].ff.net[2]
        ff2.requires_grad_(True)
        got, _ = fused_grads(X, m, x.detach(), dout)
        assert sorted(got) == ["transformer_blocks.1.ff.net.2.bias", "transformer_blocks.1.ff.net.2.weight"]
        assert all(torch.equal(bits(got[k]), bits(all_[k])) for k in got)
        # only x: grad="input"'s function carries it
        m.requires_grad_(False)
        fused = X.fuse_transformer1d(m, grad="params")
        o = fused(x)
        assert type(o.grad_fn).__name__.startswith("_InputGrad")
        assert torch.equal(bits(torch.autograd.grad(o, x, dout)[0]), bits(all_["dx"]))
        # nothing wanted: the plain kernels, no tape
        taped = []
        orig = X._run_tape
        X._run_tape = lambda *a: taped.append(1) or orig(*a)
        try:
            o = fused(x.detach())
            with torch.no_grad():
                o2 = fused(x)
        finally:
            X._run_tape = orig
        assert not taped and not o.requires_grad and not o2.requires_grad and torch.equal(bits(o), bits(out_all)) and torch.equal(bits(o2), bits(out_all))
    finally:
        m.requires_grad_(True)


def test_a_skipped_gradient_is_never_written(dev, X, small):
    """gh_xf_backward_params through the C entry point: every gradient buffer is a slice of one poisoned arena; only the slices whose
    pointers were passed change, they hold the autograd function's bits, and dx == NULL is taken."""
    from guassianhand_amd import _abi
    from guassianhand_amd._call import lib, stream, workspace
    m, x, dout, all_, _out = small
    p = X.params_of(m)
    packed = X._Packed(p)
    xc = x.detach().contiguous()
    with torch.no_grad():
        _o, tape = X._run_tape(packed, xc)
    stem_t, layers_t = packed.transposed()
    dims = X._dims(packed, xc)
    M = 64
    wanted = {(None, "out_b"): "proj_out.bias", (1, "ff2_w"): "transformer_blocks.1.ff.net.2.weight", (0, "ln2_w"): "transformer_blocks.0.norm2.weight",
              (0, "qkv1"): None}
    sizes = {(None, "out_b"): 64, (1, "ff2_w"): M * 4 * M, (0, "ln2_w"): M, (0, "qkv1"): 3 * M * M}
    POISON = -7.25
    arena = torch.full((sum(sizes.values()) + 64 * (len(sizes) + 1) + xc.numel(),), POISON, device=dev)
    gstem, glayers, at, where = _abi.GhXfStemG(), (_abi.GhXfLayerG * 2)(), 64, {}
    for key, n in sizes.items():
        where[key] = (at, n)
        setattr(gstem if key[0] is None else glayers[key[0]], key[1], arena[at:at + n].data_ptr())
        at += n + 64
    nbytes = int(lib().gh_xf_backward_params_workspace_bytes(C.byref(dims)))
    ws = workspace(nbytes, dev)
    rc = lib().gh_xf_backward_params(C.byref(dims), C.byref(stem_t), layers_t, C.byref(packed.stem), packed.layers, C.byref(gstem), glayers,
                                     xc.data_ptr(), tape.data_ptr(), dout.data_ptr(), None, ws.data_ptr(), nbytes, stream(dev))
    assert rc == _abi.GH_OK
    assert lib().gh_xf_backward_params(C.byref(dims), C.byref(stem_t), layers_t, C.byref(packed.stem), packed.layers, C.byref(gstem), glayers,
                                       xc.data_ptr(), tape.data_ptr(), dout.data_ptr(), None, ws.data_ptr(), nbytes - 1, stream(dev)) == _abi.GH_ERR_WORKSPACE_SMALL
    torch.cuda.synchronize()
    untouched = torch.ones_like(arena, dtype=torch.bool)
    for key, (o, n) in where.items():
        untouched[o:o + n] = False
        got = arena[o:o + n]
        if wanted[key] is not None:
            assert torch.equal(bits(got), bits(all_[wanted[key]].reshape(-1))), key
        else:
            a1 = m.transformer_blocks[0].attn1
            want = torch.cat([all_["transformer_blocks.0.attn1.to_%s.weight" % k] for k in "qkv"], dim=0)
            assert torch.equal(bits(got), bits(want.reshape(-1))) and a1.to_q.weight.shape == (M, M)
    assert bool((arena[untouched] == POISON).all())


def test_graph_capture_replays_bitwise(dev, X):
    m, x = P.trainable((64, 2, 32, 2, 2, 129, True), device=dev)
    x.requires_grad_(True)
    fused = X.fuse_transformer1d(m, grad="params")
    dout = rnd(dev, 2, 64, 129, seed=12)
    ins = [x, *m.parameters()]
    step = lambda: torch.autograd.grad(fused(x), ins, dout)
    eager = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gs = step()
    for _ in range(2):
        for t in gs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(gs, eager))


def test_an_optimiser_step_rebuilds_the_cached_weights(dev, X):
    m, x = P.trainable((64, 2, 32, 1, 1, 33, True), device=dev)
    fused = X.fuse_transformer1d(m, grad="params")
    dout = rnd(dev, 1, 64, 33, seed=4)
    a, _ = P.module_grads(fused, m, x, dout)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.add_(0.01 * torch.sign(p_))                        # what an optimiser does: in place, the version counter moves
    b, _ = P.module_grads(fused, m, x, dout)
    c, _ = P.module_grads(lambda t: X.transformer1d(X.params_of(m), t, grad="params"), m, x, dout)
    k = "transformer_blocks.0.attn1.to_q.weight"
    assert not torch.equal(a[k], b[k]) and all(torch.equal(bits(b[n]), bits(c[n])) for n in b)


def test_empty_inputs(dev, X):
    m, _x = P.trainable((64, 2, 32, 1, 1, 33, True), device=dev)
    for shape in ((0, 64, 33), (2, 64, 0)):
        x = torch.zeros(shape, device=dev, requires_grad=True)
        assert X.kernel_reason(m, x, grad="params") is None
        got, out = fused_grads(X, m, x, torch.zeros(shape, device=dev))
        assert tuple(out.shape) == shape and tuple(got["dx"].shape) == shape
        for n, p_ in m.named_parameters():
            assert got[n].shape == p_.shape and got[n].is_cuda and float(got[n].abs().max()) == 0.0, n


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_a_backbone_wider_than_the_data_product_takes_the_torch_path(dev, X):
    m = K.make_module(64, 16, 64, 1, seed=3, device=dev)         # M = 1024
    x = K.make_x(1, 64, 33, device=dev).requires_grad_(True)
    dout = rnd(dev, 1, 64, 33, seed=6)
    assert X.kernel_reason(m, x, grad="params") == "sizes"
    want, wout = P.module_grads(m, m, x, dout)                    # the base class's own forward and autograd
    g64 = P.autograd_grads(m, x, dout, torch.float64)
    n = K.StandIn.calls
    got, out = P.module_grads(X.fuse_transformer1d(m, grad="params"), m, x, dout)
    assert K.StandIn.calls == n + 1 and set(got) == set(want)
    assert float((out - wout).abs().max()) <= 2.0 ** -20 * float(wout.abs().max())
    three_way(got, want, g64, tuple(want), tag="M = 1024, the seam against the base forward")
    ref, _ = P.module_grads(lambda t: X.transformer1d(X.params_of(m), t, grad="params"), m, x, dout)   # the function form: the restatement
    three_way(ref, want, g64, tuple(want), tag="M = 1024, the restatement against the base forward")
