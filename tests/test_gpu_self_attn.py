"""The interaction attention on the device (include/gh_attn.h through guassianhand_amd/attention.py).

Criterion, per field, printed with its three errors:

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * scale

f64 is attention_ref with acc=torch.float64, torch32 is attention_ref in float32, both on the device. scale: out max|v|; dv max|dout|;
dq max|dout| max|v| max|k| / norm; dk max|dout| max|v| max|q| / norm (the size of the terms that are added, not max|f64|: at V = 1 the
true dq and dk are exactly zero and any recomputation leaves about 1e-7). For the module's fields scale = max|f64 field| + max|f64 x|,
since the residual carries x.

Shapes are where the kernels can go wrong: V around a wave's 32 rows, a 32-key tile, the 64 rows staged per barrier and a workgroup's
128 rows, several tiles with a partial last, two batch elements, V = 4099 once. Bitwise properties (row and head permutations, inputs
read in place, run-to-run, the query-only backward, graph replay) are asserted as equalities."""
import math
from types import SimpleNamespace

import pytest
import torch

from guassianhand_amd import attention as A
from tests.self_attn_cases import F_DIM, KEYS, MATRICES, ROWS, PlainSelfAttn, errors, load_fixture, projected, run_module, sampled

pytestmark = pytest.mark.gpu

H, D = 4, 32
NORM = float(torch.tensor(32.0).sqrt())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def launches(monkeypatch):
    """The names of the entry points attention.py calls, in order."""
    names, real = [], A.launch

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(A, "launch", spy)
    return names


def make(dev, BS, V, seed=0, q_scale=1.0, d=D):
    g = torch.Generator().manual_seed(1000 * seed + 7 * BS + V)
    q, k, v = (torch.randn(BS, V, H, d, generator=g) for _ in range(3))
    cot = torch.randn(BS, V, H * d, generator=g)
    return (q * q_scale).to(dev), k.to(dev), v.to(dev), cot.to(dev)


def run(mode, q, k, v, cot, need=(True, True, True)):
    """(out, dq, dk, dv) with `cot` as the cotangent. mode: 'kernel' | 'torch32' | 'f64'."""
    dt = torch.float64 if mode == "f64" else torch.float32
    leaves = [t.detach().to(dt).clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
    if mode == "kernel":
        out = A.attention(*leaves)
    else:
        out = A.attention_ref(*leaves, norm=NORM, acc=torch.float64 if mode == "f64" else None)
    (out * cot.to(dt)).sum().backward()
    return (out.detach(),) + tuple(t.grad for t in leaves)


def check(label, q, k, v, cot):
    got, t32, f64 = (run(m, q, k, v, cot) for m in ("kernel", "torch32", "f64"))
    mx = lambda t: float(t.abs().max()) if t.numel() else 0.0
    scales = {"out": mx(v), "dq": mx(cot) * mx(v) * mx(k) / NORM, "dk": mx(cot) * mx(v) * mx(q) / NORM, "dv": mx(cot)}
    bad = []
    for i, name in enumerate(("out", "dq", "dk", "dv")):
        assert got[i].dtype == torch.float32 and got[i].numel() == f64[i].numel(), name
        assert bool(torch.isfinite(got[i]).all()), name
        errors(f"{label} {name}", got[i], f64[i], t32[i], lambda e, s=scales[name]: 4 * e + 2.0 ** -20 * s, bad)
    assert not bad, bad
    return got


@pytest.mark.parametrize("V", [1, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1031])
def test_forward_and_backward_meet_the_criterion(dev, V):
    check(f"V={V}", *make(dev, 1, V))


def test_two_batch_elements(dev):
    q, k, v, cot = make(dev, 2, 65)
    got = check("BS=2 V=65", q, k, v, cot)
    for b in range(2):                                             # a batch element alone gives the same bits
        alone = run("kernel", q[b:b + 1], k[b:b + 1], v[b:b + 1], cot[b:b + 1])
        for a, w in zip(alone, got):
            assert torch.equal(a.reshape(-1), w[b].reshape(-1))


def test_v_4099(dev):
    check("V=4099", *make(dev, 1, 4099))


def test_empty_inputs_launch_nothing(dev, launches):
    for BS, V in ((1, 0), (0, 5), (0, 0)):
        q, k, v, cot = make(dev, BS, V)
        out, dq, dk, dv = run("kernel", q, k, v, cot)
        assert tuple(out.shape) == (BS, V, H * D) and tuple(dq.shape) == tuple(dk.shape) == tuple(dv.shape) == (BS, V, H, D)
        lse = A.attention(q, k, v, return_lse=True)[1]
        assert tuple(lse.shape) == (BS, H, V)
    assert launches == []


def test_online_softmax_large_scores(dev):
    """q scaled by 8: scores reach about +-45, and the running maximum is superseded tile after tile."""
    q, k, v, cot = make(dev, 1, 300, q_scale=8.0)
    s = torch.einsum("bihd,bjhd->bhij", q, k) / NORM
    assert float(s.abs().max()) > 30
    check("q*8 V=300", q, k, v, cot)


def test_online_softmax_late_dominant_key(dev):
    """One key in the last tile that every query scores about 60 above the rest: everything summed before it is rescaled away."""
    q, k, v, cot = make(dev, 1, 300)
    q[..., 0] = 1.0
    k[..., 0] = 0.0
    k[:, 290, :, 0] = 60.0 * NORM
    s = torch.einsum("bihd,bjhd->bhij", q, k) / NORM
    rest = torch.cat([s[..., :290], s[..., 291:]], -1).amax(-1)
    assert float((s[..., 290] - rest).min()) > 50
    got = check("late key V=300", q, k, v, cot)
    assert float((got[0].view(1, 300, H, D) - v[:, 290:291]).abs().max()) < 1e-5      # the output is that key's value


def test_identical_rows_give_the_column_mean(dev):
    q, k, v, cot = make(dev, 1, 200)
    q, k = q[:, :1].expand(1, 200, H, D).contiguous(), k[:, :1].expand(1, 200, H, D).contiguous()
    out = A.attention(q, k, v)
    mean64 = v.double().mean(1, keepdim=True).expand(1, 200, H, D)
    t32 = A.attention_ref(q, k, v)
    bad = []
    errors("uniform out", out, mean64.reshape(1, 200, H * D), t32, lambda e: 4 * e + 2.0 ** -20 * float(v.abs().max()), bad)
    assert not bad, bad


def test_row_and_head_permutations_permute_the_result_bitwise(dev):
    q, k, v, _ = make(dev, 2, 203)
    out, lse = A.attention(q, k, v, return_lse=True)
    perm = torch.randperm(203, generator=torch.Generator().manual_seed(1)).to(dev)
    out_p, lse_p = A.attention(q[:, perm].contiguous(), k, v, return_lse=True)
    assert torch.equal(out_p, out[:, perm]) and torch.equal(lse_p, lse[:, :, perm])
    heads = torch.tensor([2, 0, 3, 1], device=dev)
    out_h, lse_h = A.attention(q[:, :, heads].contiguous(), k[:, :, heads].contiguous(), v[:, :, heads].contiguous(), return_lse=True)
    assert torch.equal(out_h.view(2, 203, H, D), out.view(2, 203, H, D)[:, :, heads]) and torch.equal(lse_h, lse[:, heads])
    # lse is what it says: ln sum exp(score)
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) / NORM
    assert float((lse.double() - torch.logsumexp(s, -1)).abs().max()) < 1e-5


def test_inputs_are_read_in_place(dev, launches):
    """q, k, v as column windows of one (BS, V, 384) tensor: no copy is made and the bits are those of the contiguous copies."""
    BS, V = 2, 77
    g = torch.Generator().manual_seed(5)
    big = torch.randn(BS, V, 3 * H * D, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(BS, V, H * D, generator=g).to(dev)
    wins = [big[..., i * H * D:(i + 1) * H * D].view(BS, V, H, D) for i in range(3)]
    for w in wins:
        assert not w.is_contiguous() and A._in_place(w).data_ptr() == w.data_ptr()
    out = A.attention(*wins)
    (out * cot).sum().backward()
    copies = [w.detach().contiguous().requires_grad_(True) for w in wins]
    out_c = A.attention(*copies)
    (out_c * cot).sum().backward()
    assert torch.equal(out, out_c)
    for i, c in enumerate(copies):
        assert torch.equal(big.grad[..., i * H * D:(i + 1) * H * D].reshape(BS, V, H, D), c.grad), "qkv"[i]
    # a last stride other than 1 takes one copy and gives the same result
    t = copies[0].detach().transpose(2, 3).contiguous().transpose(2, 3)
    assert t.stride(3) != 1 and A._in_place(t).data_ptr() != t.data_ptr()
    assert torch.equal(A.attention(t, copies[1].detach(), copies[2].detach()), out_c)
    assert launches.count("gh_attn_forward") == 3 and launches.count("gh_attn_backward") == 2


def test_backward_is_reproducible_zero_for_a_zero_cotangent_and_selective(dev, launches):
    q, k, v, cot = make(dev, 1, 333)
    a, b = run("kernel", q, k, v, cot), run("kernel", q, k, v, cot)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for gz in run("kernel", q, k, v, torch.zeros_like(cot))[1:]:
        assert float(gz.abs().max()) == 0.0
    only_q = run("kernel", q, k, v, cot, need=(True, False, False))
    assert only_q[2] is None and only_q[3] is None and torch.equal(only_q[1], a[1])
    only_kv = run("kernel", q, k, v, cot, need=(False, True, True))
    assert only_kv[1] is None and torch.equal(only_kv[2], a[2]) and torch.equal(only_kv[3], a[3])
    only_v = run("kernel", q, k, v, cot, need=(False, False, True))
    assert only_v[1] is None and only_v[2] is None and torch.equal(only_v[3], a[3])


def test_other_head_dimensions_take_the_torch_path(dev, launches):
    q, k, v, cot = make(dev, 1, 50, d=16)
    ql = q.clone().requires_grad_(True)
    out = A.attention(ql, k, v)
    assert torch.equal(out, A.attention_ref(q, k, v))
    (out * cot).sum().backward()
    qr = q.clone().requires_grad_(True)
    (A.attention_ref(qr, k, v) * cot).sum().backward()
    assert torch.equal(ql.grad, qr.grad)
    q, k, v, cot = make(dev, 1, 50)
    assert torch.equal(A.attention(q, k, v, ops="torch"), A.attention_ref(q, k, v))
    for dt in (torch.float64, torch.bfloat16):                     # a dtype other than float32 takes torch too, and does not raise
        a, b, c = q.to(dt), k.to(dt), v.to(dt)
        out = A.attention(a, b, c)
        assert out.dtype == dt and torch.equal(out, A.attention_ref(a, b, c))
    assert launches == []


def test_memory_stays_far_below_the_score_matrix(dev):
    """V = 8192: the peak over forward + backward, minus what was held before, stays below 1/8 of the 8192^2 x 4 x 4 B score matrix
    (a condition, not a measurement: q, k, v, out, the four gradients and lse total 32 MB)."""
    V = 8192
    q, k, v, cot = make(dev, 1, V)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    out = A.attention(q, k, v)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - held
    print(f"V={V}: peak {peak / 2 ** 20:.1f} MiB above the inputs; the score matrix is {V * V * 16 / 2 ** 20:.0f} MiB")
    assert peak < V * V * 4 * 4 // 8
    assert bool(torch.isfinite(q.grad).all()) and bool(torch.isfinite(k.grad).all()) and bool(torch.isfinite(v.grad).all())


def test_graph_capture_replays_the_eager_bits(dev):
    q, k, v, cot = make(dev, 1, 150)
    eager = run("kernel", q, k, v, cot)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        out = A.attention(ql, kl, vl)                              # warm-up on the capture stream
        torch.autograd.grad((out * cot).sum(), (ql, kl, vl))
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = A.attention(ql, kl, vl)
        grads = torch.autograd.grad((out * cot).sum(), (ql, kl, vl))
    for _ in range(2):
        out.zero_()
        for g in grads:
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out,) + tuple(grads), eager):
            assert torch.equal(got, want)


# ---- the module ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modules(dev, golden_dir):
    """(fx, x, cot, state, the grafted module on a stand-in renderer, the ungrafted module, the float64 module), all on the device."""
    fx, x, cot, st = load_fixture(golden_dir)
    grafted, plain = PlainSelfAttn().to(dev), PlainSelfAttn().to(dev)
    m64 = PlainSelfAttn().double().to(dev)
    for m in (grafted, plain):
        m.load_state_dict(st, strict=True)
    m64.load_state_dict({k: t.double() for k, t in st.items()}, strict=True)
    r = SimpleNamespace(self_attn_layer=grafted)
    assert A.fuse_self_attn(r).self_attn_layer is grafted and type(grafted) is A.fused_self_attn_cls(PlainSelfAttn)
    return fx, x.to(dev), cot.to(dev), st, grafted, plain, m64


def test_grafted_module_against_the_fixture(dev, modules, launches):
    fx, x, cot, st, grafted, plain, m64 = modules
    for m in (grafted, plain, m64):
        m.eval()
    y, gx, gp = run_module(grafted, x, cot)
    assert launches == ["gh_attn_forward", "gh_attn_backward"] and grafted.calls == 0
    y32, gx32, gp32 = run_module(plain, x, cot)
    y64, gx64, gp64 = run_module(m64, x.double(), cot.double())
    xs = float(x.abs().max())
    bad = []

    def field(name, got, t32, f64, recorded):
        bound = lambda e, s=float(f64.abs().max()) + xs: 4 * e + 2.0 ** -20 * s
        errors(name, got, f64, t32, bound, bad)
        if recorded is None:
            return
        rec = torch.tensor(recorded).to(dev)
        e_rec = float((rec.double() - f64).abs().max())               # the reference's own run, recorded on the CPU
        e32 = float((t32.double() - f64).abs().max())
        assert float((got.double() - rec.double()).abs().max()) <= bound(e32) + e_rec, name

    field("out", y[:, ::ROWS], y32[:, ::ROWS], y64[:, ::ROWS], fx["out_r4"])
    field("grad_x", gx[:, ::ROWS], gx32[:, ::ROWS], gx64[:, ::ROWS], fx["grad_x_r4"])
    for k in KEYS:
        name, got = sampled(k, gp[k])
        field(name, got, sampled(k, gp32[k])[1], sampled(k, gp64[k])[1], fx[name])
        if k in MATRICES:                                           # every row of the matrix's gradient, as one signed sum
            name, got = projected(k, gp[k])
            field(name, got, projected(k, gp32[k])[1], projected(k, gp64[k], round32=False)[1], fx[name])
        field(f"grad.{k} (all)", gp[k], gp32[k], gp64[k], None)
    assert not bad, bad


def test_masked_assignment_of_the_flagged_rows(dev, modules):
    """The reference's own statement `feat[mask] = layer(feat[mask].unsqueeze(0)).squeeze(0)` (renderer_one_shot.py:572) with about
    300 of 1000 rows flagged: the gradient of feat under the criterion against the ungrafted module."""
    _, _, _, _, grafted, plain, m64 = modules
    for m in (grafted, plain, m64):
        m.eval()
    g = torch.Generator().manual_seed(9)
    feat0 = torch.randn(1000, F_DIM, generator=g).to(dev)
    cot = torch.randn(1000, F_DIM, generator=g).to(dev)
    mask = (torch.rand(1000, generator=g) < 0.3).to(dev)
    assert 250 < int(mask.sum()) < 350

    def grad_of(layer, dt):
        leaf = feat0.to(dt).clone().requires_grad_(True)
        feat = leaf * 1.0
        feat[mask] = layer(feat[mask].unsqueeze(0)).squeeze(0)
        (feat * cot.to(dt)).sum().backward()
        return feat.detach(), leaf.grad

    (f, gf), (f32, gf32), (f64, gf64) = grad_of(grafted, torch.float32), grad_of(plain, torch.float32), grad_of(m64, torch.float64)
    xs = float(feat0.abs().max())
    bad = []
    errors("feat", f, f64, f32, lambda e: 4 * e + 2.0 ** -20 * (float(f64.abs().max()) + xs), bad)
    errors("grad_feat", gf, gf64, gf32, lambda e: 4 * e + 2.0 ** -20 * (float(gf64.abs().max()) + xs), bad)
    assert not bad, bad
    assert torch.equal(gf[~mask], cot[~mask])                          # rows that are not flagged pass through


def test_train_mode_takes_the_base_path(dev, modules, launches):
    _, x, _, _, grafted, plain, _ = modules
    grafted.train()
    plain.train()
    calls = grafted.calls
    torch.manual_seed(0)
    a = grafted(x)
    state_a = torch.cuda.get_rng_state(dev)
    torch.manual_seed(0)
    b = plain(x)
    assert torch.equal(a, b) and torch.equal(state_a, torch.cuda.get_rng_state(dev))
    assert grafted.calls == calls + 1 and launches == []
    for d in (grafted.dropout1, grafted.dropout2):
        d.p = 0.0
    try:
        grafted(x)
        assert launches == ["gh_attn_forward"] and grafted.calls == calls + 1      # p = 0: nothing to drop, the kernels again
    finally:
        for d in (grafted.dropout1, grafted.dropout2):
            d.p = 0.1
        grafted.eval()
        plain.eval()
    assert math.isfinite(float(a.detach().abs().max()))
