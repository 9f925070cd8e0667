"""The point conditioning on the device (include/gh_cond.h through guassianhand_amd/cond.py) against its plain-torch restatement.

The tolerance is the three-way rule of tests/test_gpu_vert_mlp.py. For the output and the gradient of `code` three things are computed
on the same inputs on the device: the float64 restatement, the float32 torch path (torch.cat, F.layer_norm, F.linear, autograd) and
the kernels. The kernels pass when, per field,

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

The three errors, their ratio and the share of the bound used are printed per field."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guassianhand_amd import cond

from tests.cond_cases import LAYOUTS, make_case, point_rows, run

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _abi, _lib
    _lib.lib()
    assert _abi.GH_COND_ROWS == 64
    return torch.device("cuda:0")


def check(res, tag=""):
    bad, share = [], 0.0
    for k in res["f64"]:
        ref, t32, ker = res["f64"][k], res["torch32"][k], res["kernel"][k]
        assert ker.dtype == torch.float32 and ker.shape == ref.shape and ker.device == ref.device, (k, ker.shape, ref.shape)
        e_k = float((ker.double() - ref).abs().max()) if ref.numel() else 0.0
        e_t = float((t32.double() - ref).abs().max()) if ref.numel() else 0.0
        m = float(ref.abs().max()) if ref.numel() else 0.0
        bound = 4 * e_t + 2.0 ** -20 * m
        share = max(share, e_k / bound if bound else 0.0)
        print(f"{tag} {k:10s} kernel-f64 {e_k:.3e}  torch32-f64 {e_t:.3e}  max|f64| {m:.3e}  ratio {e_k / e_t if e_t else float('inf'):.2f}"
              f"  share of bound {e_k / bound if bound else 0.0:.2f}")
        if not e_k <= bound:
            bad.append((k, e_k, e_t, m))
    assert not bad, bad
    return share


def took_the_kernels(out):
    """Whether the autograd graph behind `out` holds the fused MLP's node."""
    seen, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "_CondMlpFn" in type(fn).__name__:
            return True
        todo += [f for f, _ in fn.next_functions]
    return False


def three_way(case, tag=""):
    res = {m: run(m, case) for m in ("f64", "torch32", "kernel")}
    check(res, tag)
    return res


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_shapes_and_layouts(dev, N, B, layout):
    """Rows per batch element around the 64-row tile, alone and with three batch elements (at N = 65 a tile straddles two, at N = 1 it
    holds three), crossed with every layout."""
    res = three_way(make_case(dev, B, N, layout), tag=f"N={N} B={B} {layout}")
    assert ("grad_code" in res["kernel"]) == (LAYOUTS[layout][3] > 0)


@pytest.mark.parametrize("scale", [0.05, 5.0])
def test_broadcast_vector_scale(dev, scale):
    """The batch-wide columns small and large against the row's own: the pairwise combination of the two variances."""
    three_way(make_case(dev, 2, 257, "full", seed=1, e_scale=scale), tag=f"e_scale={scale}")


def test_no_rows(dev):
    """B = 0 and N = 0: shapes and devices, without a launch; the backward gives an empty gradient."""
    t, params, _, L = make_case(dev, 2, 4, "full")
    for cut in (lambda v: v[:0], lambda v: v[:, :0]):
        e = t["e"][:0] if cut(t["uv"]).shape[0] == 0 else t["e"]
        code = cut(t["code"]).clone().requires_grad_(True)
        rows = cond.PointRows(uv=cut(t["uv"]), xyz=cut(t["xyz"]), flag=cut(t["flag"]), code=code, broadcast=(e,), levels=L)
        out = cond.cond_mlp(rows, params)
        assert tuple(out.shape) == (rows.B, rows.N, 51) and out.is_cuda and out.dtype == torch.float32
        out.sum().backward()
        assert tuple(code.grad.shape) == tuple(code.shape) and code.grad.is_cuda
        v = rows.varying()
        assert tuple(v.shape) == (rows.B, rows.N, 84) and v.is_cuda


@pytest.fixture(scope="module")
def c257(dev):
    case = make_case(dev, 1, 257, "full", seed=3)
    return case, run("kernel", case)


def test_nan_in_one_code_entry_stays_in_its_row(dev, c257):
    case, clean = c257
    t, params, cot, L = case
    dirty = dict(t)
    dirty["code"] = t["code"].clone()
    dirty["code"][0, 130, 17] = float("nan")
    got = run("kernel", (dirty, params, cot, L))
    keep = torch.arange(257, device=dev) != 130
    assert bool(torch.isnan(got["out"][0, 130]).all()) and bool(torch.isnan(got["grad_code"][0, 130]).all())
    assert torch.equal(got["out"][0, keep], clean["out"][0, keep]) and torch.equal(got["grad_code"][0, keep], clean["grad_code"][0, keep])


def test_strided_code_is_read_in_place_and_matches_the_copy_bitwise(dev, c257):
    """code = big[..., 5:38]: row stride 47, rows not 16-byte aligned."""
    case, full = c257
    t, params, cot, L = case
    big = torch.randn(1, 257, 47, device=dev)
    big[..., 5:38] = t["code"]
    view = big[..., 5:38]
    assert view.stride(1) == 47 and not view.is_contiguous()
    leaf = big.clone().requires_grad_(True)
    out = cond.cond_mlp(point_rows(t, L, leaf[..., 5:38]), params)
    (out * cot).sum().backward()
    assert torch.equal(out.detach(), full["out"]) and torch.equal(leaf.grad[..., 5:38], full["grad_code"])
    assert float(leaf.grad[..., :5].abs().max()) == 0.0 and float(leaf.grad[..., 38:].abs().max()) == 0.0
    v = point_rows(t, L, view).varying()
    assert torch.equal(v, point_rows(t, L).varying())


def test_row_130_alone_is_bitwise_the_same(dev, c257):
    case, full = c257
    t, params, cot, L = case
    one = {k: (v if k == "e" else v[:, 130:131]) for k, v in t.items()}
    got = run("kernel", (one, params, cot[:, 130:131], L))
    assert torch.equal(got["out"], full["out"][:, 130:131]) and torch.equal(got["grad_code"], full["grad_code"][:, 130:131])


def test_two_runs_are_bitwise_equal(dev, c257):
    case, full = c257
    again = run("kernel", case)
    assert torch.equal(again["out"], full["out"]) and torch.equal(again["grad_code"], full["grad_code"])
    assert float(full["grad_code"].abs().max()) > 0


def test_null_cotangent_writes_zeros(dev, c257):
    """gh_cond_mlp_backward with g_out = NULL: every element of dcode is written, as zero."""
    from guassianhand_amd import _abi, _call
    (t, params, _, L), _ = c257
    lib, ptr, stream = _call.lib(), _call.ptr, _call.stream(dev)
    flat = [t["uv"].reshape(-1, 2), t["xyz"].reshape(-1, 3), t["flag"].reshape(-1).float(), t["code"].reshape(-1, 33)]
    d = _abi.GhCondRows(*[x.data_ptr() for x in flat], 33, 33, L)
    ps = _call.struct(_abi.GhCondParams, params)
    n = int(lib.gh_cond_fold_bytes(1, 84, 51))
    fold = torch.empty(n // 4, device=dev)
    dcode = torch.full((257, 33), 7.0, device=dev)
    rc1 = lib.gh_cond_fold(ptr(t["e"]), 1, 768, 84, 51, C.byref(ps), ptr(fold), n, stream)
    rc2 = lib.gh_cond_mlp_backward(C.byref(d), 257, 257, 768, 51, C.byref(ps), ptr(fold), 1e-6, None, ptr(dcode), 33, stream)
    torch.cuda.synchronize()
    assert rc1 == 0 and rc2 == 0 and float(dcode.abs().max()) == 0.0
    assert bool(torch.isfinite(fold).all())


def test_forward_and_backward_are_graph_capturable(dev, c257):
    """Fold, forward and backward captured in one graph on a single stream, replayed once, equal to the eager result bitwise."""
    (t, params, cot, L), full = c257
    code = t["code"].detach().clone().requires_grad_(True)

    def step():
        out = cond.cond_mlp(point_rows(t, L, code), params)
        return [out] + list(torch.autograd.grad((out * cot).sum(), [code]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], full["out"]) and torch.equal(outs[1], full["grad_code"])


@pytest.mark.parametrize("L", [1, 4, 8])
def test_rows_alone(dev, L):
    """gh_cond_rows against torch's own SpatialEncoder statements on the device: the copied columns bit-equal, the sin / cos columns
    within 2 ulp of float32 at the value (the spread between two correctly documented sinf implementations)."""
    g = torch.Generator().manual_seed(40 + L)
    B, N, Cc = 2, 130, 33
    t = {"uv": torch.rand(B, N, 2, generator=g).to(dev), "xyz": (0.1 * torch.randn(B, N, 3, generator=g)).to(dev),
         "flag": (torch.rand(B, N, 1, generator=g) < 0.4).to(dev), "code": torch.randn(B, N, Cc, generator=g).to(dev), "e": None}
    rows = point_rows(t, L)
    got, want = rows.varying(), rows.dense()
    assert got.shape == want.shape == (B, N, 10 + 10 * L + 1 + Cc) and got.dtype == torch.float32
    trig = torch.zeros(got.shape[-1], dtype=torch.bool)
    trig[4:4 + 4 * L] = True
    trig[4 + 4 * L + 6:4 + 4 * L + 6 + 6 * L] = True
    trig = trig.to(dev)
    assert torch.equal(got[..., ~trig], want[..., ~trig])
    a, b = got[..., trig].cpu().numpy(), want[..., trig].cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(b), np.float32(2.0 ** -100)).astype(np.float32))
    off = np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp
    i = int(off.argmax())
    print(f"L={L}: worst sin / cos column {off.max():.2f} ulp at value {b.reshape(-1)[i]:.9e} (kernel {a.reshape(-1)[i]:.9e}); "
          f"{int((off > 0).sum())} of {off.size} differ")
    assert off.max() <= 2.0
    # without code, and flag alone
    assert torch.equal(cond.PointRows(uv=t["uv"], levels=L).varying(), got[..., :4 + 4 * L])
    assert torch.equal(cond.PointRows(flag=t["flag"], code=t["code"], levels=L).varying(), got[..., 10 + 10 * L:])
    # the gradient of code is the last Cc columns of the incoming gradient
    code = t["code"].clone().requires_grad_(True)
    cot = torch.randn(got.shape, generator=g).to(dev)
    (point_rows(t, L, code).varying() * cot).sum().backward()
    assert torch.equal(code.grad, cot[..., -Cc:])


def test_additional_features_on_the_fixture(dev, golden_dir):
    """The seam on the recorded tensors of the reference's module: output and gradient of identity_code_vert within twice the
    reference's own float32 error against float64 (the rule of tests/test_cond_cpu.py), and the kernels were what ran."""
    from test_cond_cpu import KEYS, fixture_case, within_twice
    fx = np.load(os.path.join(golden_dir, "cond_fixture.npz"), allow_pickle=False)
    inp, params, cot = fixture_case(fx)
    inp, params, cot = {k: v.to(dev) for k, v in inp.items()}, [p.to(dev) for p in params], cot.to(dev)
    m = cond.AdditionalFeaturesFC(852, 51).to(dev).eval()
    m.load_state_dict({KEYS[k]: p for k, p in zip(cond.PARAMS, params)}, strict=True)
    for p in m.parameters():
        p.requires_grad_(False)                                   # the one-shot fit's state: everything but the code is frozen
    code = inp["code"].clone().requires_grad_(True)
    out = cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], code, inp["pose"])
    assert took_the_kernels(out)
    (out * cot).sum().backward()
    c64 = inp["code"].clone().requires_grad_(True)
    rows64 = cond.PointRows(uv=inp["uv"], xyz=inp["xyz"], flag=inp["flag"], code=c64, broadcast=(inp["pose"],))
    out64 = cond._cond_mlp_ref(rows64, params, acc=torch.float64)
    (out64 * cot.double()).sum().backward()
    within_twice("out", out.detach().cpu(), fx["out"], out64.detach().cpu())
    within_twice("grad_code", code.grad.cpu(), fx["grad_code"], c64.grad.cpu())
    # a parameter that wants a gradient takes the torch path, and gets it
    m.ff1.fc1.weight.requires_grad_(True)
    out2 = cond.additional_features(m, inp["uv"], inp["xyz"], inp["flag"], code, inp["pose"])
    assert not took_the_kernels(out2)
    out2.sum().backward()
    assert m.ff1.fc1.weight.grad is not None


def test_train_mode_takes_the_torch_path(dev):
    """The module in train() with p = 0.1 returns exactly what the reference's statements return under the same seed."""
    t, params, _, L = make_case(dev, 2, 65, "full", seed=5)
    m = cond.AdditionalFeaturesFC(852, 51).to(dev)
    with torch.no_grad():
        for dst, src in zip(cond._block_params(m.ff1), params):
            dst.copy_(src)
    m.train()
    torch.manual_seed(11)
    got = cond.additional_features(m, t["uv"], t["xyz"], t["flag"], t["code"], t["e"])
    torch.manual_seed(11)
    feats = torch.cat([t["uv"], cond.spatial_encode(t["uv"], 4), t["xyz"], cond.spatial_encode(t["xyz"], 4), t["flag"], t["code"],
                       t["e"].repeat(1, 65, 1)], dim=-1)
    want = m.ff1.dropout2(m.ff1.fc2(m.ff1.dropout1(F.relu(m.ff1.fc1(m.ff1.layer_norm(feats))))))
    assert torch.equal(got, want)
    m.eval()
    with torch.no_grad():
        assert not torch.equal(cond.additional_features(m, t["uv"], t["xyz"], t["flag"], t["code"], t["e"]), want)


@pytest.mark.parametrize("layout", ["shade", "texture"])
def test_pointnet_forward_over_point_rows(dev, layout):
    """pool.pointnet_forward given a PointRows against the same encoder given dense(): the planes and the gradients of code (texture),
    the pose vector (shade) and fc_pos.weight, by the three-way rule (float64: the encoder in double, plain torch)."""
    from guassianhand_amd import pool
    B, N = 2, 257
    g = torch.Generator().manual_seed(70)
    r = lambda *s: torch.randn(*s, generator=g)
    uv, xyz = (2 * torch.rand(B, N, 2, generator=g) - 1).to(dev), (0.1 * r(B, N, 3)).to(dev)
    flag, code = (torch.rand(B, N, 1, generator=g) < 0.4).to(dev), (2 * torch.rand(B, N, 33, generator=g) - 1).to(dev)
    pose, cam = r(B, 1, 768).to(dev), r(B, 1, 768).to(dev)
    width = 1587 if layout == "shade" else 53
    torch.manual_seed(8)
    enc = pool.LocalPoolPointnet(input_channels=width, c_dim=16, hidden_dim=32, plane_size=8, n_blocks=3)
    for blk in enc.blocks:
        torch.nn.init.normal_(blk.fc_1.weight, std=0.2)
    enc = enc.to(dev).eval()
    cot = r(B, 16, 8, 8).to(dev)

    def one(mode):
        dt = torch.float64 if mode == "f64" else torch.float32
        e = copy.deepcopy(enc).to(dt)
        leaves = {"code": code.to(dt).requires_grad_(True), "pose": pose.to(dt).requires_grad_(True)}
        if layout == "shade":
            rows = cond.PointRows(uv=uv.to(dt), xyz=xyz.to(dt), flag=flag, broadcast=(leaves["pose"], cam.to(dt)))
        else:
            rows = cond.PointRows(uv=uv.to(dt), code=leaves["code"])
        planes = pool.pointnet_forward(e, rows if mode == "kernel" else rows.dense(), ops="torch" if mode == "f64" else "fused")
        leaf = leaves["pose"] if layout == "shade" else leaves["code"]
        grads = torch.autograd.grad((planes * cot.to(dt)).sum(), [leaf, e.fc_pos.weight])
        return {"planes": planes.detach(), "grad_pose" if layout == "shade" else "grad_code": grads[0], "grad_fc_pos_weight": grads[1]}

    res = {m: one(m) for m in ("f64", "torch32", "kernel")}
    assert tuple(res["kernel"]["planes"].shape) == (B, 16, 8, 8)
    check(res, tag=layout)


def test_the_concatenation_is_never_allocated(dev):
    """At N = 4,096, B = 1: the fused forward's peak allocation stays below a quarter of the (N, 852) float32 concatenation, and
    PointRows.linear's on the shade layout below a quarter of the (N, 1587) one. The outputs and the rows are 0.84 MB + 1.4 MB and
    4.2 MB + 0.84 MB against bounds of 3.5 MB and 6.5 MB; a path that built the concatenation cannot pass."""
    N = 4096
    t, params, _, L = make_case(dev, 1, N, "full", seed=6)
    code = t["code"].clone().requires_grad_(True)
    g = torch.Generator().manual_seed(3)
    cam = torch.randn(1, 1, 768, generator=g).to(dev)
    fc = torch.nn.Linear(1587, 256).to(dev)
    shade = cond.PointRows(uv=t["uv"], xyz=t["xyz"], flag=t["flag"], broadcast=(t["e"], cam))

    def peak(fn):
        out = fn()                                                  # once before measuring: lazily created handles and workspaces
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - base
        assert out.is_cuda
        return rise

    mlp = peak(lambda: cond.cond_mlp(point_rows(t, L, code), params))
    lin = peak(lambda: shade.linear(fc))
    print(f"peak rise: fused MLP {mlp} B against {N * 852 * 4 // 4}; linear (shade) {lin} B against {N * 1587 * 4 // 4}")
    assert mlp < N * 852 * 4 / 4 and lin < N * 1587 * 4 / 4
    dense = peak(lambda: cond.cond_mlp(point_rows(t, L, code), params, ops="torch"))
    assert dense > N * 852 * 4                                      # (the yardstick does build it)
