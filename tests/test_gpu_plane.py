"""The plane fetch on the device (include/gh_plane.h through guassianhand_amd/plane.py).

Two yardsticks. (1) Bit equality with the project's own deterministic path on the channel-last copy of the plane: uvmap.uv_sample
forward (gh_uv_sample_forward) and its backward over host-built lists (uvmap.ActiveTexels, gh_uv_scatter_sorted). Both paths add the
same products in the same order, so equality is the contract, not a tolerance. (2) The measured rule of test_gpu_vert_mlp.py against
a float64 restatement: per field

    max|kernel - f64|  <=  4 * max|torch32 - f64|  +  2^-20 * max|f64|

with torch32 = F.grid_sample in float32 on the device; the three errors are printed. Shapes are where the kernels can go wrong: N
around the wave and the sort's 256-entry block, C with a slab tail and a second slab, maps of one texel, of odd sizes, the
reference's 64 x 128 (the sort's limit) and 90 x 91 = 8190 texels; UVs uniform in [-1.1, 1.1] with rows at exactly +-1."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 257, 4099)
CS = (1, 3, 65, 80)
MAPS = ((1, 1), (2, 3), (5, 7), (64, 128), (90, 91))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def launches(monkeypatch):
    """The names of the entry points plane.py calls, in order."""
    from guassianhand_amd import plane as P
    names, real = [], P.launch

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(P, "launch", spy)
    return names


def make_inputs(dev, N, C, Hp, Wp, seed=0):
    from test_plane_cpu import edge_uvs
    g = torch.Generator().manual_seed(1000 * seed + N + 7 * C + 13 * Hp + Wp)
    plane = torch.randn(C, Hp, Wp, generator=g)
    uv = edge_uvs(N, seed=seed + N) if N else torch.zeros(0, 2)
    cot = torch.randn(N, C, generator=g)
    return plane.to(dev), uv.to(dev), cot.to(dev)


def run(mode, plane, uv, cot, index=None):
    """(out (N,C), grad_plane (C,Hp,Wp)) with `cot` as the cotangent. mode: 'kernel' | 'torch32' | 'f64' | 'uvmap'."""
    from guassianhand_amd import plane as P, uvmap
    if mode == "uvmap":
        m = plane.permute(1, 2, 0).contiguous().requires_grad_(True)
        out = uvmap.uv_sample(m, uv)
        (g,) = torch.autograd.grad(out, m, cot)
        return out.detach(), g.permute(2, 0, 1).contiguous()
    p = plane.detach().clone().requires_grad_(True)
    if mode == "f64":
        out = P._plane_sample_ref(p[None], uv[None], acc=torch.float64)[0]
    else:
        out = P.plane_sample(p[None], uv[None], index=index, ops="torch" if mode == "torch32" else "fused")[0]
    (g,) = torch.autograd.grad(out, p, cot.to(out.dtype))
    return out.detach(), g


def check_rule(res, tag=""):
    bad = []
    for i, k in enumerate(("out", "grad_plane")):
        ref, t32, ker = res["f64"][i], res["torch32"][i], res["kernel"][i]
        assert ker.dtype == torch.float32 and ker.shape == ref.shape, (k, ker.shape, ref.shape)
        e_k = float((ker.double() - ref).abs().max()) if ref.numel() else 0.0
        e_t = float((t32.double() - ref).abs().max()) if ref.numel() else 0.0
        m = float(ref.abs().max()) if ref.numel() else 0.0
        print(f"{tag} {k:10s} kernel-f64 {e_k:.3e}  torch32-f64 {e_t:.3e}  max|f64| {m:.3e}")
        if not e_k <= 4 * e_t + 2.0 ** -20 * m:
            bad.append((tag, k, e_k, e_t, m))
    return bad


@pytest.mark.parametrize("Hp,Wp", MAPS)
@pytest.mark.parametrize("C", CS)
def test_shapes_bitwise_and_against_float64(dev, C, Hp, Wp):
    """Checks 1-4 for every N: forward and backward bitwise equal to the uvmap path, both under the float64 rule, and the device-built
    index equal to the plain-torch contract (integers equal, weights bitwise)."""
    from guassianhand_amd import plane as P
    bad = []
    for N in NS:
        plane, uv, cot = make_inputs(dev, N, C, Hp, Wp)
        if N == 0:                                                      # no points: shapes and a zero gradient
            out, grad = run("kernel", plane, uv, cot)
            assert tuple(out.shape) == (0, C) and tuple(grad.shape) == (C, Hp, Wp) and float(grad.abs().max()) == 0.0
            continue
        res = {m: run(m, plane, uv, cot) for m in ("f64", "torch32", "kernel")}
        assert tuple(res["kernel"][0].shape) == (N, C) and tuple(res["kernel"][1].shape) == (C, Hp, Wp)
        out_u, grad_u = run("uvmap", plane, uv, cot)
        assert torch.equal(res["kernel"][0], out_u), (N, "forward")
        assert torch.equal(res["kernel"][1], grad_u), (N, "backward")
        bad += check_rule(res, tag=f"N={N} C={C} {Hp}x{Wp}")
        ix = P.PlaneIndex(uv, Hp, Wp)
        ts, pairs, w = P.index_contract(uv.cpu(), Hp, Wp)
        assert torch.equal(ix.texel_start.cpu(), ts), N
        assert torch.equal(ix.pairs.cpu()[:int(ts[-1])], pairs), N
        assert torch.equal(ix.w.cpu(), w), N
        tail = ix.pairs.cpu()[int(ts[-1]):].long()                      # the pairs without a texel, each once
        inside = torch.zeros(4 * N, dtype=torch.bool)
        inside[pairs.long()] = True
        assert torch.equal(torch.sort(tail).values, torch.nonzero(~inside).reshape(-1)), N
    assert not bad, bad


def test_skew_all_points_at_one_uv(dev):
    """4096 points at one UV: four lists of 4096 pairs, each walked by one wave. Equal to the uvmap path bitwise; the run time of
    this test's kernel path is printed."""
    plane, _, cot = make_inputs(dev, 4096, 80, 64, 128, seed=3)
    uv = torch.tensor([[0.3137, -0.2718]], device=dev).repeat(4096, 1)
    out_u, grad_u = run("uvmap", plane, uv, cot)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, grad = run("kernel", plane, uv, cot)
    torch.cuda.synchronize()
    print(f"skew: index + forward + backward of 4096 points at one UV, C = 80, 64 x 128: {1e3 * (time.perf_counter() - t0):.2f} ms")
    assert torch.equal(out, out_u) and torch.equal(grad, grad_u)
    assert int((grad.abs().sum(0) > 0).sum()) == 4


@pytest.fixture(scope="module")
def p4099(dev):
    plane, uv, cot = make_inputs(dev, 4099, 80, 64, 128, seed=5)
    return plane, uv, cot, run("kernel", plane, uv, cot)


def test_backward_is_bitwise_reproducible(dev, p4099):
    plane, uv, cot, (out, grad) = p4099
    out2, grad2 = run("kernel", plane, uv, cot)
    assert torch.equal(out2, out) and torch.equal(grad2, grad)
    assert float(grad.abs().max()) > 0


def test_zero_cotangent_gives_zeros(dev, p4099):
    plane, uv, cot, _ = p4099
    _, grad = run("kernel", plane, uv, torch.zeros_like(cot))
    assert float(grad.abs().max()) == 0.0


def test_frozen_plane_launches_no_backward_and_no_index(dev, p4099, launches):
    from guassianhand_amd import plane as P
    plane, uv, cot, (out, _) = p4099
    res = P.plane_sample(plane[None], uv[None])
    assert not res.requires_grad and res.grad_fn is None and torch.equal(res[0], out)
    assert launches == ["gh_plane_sample_forward"]
    with torch.no_grad():                                               # a plane that needs a gradient, under no_grad: the same
        P.plane_sample(plane.clone().requires_grad_(True)[None], uv[None])
    assert launches == ["gh_plane_sample_forward"] * 2


def test_no_points_launch_nothing(dev, launches):
    from guassianhand_amd import plane as P
    p = torch.randn(1, 3, 5, 7, device=dev, requires_grad=True)
    out = P.plane_sample(p, torch.zeros(1, 0, 2, device=dev))
    assert tuple(out.shape) == (1, 0, 3) and out.is_cuda
    out.sum().backward()
    assert tuple(p.grad.shape) == (1, 3, 5, 7) and float(p.grad.abs().max()) == 0.0
    assert launches == []


def test_index_is_cached_per_uv_tensor_and_can_be_held(dev, p4099, launches):
    from guassianhand_amd import plane as P
    plane, uv, cot, (out, grad) = p4099
    uvb = uv[None].clone()
    for _ in range(2):                                                  # the same uv tensor: one index build
        p = plane.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(P.plane_sample(p[None], uvb)[0], p, cot)
        assert torch.equal(g, grad)
    assert launches.count("gh_plane_index") == 1
    uvb.add_(0.0)                                                       # a new version: built again
    P.plane_sample(plane.clone().requires_grad_(True)[None], uvb)
    assert launches.count("gh_plane_index") == 2
    held = P.PlaneIndex(uv, 64, 128)
    del launches[:]
    for _ in range(2):                                                  # a new uv object every step, a held index: no build
        p = plane.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(P.plane_sample(p[None], uv.clone()[None], index=held)[0], p, cot)
        assert torch.equal(g, grad)
    assert launches == ["gh_plane_sample_forward", "gh_plane_sample_backward"] * 2
    with pytest.raises(ValueError, match="index"):
        P.plane_sample(plane[None], uv[None, :100], index=held)


@pytest.mark.parametrize("held", [False, True])
def test_graph_capture_on_one_stream(dev, p4099, held):
    """Index build + forward + backward captured together (held=False), or forward + backward over an index built before the capture
    (held=True); replayed twice, each replay bitwise equal to the eager result."""
    from guassianhand_amd import plane as P
    plane, uv, cot, (out, grad) = p4099
    p = plane.clone().requires_grad_(True)
    before = P.PlaneIndex(uv, 64, 128) if held else None

    def step():
        ix = before if held else P.PlaneIndex(uv, 64, 128)
        o = P.plane_sample(p[None], uv[None], index=ix)[0]
        return [o.detach(), torch.autograd.grad(o, p, cot)[0]]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], out) and torch.equal(outs[1], grad)


def test_fallbacks(dev, launches):
    from guassianhand_amd import plane as P
    plane, uv, cot = make_inputs(dev, 257, 3, 5, 7, seed=7)
    u = uv.clone().requires_grad_(True)                                 # a UV gradient is torch's
    out = P.plane_sample(plane[None], u[None])
    (gu,) = torch.autograd.grad(out[0], u, cot)
    assert launches == [] and float(gu.abs().max()) > 0
    big, uvb, cotb = make_inputs(dev, 257, 3, 100, 100, seed=8)         # 10 000 texels: above the sort's limit
    p = big.clone().requires_grad_(True)
    out = P.plane_sample(p[None], uvb[None])
    (g,) = torch.autograd.grad(out[0], p, cotb)
    assert launches == [] and float(g.abs().max()) > 0                  # with a gradient: torch
    frozen = P.plane_sample(big[None], uvb[None])[0]                    # without: the kernels, any plane size
    assert launches == ["gh_plane_sample_forward"]
    assert torch.equal(frozen, run("uvmap", big, uvb, cotb)[0])
    assert P.plane_sample(big[None], uvb[None], ops="torch")[0].shape == frozen.shape and launches == ["gh_plane_sample_forward"]


@pytest.mark.parametrize("r", [1.0, 0.5])
@pytest.mark.parametrize("form", ["batched", "unbatched"])
def test_fuse_plane_fetch_reproduces_the_fixture(dev, golden_dir, launches, r, form):
    """fuse_plane_fetch on a stand-in that carries the reference's cfg.radius_texture; (1,N,2) / (1,1,80,64,128) and the unbatched
    form, on the fixture's inputs. The kernel's output and plane gradient are held to the float64 rule (torch32 = the reference's
    statements in float32 on the device); the recorded CPU values' own distance from float64 is printed beside them."""
    from types import SimpleNamespace
    from guassianhand_amd import plane as P
    from helpers import GoldenNpz
    from test_plane_cpu import fixture_case
    fx = GoldenNpz(os.path.join(golden_dir, "plane_fixture.npz"))
    plane, pos, cot = (t.to(dev) for t in fixture_case(fx, "big", r))

    def call(ops, dtype=torch.float32):
        me = SimpleNamespace(cfg=SimpleNamespace(radius_texture=r), plane_ops=ops)
        assert P.fuse_plane_fetch(me) is me
        p = plane.to(dtype).requires_grad_(True)
        if form == "batched":
            out = me.query_triplane_texture(pos.to(dtype)[None], p[None, None])
            assert tuple(out.shape) == (1, 64, 80)
            out = out[0]
        else:
            out = me.query_triplane_texture(pos.to(dtype), p[None])
            assert tuple(out.shape) == (64, 80)
        (g,) = torch.autograd.grad(out, p, cot.to(dtype))
        return out.detach(), g

    res = {"kernel": call("fused")}
    assert launches == ["gh_plane_index", "gh_plane_sample_forward", "gh_plane_sample_backward"]
    res["torch32"], res["f64"] = call("torch"), call("torch", torch.float64)
    assert res["f64"][0].dtype == torch.float64
    for i, k in enumerate(("out", "grad")):
        rec = torch.tensor(fx[f"big_r{r}_{form}_{k}"]).to(dev)
        print(f"r={r} {form} {k}: recorded-f64 {float((rec.double() - res['f64'][i]).abs().max()):.3e}  "
              f"kernel-recorded {float((res['kernel'][i] - rec).abs().max()):.3e}")
    bad = check_rule(res, tag=f"fixture r={r} {form}")
    assert not bad, bad
