"""The UV search on the device (include/gh_uvd.h through guassianhand_amd/uvd.py): criteria (a)-(c) of tests/uvd_cases.py over a sweep
of shapes and on the two-hand mesh, bitwise invariance under the split, the launch size, the point order and a rerun, the special
cases of the host file, graph replay, the no-launch case and the batch path with the hook in place."""
import ctypes as C

import pytest
import torch

from guassianhand_amd import _abi
from guassianhand_amd import uvd as U
from tests import uvd_cases as K

pytestmark = pytest.mark.gpu

N_SWEEP = (1, 63, 64, 65, 255, 256, 257, 1000)
F_SWEEP = (1, 2, 63, 64, 65, 200)          # the search stages nothing: no tile size to straddle, the loop fetches four records at a time


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _on(dev, *tensors):
    return tuple(t.to(dev) for t in tensors)


def _run(dev, pts, verts, faces, face_uv, **kw):
    out = U.closest_uv(*_on(dev, pts, verts, faces, face_uv), **kw)
    assert out[0].dtype == out[1].dtype == out[3].dtype == torch.float32 and out[2].dtype == torch.int64
    return tuple(t.cpu() for t in out)


def _points(verts, faces, n, seed):
    """On the mesh, lifted off it and far from it, a third each."""
    k = (n + 2) // 3
    far = verts.mean(0) + 3.0 * (verts.max(0).values - verts.min(0).values).norm() * torch.randn(k, 3, generator=torch.Generator().manual_seed(seed))
    return torch.cat([K.surface_points(verts, faces, k, seed=seed), K.off_surface_points(verts, faces, k, seed=seed)[0], far])[:n]


@pytest.mark.parametrize("F", F_SWEEP)
def test_shape_sweep(dev, F):
    verts, faces, face_uv = K.grid_mesh(F, seed=F)
    pts = _points(verts, faces, max(N_SWEEP), seed=F)
    d64 = K.loop_reference(pts, verts, faces)
    ref32 = U.closest_uv_ref(pts, verts, faces, face_uv)
    full = None
    for N in sorted(N_SWEEP, reverse=True):
        out = _run(dev, pts[:N], verts, faces, face_uv)
        K.check(f"N={N} F={F}", pts[:N], verts, faces, face_uv, out, tuple(t[:N] for t in ref32), d64[:N])
        full = full or out
        for got, want in zip(out, full):                                       # and the same bits whatever N
            assert torch.equal(got, want[:N]), (N, F)


@pytest.mark.parametrize("F", [20, 2])
def test_split_invariance(dev, F):
    """F = 20: uneven chunks (20 = 7 + 7 + 6, 16 chunks of 2 and 2 left over); F = 2: most chunks are empty."""
    verts, faces, face_uv = K.grid_mesh(F, seed=3)
    pts = _points(verts, faces, 700, seed=4)
    want = _run(dev, pts, verts, faces, face_uv, split=0)
    assert bool((want[2] >= 0).all()) and (F == 2 or len(set(want[2].tolist())) > 10)
    for split in (1, 2, 3, U.MAX_SPLIT):
        got = _run(dev, pts, verts, faces, face_uv, split=split)
        for name, g, w in zip(("uv", "d", "face", "bary"), got, want):
            assert torch.equal(g, w), (split, name)


def test_order_invariance(dev, golden_dir):
    verts, faces, face_uv = K.hand_mesh(golden_dir)
    pts = K.surface_points(verts, faces, 1000, seed=7)
    want = _run(dev, pts, verts, faces, face_uv)
    again = _run(dev, pts, verts, faces, face_uv)
    head = _run(dev, pts[:100], verts, faces, face_uv)
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(8))
    shuffled = _run(dev, pts[perm], verts, faces, face_uv)
    forced = _run(dev, pts, verts, faces, face_uv, split=5)
    for name, w, a, h, s, f in zip(("uv", "d", "face", "bary"), want, again, head, shuffled, forced):
        assert torch.equal(a, w) and torch.equal(h, w[:100]) and torch.equal(s, w[perm]) and torch.equal(f, w), name


def test_special_cases_on_the_device(dev):
    K.check_special_cases(lambda p, v, f, t: _run(dev, p, v, f, t))
    K.check_special_cases(lambda p, v, f, t: _run(dev, p, v, f.int(), t, split=3))


def test_hand_mesh(dev, golden_dir):
    verts, faces, face_uv = K.hand_mesh(golden_dir)
    pts = K.surface_points(verts, faces, K.N_HAND)
    d64 = K.loop_reference(pts, verts, faces)
    ref32 = tuple(t.cpu() for t in U.closest_uv_ref(*_on(dev, pts, verts, faces, face_uv)))
    out = _run(dev, pts, verts, faces, face_uv)
    K.check(f"hand N={K.N_HAND}", pts, verts, faces, face_uv, out, ref32, d64)
    assert float(out[0][:, 0].max()) <= 1.0 and float(out[0][:, 1].max()) <= 0.5 and float(out[0].min()) >= 0.0
    assert U.auto_split(K.N_HAND, 3076) > 1                                     # this shape runs the finish kernel


def test_graph_replay(dev):
    verts, faces, face_uv = K.grid_mesh(200, seed=5)
    pts = _points(verts, faces, 1000, seed=6)
    args = _on(dev, pts, verts, faces.int(), face_uv)
    for split in (1, 4):
        eager = U.closest_uv(*args, split=split)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            U.closest_uv(*args, split=split)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = U.closest_uv(*args, split=split)
        for _ in range(2):
            for o in outs:
                o.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for name, o, e in zip(("uv", "d", "face", "bary"), outs, eager):
                assert torch.equal(o, e), (split, name)


def test_no_points_launch_nothing(dev):
    verts, faces, face_uv = K.grid_mesh(8)
    out = _run(dev, torch.zeros(0, 3), verts, faces, face_uv)
    assert [tuple(t.shape) for t in out] == [(0, 2), (0,), (0,), (0, 3)]
    uv, _, rest = U.get_uvd(*_on(dev, torch.zeros(0, 3), verts, faces, face_uv))
    assert tuple(uv.shape) == (0, 2) and uv.is_cuda and tuple(rest["bary"].shape) == (0, 3)
    from guassianhand_amd import _lib
    assert _lib.lib().gh_uvd_forward(None, 0, None, 5, None, None, 8, 0, None, None, None, None, None, 0, None) == _abi.GH_OK
    uv = torch.full((4, 2), 7.0, device=dev)                                   # and with buffers given, none is written
    p = C.c_void_p(uv.data_ptr())
    assert _lib.lib().gh_uvd_forward(p, 0, p, 5, p, p, 8, 0, p, None, None, None, p, 16, None) == _abi.GH_OK
    torch.cuda.synchronize()
    assert bool((uv == 7.0).all())


def test_batch_path_with_the_hook(dev, golden_dir):
    """renderer.forward_single_batch with fuse_get_uvd on the stand-in namespace and the hand mesh, against the same call with
    closest_uv_ref (device, float32) as get_uvd, within the two-call protocol test's image tolerance (tests/test_gpu_single_batch.py).
    The points lie 1.5 mm off the mesh over the interior of the face that is nearest to them (in float64), and the stand-in
    refinement moves none: both choose the same face."""
    from helpers import BatchStandIns, batch_inputs
    from guassianhand_amd.renderer import forward_single_batch
    verts, faces, face_uv = K.hand_mesh(golden_dir)
    st, inp = BatchStandIns(dev, use_rgb=True), batch_inputs(N=400)
    st.Wr = torch.zeros_like(st.Wr)
    cand, lifted_from, _ = K.off_surface_points(verts, faces, 700, seed=9, lift_abs=0.0015)
    nearest = U.closest_uv_ref(cand, verts, faces, face_uv, acc=torch.float64)[2]      # where a crease or the other hand is nearer, the
    inp["pts"] = cand[nearest == torch.tensor(lifted_from)][:400]                      # closest point lies on a shared edge: a tie
    assert inp["pts"].shape[0] == 400
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    mesh = _on(dev, verts, faces, face_uv)
    seen = {}

    def ref_get_uvd(p, v, f, t):
        uv, dist, face, _ = U.closest_uv_ref(p, v, f, t)
        seen["ref"] = face
        return uv, dist, None

    def run(ns):
        return forward_single_batch(ns, d["feat"], d["pts"], d["w2cs"], d["Ks"], d["H"], d["W"], 0.71, 1.42, d["bg"], color_w=d["color_w"],
                                    xyz_b=d["xyz_b"], color_b=d["color_b"], opacity_b=d["opacity_b"], vert3d_uv=mesh[0][None],
                                    face_uv=mesh[1], face_uv_xy=mesh[2])

    fused_ns = U.fuse_get_uvd(st.namespace(dev))
    assert fused_ns.get_uvd is U.get_uvd
    got = run(fused_ns)
    ref_ns = st.namespace(dev)
    ref_ns.get_uvd = ref_get_uvd
    want = run(ref_ns)
    n = got["3dgs"].xyz.shape[0]
    assert n > 400 and torch.equal(got["3dgs"].xyz, want["3dgs"].xyz)          # kept and duplicated points
    pts = torch.cat([d["pts"][d["feat"][:, 0] > st.threshold_low], d["pts"][d["feat"][:, 0] > st.threshold_high]])
    assert torch.equal(U.closest_uv(pts, *mesh)[2], seen["ref"])                # the same faces, as the docstring promises
    for k in ("comp_rgb", "comp_mask"):
        err = (got[k] - want[k]).abs().max().item()
        print(f"uvd batch {k}: {err:.3g}")
        assert err <= 2e-6, (k, err)
    assert float(got["comp_mask"].max()) > 0.5 and float(got["comp_rgb"].std()) > 0.01
