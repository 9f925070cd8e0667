"""Time metrics.image_scores (gh_image_scores: MSE, PSNR, SSIM of a stack of views) on the device for 1 and 8 views at 512x334
and at 1024x1024, both layouts: eager calls (host + launches, the caller's view), the same call replayed from a captured HIP graph
(the device time of the three kernels plus one graph launch), and the float64 CPU restatement of the same scores for scale.
usage: python tools/metrics_time.py [n_calls]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from guassianhand_amd.metrics import image_scores

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def inputs(nv, H, W, layout):
    g = torch.Generator().manual_seed(nv * H + W)
    gt = torch.rand(nv, 3, H, W, generator=g)
    pred = (gt + 0.05 * torch.randn(nv, 3, H, W, generator=g)).clamp(0, 1)
    mask = torch.zeros(nv, H, W, dtype=torch.uint8)
    mask[:, H // 8:H - H // 8, W // 8:W - W // 8] = 1
    bb = torch.ones(nv, H, W, dtype=torch.uint8)
    if layout == "hwc":
        pred, gt = pred.permute(0, 2, 3, 1).contiguous(), gt.permute(0, 2, 3, 1).contiguous()
    return pred, gt, mask, bb


def per_call_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


print(f"{'views':>5} {'H x W':>10} {'layout':>6} {'eager ms':>9} {'graph ms':>9} {'CPU f64 ms':>11} {'ssim':>9}")
for nv, H, W in ((1, 512, 334), (8, 512, 334), (1, 1024, 1024), (8, 1024, 1024)):
    for layout in ("chw", "hwc"):
        cpu = inputs(nv, H, W, layout)
        pred, gt, mask, bb = (t.to(dev) for t in cpu)
        call = lambda: image_scores(pred, gt, mask, bbox_mask=bb, layout=layout)
        eager = per_call_ms(call, n)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        replay = per_call_ms(graph.replay, n)
        k = 3 if H * W * nv <= 512 * 334 * 8 else 1
        t0 = time.perf_counter()
        for _ in range(k):
            ref = image_scores(*cpu[:3], bbox_mask=cpu[3], layout=layout)
        t_cpu = (time.perf_counter() - t0) / k * 1e3
        torch.cuda.synchronize()
        d = (out.ssim.cpu() - ref.ssim).abs().max().item()
        assert d <= 1e-6, d
        print(f"{nv:>5} {f'{H}x{W}':>10} {layout:>6} {eager:>9.4f} {replay:>9.4f} {t_cpu:>11.1f} {out.ssim[0].item():>9.6f}")
        del graph
