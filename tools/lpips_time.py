"""Time the evaluator's perceptual score on the device: lpips_scores over the full-width AlexNet with random weights (the real ones are
not shipped), full frames of 512x334 and 1024x1024, Nv = 1 and 8, the HIP path (ops="fused") against the torch statements (ops="torch",
MIOpen, view by view as the reference scores) on the same device, alternating; then every convolution of the fused path alone with
the FLOP/s its shape gives it (2 K K Cin Cout per output pixel, computed here from the shapes).

    python tools/lpips_time.py [--out profiles/lpips_time.txt] [--repeat 5] [--iters 20] [--kernels-only]

Times are device events around `iters` calls after a warm-up of every shape; the spread over `repeat` windows is printed with the
median. --kernels-only runs the fused path a few times and writes nothing: the workload of a rocprofv3 --kernel-trace --stats run.
Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1, 334, 512), (8, 334, 512), (1, 1024, 1024), (8, 1024, 1024))          # (Nv, H, W): the reference's frames are 512 wide, 334 high


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_time.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import lpips as LP
    dev = torch.device("cuda:0")
    net = LP.AlexLPIPS.synthetic(0).to(dev)
    gen = torch.Generator().manual_seed(0)
    if args.kernels_only:
        for Nv, H, W in SIZES:
            pred, gt = torch.rand(Nv, 3, H, W, generator=gen).to(dev), torch.rand(Nv, 3, H, W, generator=gen).to(dev)
            for _ in range(3):
                LP.lpips_scores(net, pred, gt)
        torch.cuda.synchronize()
        return
    lines = [f"lpips_scores, AlexNet widths {LP.WIDTHS}, random weights, float32, whole frames (no mask), quantize=True, {torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the two paths alternating", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for Nv, H, W in SIZES:
        pred, gt = torch.rand(Nv, 3, H, W, generator=gen).to(dev), torch.rand(Nv, 3, H, W, generator=gen).to(dev)
        steps = {ops: (lambda ops=ops: LP.lpips_scores(net, pred, gt, ops=ops)) for ops in ("fused", "torch")}
        outs = {ops: steps[ops]() for ops in steps}                                      # warm-up of every shape, and the outputs
        for ops in steps:
            steps[ops]()
        torch.cuda.synchronize()
        rel = float(((outs["fused"] - outs["torch"]).abs() / outs["torch"].abs()).max())
        ms = {ops: [] for ops in steps}
        for _ in range(args.repeat):
            for ops in steps:
                ms[ops].append(timed(steps[ops], args.iters))
        sizes, h, w, cin = [], H, W, 3
        for (_, K, s, p, pool), cout in zip(LP.CONVS, net.widths):
            if pool:
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            ho, wo = (h + 2 * p - K) // s + 1, (w + 2 * p - K) // s + 1
            sizes.append((cin, cout, K, s, p, h, w, ho, wo))
            h, w, cin = ho, wo, cout
        flop = sum(2 * K * K * ci * co * 2 * Nv * ho * wo for ci, co, K, _, _, _, _, ho, wo in sizes)
        med = {ops: statistics.median(ms[ops]) for ops in steps}
        say(f"Nv={Nv} {W}x{H}: {flop / 1e9:.1f} GFLOP in the convolutions (both images)")
        for ops in steps:
            say(f"  ops={ops:5s}  {med[ops]:9.3f} ms [{min(ms[ops]):.3f} .. {max(ms[ops]):.3f}]  {flop / med[ops] / 1e9:6.1f} TFLOP/s end to end")
        say(f"  fused / torch = {med['fused'] / med['torch']:.2f}   max|fused - torch| / |torch| = {rel:.2e}")
        say("  per convolution, the HIP kernel alone (bias and ReLU fused):")
        for k, (ci, co, K, s, p, h, w, ho, wo) in enumerate(sizes, 1):
            conv = getattr(net, f"conv{k}")
            xin, packed = torch.randn(2 * Nv, h, w, ci, device=dev), LP.pack_conv(conv.weight)
            run = lambda: LP.conv2d(xin, conv.weight, conv.bias, s, p, relu=True, packed=packed)
            run()
            win = [timed(run, args.iters) for _ in range(args.repeat)]
            t = statistics.median(win)
            fl = 2 * K * K * ci * co * 2 * Nv * ho * wo
            say(f"    conv{k} {ci:3d} -> {co:3d} k{K:<2d} s{s} at {h:4d}x{w:<4d} -> {ho:3d}x{wo:<3d}  {t:8.3f} ms [{min(win):.3f} .. {max(win):.3f}] "
                f"{fl / t / 1e9:6.1f} TFLOP/s")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
