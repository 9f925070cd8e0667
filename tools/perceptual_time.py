"""Time the perceptual loss on the device: the full-width VGG19 slices with random weights, forward plus image gradient against a
cached target, the HIP path (ops="fused") against the torch statements (ops="torch", MIOpen) on the same device, alternating, and
the peak memory each allocates; then every convolution of the fused path alone, forward and backward-data, with the FLOP/s its shape
gives it (2 * 9 * Cin * Cout * N * H * W per direction, computed here from the shapes).

    python tools/perceptual_time.py [--out profiles/perceptual_time.txt] [--repeat 5] [--iters 10]

Times are device events around `iters` calls after a warm-up of every shape; the spread over `repeat` windows is printed with the
median. Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((8, 256, 256), (1, 256, 256))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual_time.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import perceptual as P
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    feats = P.VGG19Features().to(dev)
    with torch.no_grad():
        for _, n, _, _ in P.CONVS:
            c = feats.conv(n)
            c.weight.normal_(0.0, (2.0 / (9 * c.weight.shape[1])) ** 0.5)
            c.bias.normal_(0.0, 0.1)
    lines = [f"perceptual loss, VGG19 to relu4_1, random weights, float32, {torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the two paths alternating", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for B, H, W in SIZES:
        x, y = torch.rand(B, 3, H, W, device=dev), torch.rand(B, 3, H, W, device=dev)
        mods, steps = {}, {}
        for ops in ("fused", "torch"):
            mods[ops] = P.PerceptualLoss(feats, ops=ops)
            mods[ops].set_target(y)

            def step(ops=ops):
                xl = x.detach().requires_grad_(True)
                mods[ops](xl).backward()
                return xl.grad
            steps[ops] = step
        grads = {ops: steps[ops]() for ops in steps}                                     # warm-up of every shape, and the outputs
        for ops in steps:
            steps[ops]()
        torch.cuda.synchronize()
        rel = float((grads["fused"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        ms = {ops: [] for ops in steps}
        for _ in range(args.repeat):
            for ops in steps:
                ms[ops].append(timed(steps[ops], args.iters))
        peak = {}
        for ops in steps:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            steps[ops]()
            torch.cuda.synchronize()
            peak[ops] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        flop = 2 * sum(2 * 9 * feats.conv(n).weight.shape[1] * feats.conv(n).weight.shape[0] * B * (H >> s) * (W >> s)
                       for (_, n, _, _), s in zip(P.CONVS, (0, 0, 1, 1, 2, 2, 2, 2, 3)))
        say(f"{B}x3x{H}x{W}: forward + image gradient, cached target ({flop / 1e9:.1f} GFLOP in the convolutions, both directions)")
        for ops in steps:
            m = statistics.median(ms[ops])
            say(f"  ops={ops:5s}  {m:8.3f} ms [{min(ms[ops]):.3f} .. {max(ms[ops]):.3f}]  {flop / m / 1e9:6.1f} TFLOP/s end to end  "
                f"peak allocated above the inputs {peak[ops]:8.1f} MiB")
        say(f"  max|grad fused - grad torch| / max|grad torch| = {rel:.2e}")
        say("  per convolution, the HIP kernels alone (forward with ReLU and gate; backward-data through the gate):")
        s = 0
        for _, n, _, _ in P.CONVS:
            if n in P.POOL_BEFORE:
                s += 1
            conv = feats.conv(n)
            Cout, Cin = conv.weight.shape[:2]
            h, w = H >> s, W >> s
            xin, g = torch.randn(B, h, w, Cin, device=dev), torch.randn(B, h, w, Cout, device=dev)
            wf, wb = P.pack_weights(conv.weight)
            _, gate = P._conv_forward(xin, wf, conv.bias, Cout, True)
            P._conv_backward(g, gate, wb, Cin, True)
            wf_ = [timed(lambda: P._conv_forward(xin, wf, conv.bias, Cout, True), args.iters) for _ in range(args.repeat)]
            wb_ = [timed(lambda: P._conv_backward(g, gate, wb, Cin, True), args.iters) for _ in range(args.repeat)]
            tf, tb = statistics.median(wf_), statistics.median(wb_)
            fl = 2 * 9 * Cin * Cout * B * h * w
            say(f"    features.{n:<2d} {Cin:3d} -> {Cout:3d} at {h:3d}x{w:<3d}  forward {tf:7.3f} ms [{min(wf_):.3f} .. {max(wf_):.3f}] "
                f"{fl / tf / 1e9:6.1f} TFLOP/s   backward-data {tb:7.3f} ms [{min(wb_):.3f} .. {max(wb_):.3f}] {fl / tb / 1e9:6.1f} TFLOP/s")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
