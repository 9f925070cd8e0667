"""Time the hand points on the device: pose_hands for two hands of synthetic_model(20, 39) (V = 780, three levels, 46,665 points
each, the second with the mirrored winding) at B = 1 and B = 32, forward alone and forward plus the gradient of all four inputs, the
HIP path (ops="fused") against the torch statements (ops="torch", mano_ref per hand) on the same device, alternating. The parent of
this block had no device path at all, so mano_ref on the device is the only baseline there is.

    python tools/mano_time.py [--out profiles/mano_time.txt] [--repeat 5] [--iters 20]

Times are device events around `iters` calls after a warm-up of every shape; the spread over `repeat` windows is printed with the
median. Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mano_time.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mano_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import mano as M
    dev = torch.device("cuda:0")
    models = (M.synthetic_model(20, 39, seed=0), M.synthetic_model(20, 39, seed=1, flip=True))
    P = sum(m.n_points for m in models)
    lines = [f"hand points, 2 x synthetic_model(20, 39): V = 780, levels = 3, {P} points per parameter set, float32, {torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the two paths alternating", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for B in BATCHES:
        g = torch.Generator().manual_seed(B)
        ps = [t.to(dev) for t in (0.5 * torch.randn(B, 2, 3, generator=g), 0.5 * torch.randn(B, 2, 45, generator=g),
                                  torch.randn(B, 2, 10, generator=g), 0.3 * torch.randn(B, 2, 3, generator=g))]
        gp, gj = torch.randn(B, P, 3, generator=g).to(dev), torch.randn(B, 32, 3, generator=g).to(dev)
        steps = {}
        for ops in ("fused", "torch"):
            def fwd(ops=ops):
                with torch.no_grad():
                    return M.pose_hands(models, *ps, ops=ops)

            def both(ops=ops):
                leaves = [p.detach().requires_grad_(True) for p in ps]
                out = M.pose_hands(models, *leaves, ops=ops)
                return torch.autograd.grad([out.points, out.joints], leaves, [gp, gj])
            steps[ops] = {"forward": fwd, "forward + backward": both}
        outs = {ops: (steps[ops]["forward"](), steps[ops]["forward + backward"]()) for ops in steps}        # warm-up, and the outputs
        torch.cuda.synchronize()
        rel_p = float((outs["fused"][0].points - outs["torch"][0].points).abs().max() / outs["torch"][0].points.abs().max())
        rel_g = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs["fused"][1], outs["torch"][1]))
        say(f"B = {B}")
        for what in ("forward", "forward + backward"):
            ms = {ops: [] for ops in steps}
            for _ in range(args.repeat):
                for ops in steps:
                    ms[ops].append(timed(steps[ops][what], args.iters))
            for ops in steps:
                m = statistics.median(ms[ops])
                say(f"  {what:18s} ops={ops:5s}  {m:8.3f} ms [{min(ms[ops]):.3f} .. {max(ms[ops]):.3f}]")
        say(f"  max|points fused - torch| / max|points| = {rel_p:.2e};  largest such figure over the four gradients = {rel_g:.2e}")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
