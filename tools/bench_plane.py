"""Time the plane fetch (guassianhand_amd.plane, include/gh_plane.h) at the reference's size — N = 98 562 points, a (80, 64, 128) texture
code — next to F.grid_sample(bilinear, align_corners=True) on the same tensors, in the same process:

    forward          plane_sample without a gradient (transpose + gather)          | grid_sample forward
    backward_held    the backward alone over a held PlaneIndex (one launch)        | grid_sample's backward alone (float atomics)
    index            PlaneIndex(uv, 64, 128) on its own (one kernel + the counting sort's three)
    step_held        forward + backward with a held index                          | grid_sample forward + backward
    step_new_uv      index build + forward + backward (a UV tensor that is new)    | the same torch figure

UVs are uniform in [-1, 1]^2 unless `--chart F` confines them to the central fraction F of the map (longer lists on fewer texels).
Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows
alternating fused / torch / fused / torch; median, p10 and p90 per window. Each window runs under an alarm (`--step-timeout` seconds)
that ends the process. Prints one line per window and ONE JSON line at the end; `--out FILE` also writes them there (meant for
profiles/plane_timing.txt).
usage: python tools/bench_plane.py [--iters 20] [--warmup 5] [--chart 1.0] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from guassianhand_amd import plane as P  # noqa: E402

N, C, HP, WP = 98562, 80, 64, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chart", type=float, default=1.0)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    planes = torch.randn(1, C, HP, WP, generator=g).to(dev)
    uv = ((torch.rand(1, N, 2, generator=g) * 2.0 - 1.0) * args.chart).to(dev)
    cot = torch.randn(1, N, C, generator=g).to(dev)
    leaf = planes.clone().requires_grad_(True)
    held = P.PlaneIndex(uv[0], HP, WP)
    counts = (held.texel_start[1:] - held.texel_start[:-1]).float()
    out_f = P.plane_sample(leaf, uv, index=held)
    out_t = P.plane_sample(leaf, uv, ops="torch")

    def grid(p):
        return F.grid_sample(p, uv[:, :, None], align_corners=True, mode="bilinear")

    def grid_bwd_out():
        o = grid(leaf)
        return o, cot.permute(0, 2, 1).reshape(o.shape).contiguous()

    o_t, cot_t = grid_bwd_out()
    cases = {
        "forward": {"fused": lambda: P.plane_sample(planes, uv), "torch": lambda: grid(planes)},
        "backward_held": {"fused": lambda: torch.autograd.grad(out_f, leaf, cot, retain_graph=True),
                          "torch": lambda: torch.autograd.grad(o_t, leaf, cot_t, retain_graph=True)},
        "index": {"fused": lambda: P.PlaneIndex(uv[0], HP, WP)},
        "step_held": {"fused": lambda: torch.autograd.grad(P.plane_sample(leaf, uv, index=held), leaf, cot),
                      "torch": lambda: torch.autograd.grad(grid(leaf), leaf, cot_t)},
        "step_new_uv": {"fused": lambda: torch.autograd.grad(P.plane_sample(leaf, uv, index=P.PlaneIndex(uv[0], HP, WP)), leaf, cot),
                        "torch": lambda: torch.autograd.grad(grid(leaf), leaf, cot_t)},
    }
    del out_t

    def window(fn):
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        signal.alarm(0)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        q = statistics.quantiles(ms, n=10)
        return statistics.median(ms), q[0], q[-1]

    lines = [f"plane timing: N={N} C={C} {HP}x{WP}, chart {args.chart}, lists per texel: max {int(counts.max())} mean {float(counts.mean()):.1f} "
             f"empty {int((counts == 0).sum())}, {args.warmup} warm-up + {args.iters} timed iterations per window, device "
             f"{torch.cuda.get_device_name(0)}"]
    result = {"N": N, "C": C, "Hp": HP, "Wp": WP, "chart": args.chart, "longest_list": int(counts.max()), "empty_texels": int((counts == 0).sum()),
              "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": {}}
    for case, fns in cases.items():
        res = {k: [] for k in fns}
        for which in [w for _ in range(2) for w in fns]:
            med, p10, p90 = window(fns[which])
            res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
            lines.append(f"{case:14s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
            print(lines[-1], flush=True)
        entry = {}
        for which, wins in res.items():
            entry[f"{which}_ms"] = round(statistics.mean(w["median_ms"] for w in wins), 4)
            entry[f"{which}_windows"] = wins
            entry[f"{which}_window_spread_ms"] = round(abs(wins[0]["median_ms"] - wins[1]["median_ms"]), 4)
        if "torch" in res:
            entry["torch_over_fused"] = round(entry["torch_ms"] / entry["fused_ms"], 3)
        result["cases"][case] = entry
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
