"""Time the UV search (guassianhand_amd.uvd, include/gh_uvd.h) at the workload's shape — N = 98 562 points on and near the two-hand
UV-topology mesh of the tests (V = 1810, F = 3076: 3.0e8 point-triangle pairs) — in one process:

    split=1, 2, 4, 8, 16   closest_uv with a forced split (records + search, and the finish kernel when split > 1); `--splits` for others
    auto                   closest_uv with split=0: gh_uvd_auto_split(N, F), which the tool prints
    ref                    closest_uv_ref on the device in float32: the only other implementation there is here

Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, two windows
per path, the paths alternating; median, p10 and p90 per window. Each window runs under an alarm (`--step-timeout` seconds) that ends
the process. Prints one line per window, whether auto is within 10 % of the best forced split, and ONE JSON line at the end;
`--out FILE` also writes them there (meant for profiles/uvd_timing.txt).
usage: python tools/bench_uvd.py [--iters 20] [--warmup 5] [--n 98562] [--splits 1,2,4,8,16] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from guassianhand_amd import uvd as U  # noqa: E402
from tests import uvd_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=98562)
    ap.add_argument("--splits", default="1,2,4,8,16")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    splits = tuple(sorted({1} | {int(x) for x in args.splits.split(",")}))
    dev = torch.device("cuda:0")
    verts, faces, face_uv = K.hand_mesh(os.path.join(ROOT, "tests", "golden"))
    pts = K.surface_points(verts, faces, args.n, seed=0)
    pts, verts, faces, face_uv = pts.to(dev), verts.to(dev), faces.int().to(dev), face_uv.to(dev)
    N, F = pts.shape[0], faces.shape[0]
    auto = U.auto_split(N, F)
    paths = {f"split={s}": (lambda s=s: U.closest_uv(pts, verts, faces, face_uv, split=s)) for s in splits}
    paths["auto"] = lambda: U.closest_uv(pts, verts, faces, face_uv)
    paths["ref"] = lambda: U.closest_uv_ref(pts, verts, faces, face_uv)
    want = paths["split=1"]()
    same = all(all(torch.equal(a, b) for a, b in zip(paths[k](), want)) for k in paths if k != "ref")
    ref = paths["ref"]()
    face_agree = float((ref[2] == want[2]).float().mean())
    d_diff = float((ref[1] - want[1]).abs().max())

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

    lines = [f"uvd timing: N={N} V={verts.shape[0]} F={F} ({N * F:.3g} pairs), auto split {auto}, {args.warmup} warm-up + {args.iters} timed "
             f"iterations per window, device {torch.cuda.get_device_name(0)}",
             f"outputs bitwise equal over splits and auto: {same}; ref (float32) picks the same face for {100 * face_agree:.1f} % of the "
             f"points, max |d - d_ref| {d_diff:.3g}"]
    print("\n".join(lines), flush=True)
    res = {k: [] for k in paths}
    for which in [w for _ in range(2) for w in paths]:
        med, p10, p90 = window(paths[which])
        res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
        lines.append(f"{which:9s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
        print(lines[-1], flush=True)
    result = {"N": N, "V": int(verts.shape[0]), "F": F, "auto_split": auto, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "bitwise_equal_over_splits": same, "paths": {}}
    for which, wins in res.items():
        result["paths"][which] = {"ms": round(statistics.mean(w["median_ms"] for w in wins), 4), "windows": wins,
                                  "window_spread_ms": round(abs(wins[0]["median_ms"] - wins[1]["median_ms"]), 4)}
    best = min(splits, key=lambda s: result["paths"][f"split={s}"]["ms"])
    result["best_forced_split"] = best
    result["auto_over_best_forced"] = round(result["paths"]["auto"]["ms"] / result["paths"][f"split={best}"]["ms"], 3)
    result["ref_over_auto"] = round(result["paths"]["ref"]["ms"] / result["paths"]["auto"]["ms"], 1)
    lines.append(f"best forced split {best} ({result['paths'][f'split={best}']['ms']:.4f} ms); auto (split {auto}) {result['paths']['auto']['ms']:.4f} ms = "
                 f"{result['auto_over_best_forced']:.3f} x the best: {'within' if result['auto_over_best_forced'] <= 1.10 else 'NOT within'} 10 %; "
                 f"ref {result['paths']['ref']['ms']:.2f} ms")
    print(lines[-1], flush=True)
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
