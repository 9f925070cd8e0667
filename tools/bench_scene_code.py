"""Time the texture scene code (guassianhand_amd.scene_code, include/gh_scene.h) at the config's sizes — Ci = 512, Co = 80, two planes
of 32 x 32 tokens, float32, B = 1 and B = 4 — next to the reference's five statements (scene_code_ref: the token sum, detokenize,
ConvTranspose2d per plane, the cat and the map_bias add) on the same tensors in the same process:

    forward          the call without a gradient
    step_tokens      forward + backward with a frozen upsample: gradients of both token tensors and of map_bias
    step_bias        forward + backward with a frozen upsample: the gradient of map_bias only (the fit that trains it alone)

Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows
alternating between the paths, twice round; median, p10 and p90 per window, and per path the spread between its two windows. The peak
of torch.cuda.max_memory_allocated over one call of each path, above what is held before it, and the number of device kernels and
memory operations one call launches, with the time they take on the device (torch.profiler: the medians above also hold the host's
time between launches), are reported beside the times. Each window runs under an alarm
(`--step-timeout` seconds) that ends the process. Prints one line per window and ONE JSON line at the end; `--out FILE` also writes
them there, rewritten after every case (meant for profiles/scene_code_timing.txt).
usage: python tools/bench_scene_code.py [--iters 20] [--warmup 5] [--batches 1,4] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import scene_code as SC  # noqa: E402

CI, CO, NP, S = 512, 80, 2, 32


def launch_count(fn):
    """(count, summed device microseconds, {name: microseconds}) of the device kernels and memory operations of one call, by
    torch.profiler; count None where the profiler reports no device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        per, n = {}, 0
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                name = e.name.split("(")[0].split("<")[0].replace("void ", "")[:48]
                per[name] = round(per.get(name, 0.0) + float(e.time_range.elapsed_us()), 2)
                n += 1
    except Exception as e:  # noqa: BLE001  (a profiler that cannot start is a line in the record, not the end of the timing)
        return None, None, {f"profiler: {type(e).__name__}": str(e).splitlines()[0][:160] if str(e) else ""}
    return (n, round(sum(per.values()), 2), per) if n else (None, None, {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    dev = torch.device("cuda:0")
    lines = [f"scene code timing: Ci={CI} Co={CO} Np={NP} S={S} float32, {args.warmup} warm-up + {args.iters} timed iterations per window, "
             f"device {torch.cuda.get_device_name(0)}"]
    result = {"Ci": CI, "Co": CO, "Np": NP, "S": S, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "batches": {}}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def flush(final=False):
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines + ([json.dumps(result)] if final else [])) + "\n")

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
        qt = statistics.quantiles(ms, n=10)
        return statistics.median(ms), qt[0], qt[-1]

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated(dev) - held)

    torch.manual_seed(0)
    up = SC.TriplaneUpsampleNetwork(CI, CO, NP).to(dev).requires_grad_(False)                 # the fit freezes it
    for B in (int(s) for s in args.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        ta, tb = (torch.randn(B, CI, NP * S * S, generator=g).to(dev) for _ in range(2))
        map_bias = torch.randn(CO, 2 * S, NP * 2 * S, generator=g).to(dev)
        cot = torch.randn(B, 1, CO, 2 * S, NP * 2 * S, generator=g).to(dev)
        la, lb, lm = (t.clone().requires_grad_(True) for t in (ta, tb, map_bias))
        paths = {"fused": lambda a, b, m: SC.scene_code(up, (a, b), m), "torch": lambda a, b, m: SC.scene_code_ref(up, (a, b), m)}
        size = {"B": B}
        with torch.no_grad():
            size["fused_max_abs_diff_to_torch"] = float((paths["fused"](ta, tb, map_bias) - paths["torch"](ta, tb, map_bias)).abs().max())
        cases = {"forward": {w: (lambda fn=fn: fn(ta, tb, map_bias)) for w, fn in paths.items()},
                 "step_tokens": {w: (lambda fn=fn: torch.autograd.grad(fn(la, lb, lm), (la, lb, lm), cot)) for w, fn in paths.items()},
                 "step_bias": {w: (lambda fn=fn: torch.autograd.grad(fn(ta, tb, lm), (lm,), cot)) for w, fn in paths.items()}}
        for case, fns in cases.items():
            res = {w: [] for w in fns}
            ctx = torch.no_grad() if case == "forward" else torch.enable_grad()
            with ctx:
                for which in [w for _ in range(2) for w in fns]:
                    med, p10, p90 = window(fns[which])
                    res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
                    say(f"B={B} {case:11s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
                entry = {}
                for which, wins in res.items():
                    entry[f"{which}_ms"] = round(statistics.mean(w["median_ms"] for w in wins), 4)
                    entry[f"{which}_windows"] = wins
                    entry[f"{which}_window_spread_ms"] = round(abs(wins[0]["median_ms"] - wins[1]["median_ms"]), 4)
                    entry[f"{which}_peak_bytes"] = peak_of(fns[which])
                    signal.alarm(args.step_timeout)
                    entry[f"{which}_launches"], entry[f"{which}_device_us"], entry[f"{which}_launch_us"] = launch_count(fns[which])
                    signal.alarm(0)
                    say(f"B={B} {case:11s} {which:5s} mean of medians {entry[f'{which}_ms']:.4f} ms  window spread "
                        f"{entry[f'{which}_window_spread_ms']:.4f} ms  peak {entry[f'{which}_peak_bytes'] / 2 ** 20:.1f} MiB above the inputs  "
                        f"launches {entry[f'{which}_launches']} ({entry[f'{which}_device_us']} us on the device)")
                entry["torch_over_fused"] = round(entry["torch_ms"] / entry["fused_ms"], 3)
            size[case] = entry
            flush()
        result["batches"][str(B)] = size
    print(json.dumps(result), flush=True)
    flush(final=True)


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
