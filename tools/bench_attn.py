"""Time the interaction attention's core (guassianhand_amd.attention, include/gh_attn.h) at the reference's sizes — H = 4, D = 32,
float32, BS = 1, V = 1 540 and V = 12 320 (one part of the 8 the reference cuts N = 98 562 flagged points into) — next to the
reference's three statements (attention_ref: matmul / norm, softmax, matmul) and, where it accepts these inputs, next to
F.scaled_dot_product_attention, all on the same tensors in the same process:

    forward          the call without a gradient
    step             forward + backward (gradients of q, k and v)

SDPA is asked for each fused backend in turn (flash, then memory-efficient) under torch.nn.attention.sdpa_kernel; the first that
returns a finite result is timed and named, and a line says so when none does (the math backend is the three statements again and is
not timed). Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window,
windows alternating between the paths, twice round; median, p10 and p90 per window. The peak of torch.cuda.max_memory_allocated over one
step of each path, above what is held before it, is reported beside the times. Each window runs under an alarm (`--step-timeout`
seconds) that ends the process. Prints one line per window and ONE JSON line at the end; `--out FILE` also writes them there, rewritten
after every case (meant for profiles/attn_timing.txt).
usage: python tools/bench_attn.py [--iters 20] [--warmup 5] [--sizes 1540,12320] [--no-sdpa] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from guassianhand_amd import attention as A  # noqa: E402

H, D = 4, 32


def sdpa_backend(q, k, v, scale):
    """(name, context factory) of the first fused SDPA backend that takes these tensors, or (None, reasons)."""
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
    except ImportError as e:
        return None, {"import": str(e)}
    reasons = {}
    for name in ("FLASH_ATTENTION", "EFFICIENT_ATTENTION"):
        backend = getattr(SDPBackend, name, None)
        if backend is None:
            reasons[name] = "not in this torch"
            continue
        try:
            with sdpa_kernel(backend):
                o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale)
            torch.cuda.synchronize()
            if not bool(torch.isfinite(o).all()):
                raise RuntimeError("non-finite output")
            return name, (lambda b=backend: sdpa_kernel(b))
        except Exception as e:  # noqa: BLE001  (the refusal is the finding)
            reasons[name] = str(e).strip().splitlines()[0][:200] if str(e).strip() else type(e).__name__
    return None, reasons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1540,12320")
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    dev = torch.device("cuda:0")
    norm = float(torch.tensor(float(D)).sqrt())
    lines = [f"attention timing: H={H} D={D} float32 BS=1, {args.warmup} warm-up + {args.iters} timed iterations per window, device "
             f"{torch.cuda.get_device_name(0)}"]
    result = {"H": H, "D": D, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sizes": {}}

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

    for V in (int(s) for s in args.sizes.split(",")):
        g = torch.Generator().manual_seed(V)
        q, k, v = (torch.randn(1, V, H, D, generator=g).to(dev) for _ in range(3))
        cot = torch.randn(1, V, H * D, generator=g).to(dev)
        ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
        leaves = (ql, kl, vl)
        paths = {"fused": lambda a, b, c: A.attention(a, b, c, norm=norm), "torch": lambda a, b, c: A.attention_ref(a, b, c, norm)}
        size = {"V": V, "score_matrix_bytes": 4 * H * V * V}
        if not args.no_sdpa:
            signal.alarm(args.step_timeout)
            name, how = sdpa_backend(q, k, v, 1.0 / norm)
            signal.alarm(0)
            if name is None:
                say(f"V={V}: no fused SDPA backend took float32 (1, {H}, {V}, {D}): {how}")
                size["sdpa_backend"], size["sdpa_refusals"] = None, how
            else:
                say(f"V={V}: SDPA answered with {name}")
                size["sdpa_backend"] = name

                def sdpa(a, b, c, ctx=how):
                    with ctx():
                        o = F.scaled_dot_product_attention(a.transpose(1, 2), b.transpose(1, 2), c.transpose(1, 2), scale=1.0 / norm)
                    return o.transpose(1, 2).reshape(1, V, H * D)

                paths["sdpa"] = sdpa
        with torch.no_grad():
            want = paths["torch"](q, k, v)
            for which, fn in paths.items():
                size[f"{which}_max_abs_diff_to_torch"] = float((fn(q, k, v) - want).abs().max())
            del want
        cases = {"forward": {w: (lambda fn=fn: fn(q, k, v)) for w, fn in paths.items()},
                 "step": {w: (lambda fn=fn: torch.autograd.grad(fn(*leaves), leaves, cot)) for w, fn in paths.items()}}
        for case, fns in cases.items():
            res = {w: [] for w in fns}
            ctx = torch.no_grad() if case == "forward" else torch.enable_grad()
            with ctx:
                for which in [w for _ in range(2) for w in fns]:
                    med, p10, p90 = window(fns[which])
                    res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
                    say(f"V={V:6d} {case:8s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
                entry = {}
                for which, wins in res.items():
                    entry[f"{which}_ms"] = round(statistics.mean(w["median_ms"] for w in wins), 4)
                    entry[f"{which}_windows"] = wins
                    entry[f"{which}_window_spread_ms"] = round(abs(wins[0]["median_ms"] - wins[1]["median_ms"]), 4)
                    entry[f"{which}_peak_bytes"] = peak_of(fns[which])
                    say(f"V={V:6d} {case:8s} {which:5s} peak {entry[f'{which}_peak_bytes'] / 2 ** 20:.1f} MiB above the inputs")
                for which in res:
                    if which != "fused":
                        entry[f"{which}_over_fused"] = round(entry[f"{which}_ms"] / entry["fused_ms"], 3)
            size[case] = entry
            flush()
        result["sizes"][str(V)] = size
    print(json.dumps(result), flush=True)
    flush(final=True)


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
