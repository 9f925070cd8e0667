"""Time the refinement of the flagged points (guassianhand_amd.attn_block.refine_flagged, include/gh_attn_rows.h around
include/gh_attn.h) at the bench scene's size — B = 1, N = 98 562 points, F = 131, eight ranges of 12 320 — next to the path the
renderer classes without the block take, in the same process:

    fused    refine_flagged: one launch ahead of the cores and one behind over all flagged rows, one core call per range
    torch    the reference's loop statement (renderer_one_shot.py:554-574) over a module grafted by attention.fuse_self_attn: per
             range a boolean gather, the module's own LayerNorms and nn.Linear calls around the HIP attention core, a masked scatter

with 10 % and with 40 % of the rows flagged. NOBODY HAS MEASURED THE SHARE OF FLAGGED ROWS IN A REAL SCENE: the two shares bracket a
guess, they are not data. Parameters are frozen, as in the one-shot fit; `fwd` runs without a graph, `fwd_bwd` forward + backward to
the features.

Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows
alternating fused / torch / fused / torch; median, p10 and p90 per window. Each window runs under an alarm (`--step-timeout` seconds)
that ends the process. Also reported: the bytes either path holds for the backward per flagged row (the allocator's growth over a
forward whose graph is kept, less the result). Prints one line per window and ONE JSON line at the end; `--out FILE` also writes them
there (meant for profiles/attn_block_timing.txt).
usage: python tools/bench_attn_block.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import attention, attn_block  # noqa: E402

B, N, F_DIM, PART_ROWS, N_PART = 1, 98562, 131, 30000, 8


class ReferenceShaped(torch.nn.Module):
    """A module built as the reference's SelfAttn is (the same sub-modules under the same names, `self_attn` and `forward` as torch
    statements) that is not the package's own class, so that fuse_self_attn grafts it as it grafts the reference's."""

    def __init__(self, f_dim):
        super().__init__()
        src = attention.SelfAttn(f_dim)
        for name, child in src.named_children():
            setattr(self, name, child)
        self.n_heads, self.d_q, self.d_v, self.norm, self.f_dim = src.n_heads, src.d_q, src.d_v, src.norm, src.f_dim

    def self_attn(self, x):
        return attention.SelfAttn._torch_self_attn(self, x)

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm(x))
        return self.ff(x)


def reference_loop(features, flags, layer):
    """The statements of renderer_one_shot.py:554-574 for one batch element above 30 000 points, on a copy of the features."""
    feat = features * 1.0
    part_len = int(N / N_PART)
    fb, mb = feat[0].unsqueeze(0), flags[0].unsqueeze(0)
    if mb.max() > 0:
        for p in range(N_PART):
            part = mb * 0
            part[:, part_len * p:part_len * (p + 1)] = mb[:, part_len * p:part_len * (p + 1)]
            part = part.bool()
            if part.max() < 0.5:
                continue
            fb[part] = layer(fb[part].unsqueeze(0)).squeeze(0)
    return feat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    block = attention.SelfAttn(F_DIM).to(dev).eval().requires_grad_(False)
    core = ReferenceShaped(F_DIM)
    core.load_state_dict(block.state_dict())
    core = attention.fuse_self_attn(SimpleNamespace(self_attn_layer=core.to(dev).eval().requires_grad_(False))).self_attn_layer
    assert type(core) is attention.fused_self_attn_cls(ReferenceShaped)   # someone else's class, grafted: the HIP core, torch around it
    feat = torch.randn(B, N, F_DIM, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(B, N, F_DIM, generator=g).to(dev)

    def run(which, flags):
        return attn_block.refine_flagged(feat, flags, block, part_rows=PART_ROWS, n_part=N_PART) if which == "fused" else reference_loop(feat, flags, core)

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

    lines = [f"attention block timing: B={B} N={N} F={F_DIM} ranges={N_PART} x {int(N / N_PART)}, {args.warmup} warm-up + {args.iters} timed "
             f"iterations per window, device {torch.cuda.get_device_name(0)}",
             "the share of flagged rows in a real scene has not been measured: 10 % and 40 % are assumptions"]
    print("\n".join(lines), flush=True)
    result = {"B": B, "N": N, "F": F_DIM, "n_part": N_PART, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "flagged_share_is_an_assumption": True, "cases": {}}
    for share in (0.1, 0.4):
        flags = (torch.rand(B, N, generator=g) < share).to(dev)
        n_rows = int(flags[:, :N_PART * int(N / N_PART)].sum())
        with torch.no_grad():                                           # the two paths compute the same thing
            diff = float((run("fused", flags) - run("torch", flags)).abs().max())
        held = {}
        for which in ("fused", "torch"):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(dev)
            out = run(which, flags)
            torch.cuda.synchronize()
            held[which] = (torch.cuda.memory_allocated(dev) - before - out.numel() * 4) / n_rows
            del out
        lines.append(f"flagged {share:.0%}: {n_rows} rows refined; max |fused - torch| {diff:.3e}; held for the backward per flagged row: "
                     f"fused {held['fused']:.0f} B, torch {held['torch']:.0f} B")
        print(lines[-1], flush=True)

        def fwd(which):
            def fn():
                with torch.no_grad():
                    run(which, flags)
            return fn

        def fwd_bwd(which):
            def fn():
                torch.autograd.backward([run(which, flags)], [cot])
                feat.grad = None
            return fn

        for case, make in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            res = {"fused": [], "torch": []}
            for which in ("fused", "torch", "fused", "torch"):
                med, p10, p90 = window(make(which))
                res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
                lines.append(f"flagged {share:.0%} {case:8s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
                print(lines[-1], flush=True)
            spread = max(abs(ws[0]["median_ms"] - ws[1]["median_ms"]) for ws in res.values())   # between a path's two windows
            faster = max(w["median_ms"] for w in res["fused"]) + spread < min(w["median_ms"] for w in res["torch"])
            f = statistics.mean(w["median_ms"] for w in res["fused"])
            t = statistics.mean(w["median_ms"] for w in res["torch"])
            result["cases"][f"{int(100 * share)}pct_{case}"] = {
                "rows_refined": n_rows, "fused_ms": round(f, 4), "torch_ms": round(t, 4), "torch_over_fused": round(t / f, 3),
                "fused_windows": res["fused"], "torch_windows": res["torch"], "largest_window_spread_ms": round(spread, 4),
                "both_fused_medians_below_both_torch_medians_by_more_than_the_spread": bool(faster),
                "held_bytes_per_flagged_row": {k: round(v, 1) for k, v in held.items()}, "max_abs_difference": diff}
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
