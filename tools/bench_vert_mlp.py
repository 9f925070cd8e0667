"""Time the fused vertex MLP block (guassianhand_amd.vert_mlp, include/gh_vert.h) at the reference's size — N = 98 562 rows, Cf = 131 —
next to the reference-shaped torch modules it replaces, in eval() mode, in the same process:

    gate_fwd             gs_valid(features, positions) over all N rows, no gradient
    refine_frozen        vert_pos_refinement forward + backward on the rows the gate scores above 0.9; features and positions require a
                         gradient, the parameters do not (one backward launch)
    refine_trainable     the same with the parameters requiring a gradient (two backward launches)

    fused    one launch forward; the backward recomputes the forward
    torch    torch.cat + nn.LayerNorm + three nn.Linear + the elementwise launches between them (dropout inactive)

The gate's head is scaled so that its scores spread over (0, 1); how many rows pass 0.9 is reported. Device events around every
iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows alternating fused / torch /
fused / torch; median, p10 and p90 per window. Bytes: the one-read minimum of the forward is N * (Cf + 3) * 4 in and N * K * 4 out; the
backward's adds the cotangent in and grad_x, grad_pts out (the trainable backward also writes and re-reads its per-workgroup
partials). Each window runs under an alarm (`--step-timeout` seconds) that ends the process. Prints one line per window and ONE JSON
line at the end; `--out FILE` also writes them there (meant for profiles/vert_mlp_timing.txt).
usage: python tools/bench_vert_mlp.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import vert_mlp as V  # noqa: E402

N, CF = 98562, 131
D, HD = CF + 3, (CF + 3) // 4


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
    x = torch.randn(N, CF, generator=g).to(dev)
    pts = (0.1 * torch.randn(N, 3, generator=g)).to(dev)
    torch.manual_seed(0)
    mods = {}
    for name, make in (("gate", lambda ops: V.VertValid(CF, ops=ops)), ("refine", lambda ops: V.VertPosRefinement(CF, ops=ops))):
        fused = make("fused").to(dev).eval()
        plain = make("torch").to(dev).eval()                        # ops="torch": the same layers through torch.cat / F.layer_norm / F.linear
        with torch.no_grad():
            if name == "gate":
                fused.fc.weight.mul_(8.0)                            # spread the scores over (0, 1)
            for k, v in fused.state_dict().items():
                plain.state_dict()[k].copy_(v)
        mods[name] = {"fused": fused, "torch": plain}
    with torch.no_grad():
        score = mods["gate"]["torch"](x, pts)[:, 0]
    hi = score > 0.9
    assert int(hi.sum()) >= 1000, f"only {int(hi.sum())} rows score above 0.9: rescale the gate's head"
    xs, ps = x[hi].contiguous().requires_grad_(True), pts[hi].contiguous().requires_grad_(True)
    M = int(hi.sum())
    cot = torch.randn(M, 3, device=dev)

    def gate(which):
        with torch.no_grad():
            return mods["gate"][which](x, pts)

    def refine(which):
        m = mods["refine"][which]
        out = m(xs, ps)
        torch.autograd.backward([out], [cot])
        xs.grad = ps.grad = None
        for p_ in m.parameters():
            p_.grad = None

    def window(fn, which):
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            fn(which)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            fn(which)
            b.record()
        torch.cuda.synchronize()
        signal.alarm(0)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        q = statistics.quantiles(ms, n=10)
        return statistics.median(ms), q[0], q[-1]

    per_tile = 2 * D + HD * D + HD + HD * HD + HD + 3 * HD + 3
    min_bytes = {"gate_fwd": 4 * N * (D + 1),
                 "refine_frozen": 4 * M * (D + 3) + 4 * M * (D + 3 + D),
                 "refine_trainable": 4 * M * (D + 3) + 4 * M * (D + 3 + D) + 2 * 4 * (-(-M // 64)) * per_tile}
    lines = [f"vert_mlp timing: N={N} Cf={CF} (D={D}, Hd={HD}), {M} rows above 0.9, {args.warmup} warm-up + {args.iters} timed iterations per "
             f"window, device {torch.cuda.get_device_name(0)}"]
    result = {"N": N, "Cf": CF, "rows_above_0.9": M, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "cases": {}}
    for case, fn in (("gate_fwd", gate), ("refine_frozen", refine), ("refine_trainable", refine)):
        for which in ("fused", "torch"):
            for p_ in mods["refine"][which].parameters():
                p_.requires_grad_(case == "refine_trainable")
        res = {"fused": [], "torch": []}
        for which in ("fused", "torch", "fused", "torch"):
            med, p10, p90 = window(fn, which)
            res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
            lines.append(f"{case:17s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
            print(lines[-1], flush=True)
        f = statistics.mean(w["median_ms"] for w in res["fused"])
        t = statistics.mean(w["median_ms"] for w in res["torch"])
        result["cases"][case] = {"fused_ms": round(f, 4), "torch_ms": round(t, 4), "torch_over_fused": round(t / f, 3),
                                 "fused_windows": res["fused"], "torch_windows": res["torch"],
                                 "fused_window_spread_ms": round(abs(res["fused"][0]["median_ms"] - res["fused"][1]["median_ms"]), 4),
                                 "torch_window_spread_ms": round(abs(res["torch"][0]["median_ms"] - res["torch"][1]["median_ms"]), 4),
                                 "min_bytes": min_bytes[case], "fused_GBps_of_min_bytes": round(min_bytes[case] / f / 1e6, 1)}
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
