"""Time the Gaussian head (guassianhand_amd.gs_head, include/gh_head.h) at the reference's size — P = 98 562 rows, Cin = 128, the RGB
head's O = 14 — next to the torch head it replaces, in the same process:

    fused    gs_head(x, pts, W, b): one launch forward; backward one launch (frozen head) or two (trainable head)
    torch    renderer.gs_activations over five nn.Linear(128, .) — GSLayer.forward as the package ran it before

forward + backward of sum(output * cotangent), x and pts requiring a gradient; "frozen": the five heads' parameters do not (the
one-shot fit, which trains map_bias through the head), "trainable": they do. Device events around every iteration after `--warmup`
(>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows alternating fused / torch / fused / torch; median and
p10 / p90 per window. bytes: what the fused pass must move — forward reads x and pts and writes the five outputs and raw; backward
reads raw and the five cotangents and writes grad_x and grad_pts (the trainable backward reads x again and writes and re-reads its
per-workgroup partials) — over the fused median. Each window runs under an alarm (`--step-timeout` seconds) that ends the process.
Prints one line per window and a summary; `--out FILE` also writes them there (meant for profiles/gs_head_timing.txt).
usage: python tools/bench_gs_head.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import gs_head as H  # noqa: E402
from guassianhand_amd.renderer import gs_activations  # noqa: E402

P, CIN, WIDTH = 98562, 128, 3
O = 11 + WIDTH
KW = dict(use_rgb=True, xyz_offset=True, restrict_offset=True, clip_scaling=None)
FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")


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
    x = torch.randn(P, CIN, generator=g).to(dev).requires_grad_(True)
    pts = (0.1 * torch.randn(P, 3, generator=g)).to(dev).requires_grad_(True)
    layer = H.GSLayer(dict(in_channels=CIN, use_rgb=True, restrict_offset=True)).to(dev)
    with torch.no_grad():
        for lin in layer.out_layers:
            lin.weight.normal_(0, CIN ** -0.5)
    cot = {k: torch.randn(P, n, device=dev) for k, n in zip(FIELDS, (3, 3, 4, 1, WIDTH))}
    cot["shs"] = cot["shs"].reshape(P, WIDTH // 3, 3)

    def fused():
        return layer(x, pts)

    def torch_head():
        raw = {k: lin(x) for k, lin in zip(FIELDS, layer.out_layers)}
        return gs_activations(raw, pts, **KW)

    def head_only(fn):
        """forward + backward of the head alone: the cotangents are handed to autograd directly, no loss kernels are timed"""
        gm = fn()
        torch.autograd.backward([getattr(gm, k) for k in FIELDS], [cot[k] for k in FIELDS])
        x.grad = pts.grad = None
        for p_ in layer.parameters():
            p_.grad = None

    def window(fn):
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            head_only(fn)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            head_only(fn)
            b.record()
        torch.cuda.synchronize()
        signal.alarm(0)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        q = statistics.quantiles(ms, n=10)
        return statistics.median(ms), q[0], q[-1]

    fwd_bytes = 4 * P * (CIN + 3 + 14 + O)
    bwd_bytes = 4 * P * (O + 14 + CIN + 3)
    nblk = -(-P // 64)
    extra = 4 * P * CIN + 2 * 4 * nblk * O * (CIN + 1)
    lines = [f"gs_head timing: P={P} Cin={CIN} O={O}, forward+backward, {args.warmup} warm-up + {args.iters} timed iterations per window, "
             f"device {torch.cuda.get_device_name(0)}"]
    for case in ("frozen", "trainable"):
        for p_ in layer.parameters():
            p_.requires_grad_(case == "trainable")
        res = {"fused": [], "torch": []}
        for name, fn in (("fused", fused), ("torch", torch_head), ("fused", fused), ("torch", torch_head)):
            med, p10, p90 = window(fn)
            res[name].append(med)
            lines.append(f"{case:9s} {name:5s} window {len(res[name])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
            print(lines[-1], flush=True)
        f, t = statistics.mean(res["fused"]), statistics.mean(res["torch"])
        nbytes = fwd_bytes + bwd_bytes + (extra if case == "trainable" else 0)
        lines.append(f"{case:9s} fused {f:.4f} ms vs torch {t:.4f} ms: x{t / f:.2f}; torch windows differ by {abs(res['torch'][0] - res['torch'][1]):.4f} ms, "
                     f"fused by {abs(res['fused'][0] - res['fused'][1]):.4f} ms; fused moves {nbytes / 1e6:.1f} MB -> {nbytes / f / 1e6:.0f} GB/s")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
