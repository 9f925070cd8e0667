"""Time forward_gs — the trunk MLP and the Gaussian head (guassianhand_amd.gs_trunk, include/gh_trunk.h) — at the reference's sizes,
P = 98 562 and 197 124 rows (the valid set, and the valid set with its refined copies), Cin = 131, H = Cout = 128, the RGB head's
O = 14 and the SH head's O = 59, next to the two torch forms it replaces, in the same process:

    fused        gs_trunk(x, pts, trunk, W, b): one launch forward, one backward (which recomputes the hidden layers)
    torch+head   TrunkMLP in torch (three GEMMs, two SiLU launches), then gs_head's fused head — forward_gs as the package ran it before
    torch+lin    TrunkMLP in torch, then renderer.gs_activations over five nn.Linear — the reference's own statements

"fwd": the forward alone under torch.no_grad(); "fwd+bwd": forward and backward with the cotangents handed to autograd directly, x
and pts requiring a gradient and every weight frozen (the one-shot fit). Device events around every iteration after `--warmup`
(>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, the three forms alternating, two windows each; median and
p10 / p90 per window, and per form the spread between its two windows. FLOP/s: 2 * (Cin H + H H + H Cout + Cout O) per row for a
forward and the same again for the backward's four products (what any implementation must do), over the fused time, as a share of
the 155 TF float32-matrix peak; the fused backward additionally executes the two recomputed products. Each window runs under an alarm
(`--step-timeout` seconds) that ends the process. There is no fall-back: without a ROCm device the tool fails.
Prints one line per window and a summary per configuration; `--out FILE` also writes them there (meant for profiles/gs_trunk_timing.txt).
usage: python tools/bench_gs_trunk.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import gs_head as H  # noqa: E402
from guassianhand_amd import gs_trunk as T  # noqa: E402
from guassianhand_amd.renderer import gs_activations  # noqa: E402

SIZES = (98562, 197124)
CIN, HID, COUT = 131, 128, 128
PEAK = 155e12
FIELDS = ("xyz", "scaling", "rotation", "opacity", "shs")
FORMS = ("fused", "torch+head", "torch+lin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.iters, args.warmup = max(args.iters, 20), max(args.warmup, 5)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gs_trunk: no ROCm device — the kernels have no fall-back")
    dev = torch.device("cuda:0")
    lines = [f"gs_trunk timing: Cin={CIN} H={HID} Cout={COUT}, silu, frozen weights, {args.warmup} warm-up + {args.iters} timed iterations per "
             f"window, device {torch.cuda.get_device_name(0)}"]

    def window(step):
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            step()
            b.record()
        torch.cuda.synchronize()
        signal.alarm(0)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        q = statistics.quantiles(ms, n=10)
        return statistics.median(ms), q[0], q[-1]

    for P in SIZES:
        for use_rgb in (True, False):
            width = 3 if use_rgb else 48
            O = 11 + width
            kw = dict(use_rgb=use_rgb, xyz_offset=True, restrict_offset=True, clip_scaling=None)
            g = torch.Generator().manual_seed(0)
            x = torch.randn(P, CIN, generator=g).to(dev).requires_grad_(True)
            pts = (0.1 * torch.randn(P, 3, generator=g)).to(dev).requires_grad_(True)
            torch.manual_seed(0)
            mlp = T.TrunkMLP(CIN, COUT, HID, 2, "silu").to(dev).requires_grad_(False)
            head = H.GSLayer(dict(in_channels=COUT, use_rgb=use_rgb, restrict_offset=True)).to(dev)
            with torch.no_grad():
                for lin in head.out_layers:
                    lin.weight.normal_(0, COUT ** -0.5)
            head.requires_grad_(False)
            trunk = [t for i in (0, 2, 4) for t in (mlp.layers[i].weight, mlp.layers[i].bias)]
            W, b = torch.cat([l.weight for l in head.out_layers]), torch.cat([l.bias for l in head.out_layers])
            cot = [torch.randn(P, n, device=dev) for n in (3, 3, 4, 1, width)]
            cot[4] = cot[4].reshape(P, width // 3, 3)

            def torch_lin(y):
                return gs_activations({k: lin(y) for k, lin in zip(FIELDS, head.out_layers)}, pts, **kw)

            forms = {"fused": lambda: T.gs_trunk(x, pts, trunk, W, b, shs_width=width, activation="silu", **kw),
                     "torch+head": lambda: head(mlp(x), pts), "torch+lin": lambda: torch_lin(mlp(x))}

            def forward_only(fn):
                with torch.no_grad():
                    fn()

            def both(fn):
                gm = fn()
                torch.autograd.backward([getattr(gm, k) for k in FIELDS], cot)
                x.grad = pts.grad = None

            flop = 2.0 * P * (CIN * HID + HID * HID + HID * COUT + COUT * O)
            for mode, step, work in (("fwd", forward_only, flop), ("fwd+bwd", both, 2 * flop)):
                res = {name: [] for name in FORMS}
                for name in FORMS + FORMS:
                    med, p10, p90 = window(lambda: step(forms[name]))
                    res[name].append(med)
                    lines.append(f"P={P} O={O} {mode:7s} {name:10s} window {len(res[name])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
                    print(lines[-1], flush=True)
                mean = {name: statistics.mean(v) for name, v in res.items()}
                spread = {name: abs(v[0] - v[1]) for name, v in res.items()}
                f = mean["fused"]
                lines.append(f"P={P} O={O} {mode:7s} fused {f:.4f} ms (windows differ by {spread['fused']:.4f}) vs torch+head {mean['torch+head']:.4f} "
                             f"(by {spread['torch+head']:.4f}): x{mean['torch+head'] / f:.2f}; vs torch+lin {mean['torch+lin']:.4f} (by "
                             f"{spread['torch+lin']:.4f}): x{mean['torch+lin'] / f:.2f}; fused {work / f / 1e9:.1f} TFLOP/s = "
                             f"{100 * work / (f * 1e-3) / PEAK:.1f}% of the 155 TF float32-matrix peak")
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
