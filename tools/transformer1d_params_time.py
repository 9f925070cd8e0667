"""Time a Transformer1D backbone's forward plus its backward to the input and to its parameters on the device at the shipped sizes
(in_channels 512, 8 heads of 64, 10 layers with attn2, GEGLU, N = 2 x 32 x 32 = 2048 tokens), B = 1 and B = 8, in two settings: every
parameter and x requiring a gradient, and only the last two layers trainable (x still requiring one). Three paths alternate: the fused
pair (the standalone module's forward with grad="params": gh_xf_forward_tape, then gh_xf_backward_params through torch.autograd.grad;
the cached stacked and transposed weights are rebuilt before every call, as after an optimiser step, and that cost is inside the
window), and what the same call does without the mode — torch's own statements under autograd with the explicit softmax, and with
F.scaled_dot_product_attention. Then the launch kinds one layer's backward adds for the parameters beside the data products of the
same layer, each captured `iters` times in a HIP graph so that the window holds device time alone.

    python tools/transformer1d_params_time.py [--out profiles/transformer1d_params_timing.txt] [--repeat 5] [--iters 5]
    python tools/transformer1d_params_time.py --trace 1        # three steps at B = 1 and nothing else: the run to put under a kernel trace

Times are device events around `iters` calls after a warm-up of every shape; the median and the spread over `repeat` windows are
printed. Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from transformer1d_time import BATCHES, C_IN, D, HEADS, LAYERS, N, PEAK, graphed, make_module, sdpa_forward, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer1d_params_timing.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, help="run three fused steps at this batch size and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer1d_params_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import transformer1d as X
    dev = torch.device("cuda:0")
    module = make_module(LAYERS, dev)
    p = X.params_of(module)

    def setting(which):
        module.requires_grad_(which == "all")
        if which == "last two":
            for b in module.transformer_blocks[-2:]:
                b.requires_grad_(True)
        return [t for t in module.parameters() if t.requires_grad]

    def step_of(f, x, dout, ps):
        return lambda: torch.autograd.grad(f(x), [x, *ps], dout)

    def fused(t):
        X.refresh(module)                                        # an optimiser step has moved the weights: the copies are rebuilt
        return module(t, grad="params")

    if args.trace:
        B = args.trace
        gen = torch.Generator().manual_seed(B)
        x = torch.randn(B, C_IN, N, generator=gen).to(dev).requires_grad_(True)
        dout = torch.randn(B, C_IN, N, generator=gen).to(dev)
        ps = setting("all")
        for _ in range(3):
            step_of(fused, x, dout, ps)()
        torch.cuda.synchronize()
        return

    lines = [f"Transformer1D forward + backward to x and the parameters, in_channels {C_IN}, {HEADS} heads of {D}, GEGLU, attn2 present, N = {N}, float32, "
             f"{torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the paths alternating; fused = the module's forward with "
             "grad=\"params\" and torch.autograd.grad, the cached weight copies rebuilt before every call", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spread(ms):
        return f"{statistics.median(ms):9.4f} ms [{min(ms):.4f} .. {max(ms):.4f}]"

    for B in BATCHES:
        gen = torch.Generator().manual_seed(B)
        x = torch.randn(B, C_IN, N, generator=gen).to(dev).requires_grad_(True)
        dout = torch.randn(B, C_IN, N, generator=gen).to(dev)
        for which in ("all", "last two"):
            ps = setting(which)
            assert X.kernel_reason(module, x, grad="params") is None
            paths = {"fused (gh_xf_forward_tape + gh_xf_backward_params)": step_of(fused, x, dout, ps),
                     "restatement (explicit softmax), autograd": step_of(lambda t: X.transformer1d(p, t, ops="torch"), x, dout, ps),
                     "restatement with SDPA, autograd": step_of(lambda t: sdpa_forward(p, t), x, dout, ps)}
            outs = {k: f() for k, f in paths.items()}           # warm-up, and the gradients
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            for _ in range(args.repeat):
                for k, f in paths.items():
                    ms[k].append(timed(f, args.iters))
            say(f"B = {B}, {LAYERS} layers, trainable: {which} ({len(ps)} tensors) and x")
            for k in paths:
                say(f"  {k:52s} {spread(ms[k])}")
            ref = outs["restatement (explicit softmax), autograd"]
            worst = max(float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for a, b in zip(outs[list(paths)[0]], ref))
            say(f"  worst max|g fused - g restatement| / max|g restatement| over the {len(ref)} gradients = {worst:.2e}")
            first, second, third = list(paths)
            say(f"  fused / restatement = {statistics.median(ms[first]) / statistics.median(ms[second]):.3f}, "
                f"fused / SDPA = {statistics.median(ms[first]) / statistics.median(ms[third]):.3f}")
            say()
            del outs

    # ---- what one layer's backward adds for the parameters, beside the data products of the same layer ----
    module.requires_grad_(False)
    M = HEADS * D
    blk = p["blocks"][0]
    tr = lambda w: w.t().contiguous()
    wqkv_t = tr(torch.cat([blk["attn1"]["q"], blk["attn1"]["k"], blk["attn1"]["v"]], dim=0))
    o_t, w1_t = tr(blk["attn1"]["o_w"]), tr(blk["ff1"][0])
    for B in BATCHES:
        T = B * N
        g = torch.Generator().manual_seed(10 + B)
        gh, h, dn, att = (torch.randn(T, M, generator=g).to(dev) for _ in range(4))
        dqkv, dadg, ff = (torch.randn(T, w, generator=g).to(dev) for w in (3 * M, 8 * M, 4 * M))
        mom = torch.stack([h.mean(1), (h.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)
        ln = dict(prologue="ln", gamma=blk["norm3"][0], beta=blk["norm3"][1], moments=mom)
        kinds = [
            ("data  g . W_o (K = M)", 2 * T * M * M, (M, M), lambda: X.linear(gh, o_t)),
            ("param g^T . att -> (M, M), db", 2 * T * M * M, (M, M), lambda: X.linear_wgrad(gh, att)),
            ("data  dqkv . [Wq; Wk; Wv] (K = 3M)", 2 * T * 3 * M * M, (M, 3 * M), lambda: X.linear(dqkv, wqkv_t)),
            ("param dqkv^T . LN(h) -> (3M, M)", 2 * T * 3 * M * M, (M, 3 * M), lambda: X.linear_wgrad(dqkv, h, want_b=False, **ln)),
            ("data  [da | dg] . W1 (K = 8M)", 2 * T * 8 * M * M, (M, 8 * M), lambda: X.linear(dadg, w1_t)),
            ("param [da | dg]^T . LN3(h) -> (8M, M), db", 2 * T * 8 * M * M, (M, 8 * M), lambda: X.linear_wgrad(dadg, h, **ln)),
            ("param g^T . a gelu(g) -> (M, 4M), db", 2 * T * 4 * M * M, (4 * M, M), lambda: X.linear_wgrad(gh, ff)),
            ("param a gelu(g) again (LN + GEGLU forward)", 2 * T * 8 * M * M, None,
             lambda: X.linear(h, blk["ff1"][0], prologue="ln", epilogue="geglu", bias=blk["ff1"][1], gamma=blk["norm3"][0], beta=blk["norm3"][1])),
            ("param LayerNorm dgamma, dbeta (2 launches)", 0, None, lambda: X.layernorm_param_grads(dn, h, mom)),
        ]
        say(f"B = {B}: one launch kind at a time, {args.iters} launches per HIP-graph replay")
        with torch.no_grad():
            for name, flop, shape, fn in kinds:
                replay = graphed(fn, args.iters)
                replay()
                torch.cuda.synchronize()
                ms = [timed(replay, 1) / args.iters for _ in range(args.repeat)]
                rate = f"{flop / statistics.median(ms) / 1e9:7.1f} TFLOP/s, floor {flop / PEAK * 1e3:.4f} ms" if flop else ""
                split = ""
                if name.startswith("param") and shape is not None:
                    c = X.linear_wgrad_chunk(T, *shape)
                    split = f"  T split into {(T + c - 1) // c} chunk(s) of {c}"
                say(f"  {name:44s} {spread(ms)}  {rate}{split}")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
