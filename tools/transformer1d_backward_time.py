"""Time a Transformer1D backbone's forward plus its backward to the input on the device at the shipped sizes (in_channels 512, 8 heads
of 64, 10 layers, GEGLU, N = 2 x 32 x 32 = 2048 tokens), B = 1 and B = 8, every weight frozen and x requiring a gradient, as the
one-shot fit runs the texture backbone: the fused pair (the standalone module's forward with grad="input": gh_xf_forward_tape, then
gh_xf_backward through torch.autograd.grad), the plain-torch restatement under autograd (ops="torch": explicit softmax), and the same
statements with F.scaled_dot_product_attention, the three alternating. Then the launch kinds of one layer's backward, each captured
`iters` times in a HIP graph so that the window holds device time alone, with the FLOP the kind needs over that time.

    python tools/transformer1d_backward_time.py [--out profiles/transformer1d_backward_timing.txt] [--repeat 5] [--iters 10]

Times are device events around `iters` calls after a warm-up of every shape; the median and the spread over `repeat` windows are
printed. The derived floor beside them is FLOP / 155 TFLOP/s (the measured rate of v_mfma_f32_32x32x2_f32): a bound, not a
measurement. Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from transformer1d_time import BATCHES, C_IN, D, HEADS, LAYERS, N, PEAK, graphed, make_module, sdpa_forward, stack_flop, timed  # noqa: E402


def backward_flop(B, layers):
    """The backward to x alone: per layer the data products (M M, 3M M, 8M M, twice the first two), the GEGLU's three products of inner
    width M over 4M columns, and per attention five N x N x D products (s, dp, dv, dk, dq; s and dp are formed in both kernels)."""
    T, M = B * N, HEADS * D
    per_layer = 2 * (2 * T * M * M + 2 * T * 3 * M * M) + 2 * T * 8 * M * M + 3 * 2 * T * M * 4 * M + 2 * 7 * 2 * B * HEADS * N * N * D
    return layers * per_layer + 2 * 2 * T * C_IN * M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer1d_backward_timing.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer1d_backward_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import transformer1d as X
    dev = torch.device("cuda:0")
    lines = [f"Transformer1D forward + backward to x, in_channels {C_IN}, {HEADS} heads of {D}, GEGLU, attn2 present, N = {N}, float32, weights frozen, "
             f"{torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the paths alternating; fused = the module's forward with "
             "grad=\"input\" (cached weights and transposes) and torch.autograd.grad;",
             f"floor = FLOP / {PEAK / 1e12:.0f} TFLOP/s, derived, not measured", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spread(ms):
        return f"{statistics.median(ms):9.4f} ms [{min(ms):.4f} .. {max(ms):.4f}]"

    module = make_module(LAYERS, dev).requires_grad_(False)
    p = X.params_of(module)
    for B in BATCHES:
        gen = torch.Generator().manual_seed(B)
        x = torch.randn(B, C_IN, N, generator=gen).to(dev).requires_grad_(True)
        dout = torch.randn(B, C_IN, N, generator=gen).to(dev)
        assert X.kernel_reason(module, x, grad="input") is None
        grad = lambda f: torch.autograd.grad(f(x), x, dout)[0]
        paths = {"fused (gh_xf_forward_tape + gh_xf_backward)": lambda: grad(lambda t: module(t, grad="input")),
                 "restatement (explicit softmax), autograd": lambda: grad(lambda t: X.transformer1d(p, t, ops="torch")),
                 "restatement with SDPA, autograd": lambda: grad(lambda t: sdpa_forward(p, t))}
        outs = {k: f() for k, f in paths.items()}               # warm-up, and the gradients
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(args.repeat):
            for k, f in paths.items():
                ms[k].append(timed(f, args.iters))
        with torch.no_grad():
            fwd = [timed(lambda: module(x), args.iters) for _ in range(args.repeat)]
        flop = stack_flop(B, LAYERS) + backward_flop(B, LAYERS)
        say(f"B = {B}, {LAYERS} layers: forward {stack_flop(B, LAYERS) / 1e9:.1f} + backward {backward_flop(B, LAYERS) / 1e9:.1f} GFLOP, floor {flop / PEAK * 1e3:.3f} ms")
        for k in paths:
            say(f"  {k:46s} {spread(ms[k])}  {flop / statistics.median(ms[k]) / 1e9:7.1f} TFLOP/s")
        say(f"  {'(the untaped fused forward alone, no_grad)':46s} {spread(fwd)}")
        ref = outs["restatement (explicit softmax), autograd"]
        for k in paths:
            if outs[k] is not ref:
                say(f"  max|dx {k} - dx restatement| / max|dx restatement| = {float((outs[k] - ref).abs().max() / ref.abs().max()):.2e}")
        first = list(paths)[0]
        say(f"  fused / restatement = {statistics.median(ms[first]) / statistics.median(ms[list(paths)[1]]):.3f}, "
            f"fused / SDPA = {statistics.median(ms[first]) / statistics.median(ms[list(paths)[2]]):.3f}")
        say()
        del outs

    # ---- the launch kinds of one layer's backward ----
    M = HEADS * D
    blk = p["blocks"][0]
    tr = lambda w: w.t().contiguous()
    wqkv_t = tr(torch.cat([blk["attn1"]["q"], blk["attn1"]["k"], blk["attn1"]["v"]], dim=0))
    o_t, w1_t, w2_t, in_t, out_t = tr(blk["attn1"]["o_w"]), tr(blk["ff1"][0]), tr(blk["ff2"][0]), tr(p["proj_in"][0]), tr(p["proj_out"][0])
    for B in BATCHES:
        T = B * N
        g = torch.Generator().manual_seed(10 + B)
        gh, h, dn, att_g = (torch.randn(T, M, generator=g).to(dev) for _ in range(4))
        qkv, dqkv = torch.randn(T, 3 * M, generator=g).to(dev), torch.randn(T, 3 * M, generator=g).to(dev)
        dadg = torch.randn(T, 8 * M, generator=g).to(dev)
        xin, dcf, dy = (torch.randn(B, C_IN, N, generator=g).to(dev) for _ in range(3))
        mom = torch.stack([h.mean(1), (h.var(1, unbiased=False) + 1e-5).rsqrt()], dim=1)
        gmom = X.group_moments(xin, 32)
        att, lse = X.attention_lse(qkv, B, N, HEADS, D)
        nn2d = 2 * B * HEADS * N * N * D
        zero_bias = torch.zeros(C_IN, device=dev)
        kinds = [
            ("dout rows . W_out, channel first read", 2 * T * C_IN * M, lambda: X.linear(dcf, out_t, prologue="cf")),
            ("GEGLU backward [da | dg]", 3 * 2 * T * M * 4 * M, lambda: X.geglu_backward(gh, h, mom, blk["norm3"][0], blk["norm3"][1], blk["ff1"][0],
                                                                                        blk["ff1"][1], w2_t)),
            ("[da | dg] . W1 (K = 8M)", 2 * T * 8 * M * M, lambda: X.linear(dadg, w1_t)),
            ("LayerNorm backward", 0, lambda: X.layernorm_backward(dn, h, mom, blk["norm3"][0], gh)),
            ("g . W_o (K = M)", 2 * T * M * M, lambda: X.linear(gh, o_t)),
            ("attention forward with lse", 2 * nn2d, lambda: X.attention_lse(qkv, B, N, HEADS, D)),
            ("attention backward (2 launches)", 7 * nn2d, lambda: X.attention_backward(qkv, att, lse, att_g, B, N, HEADS, D)),
            ("dqkv . [Wq; Wk; Wv] (K = 3M)", 2 * T * 3 * M * M, lambda: X.linear(dqkv, wqkv_t)),
            ("g . W_in, written channel first", 2 * T * M * C_IN, lambda: X.linear(gh, in_t, epilogue="bias_res_cf", bias=zero_bias, rows_per_batch=N)),
            ("GroupNorm backward (3 launches)", 0, lambda: X.group_norm_backward(dy, xin, gmom, p["norm"][0], dcf, 32)),
        ]
        say(f"B = {B}: one launch kind at a time, {args.iters} launches per HIP-graph replay")
        with torch.no_grad():
            for name, flop, fn in kinds:
                replay = graphed(fn, args.iters)
                replay()
                torch.cuda.synchronize()
                ms = [timed(replay, 1) / args.iters for _ in range(args.repeat)]
                rate = f"{flop / statistics.median(ms) / 1e9:7.1f} TFLOP/s, floor {flop / PEAK * 1e3:.4f} ms" if flop else ""
                say(f"  {name:40s} {spread(ms)}  {rate}")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
