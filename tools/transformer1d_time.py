"""Time a Transformer1D backbone's forward on the device at the shipped sizes (in_channels 512, 8 heads of 64, 10 layers, GEGLU,
N = 2 x 32 x 32 = 2048 tokens), B = 1 and B = 8, under torch.no_grad(): the fused stack (the standalone module's forward, which
holds its contiguous weights and the stacked [Wq; Wk; Wv] per module as the config seam's class does: one gh_xf_forward call), the
plain-torch restatement (ops="torch": explicit softmax), and the same statements with F.scaled_dot_product_attention, the
three alternating. Then the launch kinds of one layer, each captured `iters` times in a HIP graph so that the window holds device time
alone, with the FLOP the kind needs (2 T K N_out for a product, 4 B heads N^2 D for the attention) over that time.

    python tools/transformer1d_time.py [--out profiles/transformer1d_timing.txt] [--repeat 5] [--iters 10]

Times are device events around `iters` calls after a warm-up of every shape; the median and the spread over `repeat` windows are
printed. The derived floor beside them is FLOP / 155 TFLOP/s (the measured rate of v_mfma_f32_32x32x2_f32): a bound, not a
measurement. Without a ROCm device the tool fails: it has nothing to estimate from."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_IN, HEADS, D, LAYERS, N = 512, 8, 64, 10, 2048
BATCHES = (1, 8)
PEAK = 155e12


def make_module(layers, dev, seed=0):
    """transformer1d.Transformer1D at the shipped sizes with weights ~ N(0, 1 / K), biases ~ 0.1 N(0, 1), norm scales ~ 1."""
    from guassianhand_amd.transformer1d import Transformer1D
    g = torch.Generator().manual_seed(seed)
    m = Transformer1D(C_IN, HEADS, D, layers, cross_attention_dim=HEADS * D)
    with torch.no_grad():
        for name, t in m.named_parameters():
            r = torch.randn(t.shape, generator=g)
            t.copy_(r * t.shape[1] ** -0.5 if t.dim() == 2 else (1 + 0.1 * r if "norm" in name and name.endswith("weight") else 0.1 * r))
    return m.to(dev).eval()


def sdpa_forward(p, x):
    """transformer1d_ref's statements with F.scaled_dot_product_attention in place of the explicit softmax."""
    heads = p["heads"]
    B, Cc, n = x.shape
    h = F.linear(F.group_norm(x, p["groups"], *p["norm"], eps=p["gn_eps"]).permute(0, 2, 1).reshape(B, n, Cc), *p["proj_in"])
    M = h.shape[-1]
    split = lambda t: t.reshape(B, n, heads, M // heads).transpose(1, 2)
    for b in p["blocks"]:
        for nk, ak in (("norm1", "attn1"), ("norm2", "attn2")):
            a = b[ak]
            y = F.layer_norm(h, (M,), *b[nk], eps=b["ln_eps"])
            o = F.scaled_dot_product_attention(split(F.linear(y, a["q"])), split(F.linear(y, a["k"])), split(F.linear(y, a["v"])))
            h = h + F.linear(o.transpose(1, 2).reshape(B, n, M), a["o_w"], a["o_b"])
        v, gate = F.linear(F.layer_norm(h, (M,), *b["norm3"], eps=b["ln_eps"]), *b["ff1"]).chunk(2, dim=-1)
        h = h + F.linear(v * F.gelu(gate), *b["ff2"])
    return F.linear(h, *p["proj_out"]).reshape(B, n, Cc).permute(0, 2, 1).contiguous() + x


def stack_flop(B, layers):
    T, M = B * N, HEADS * D
    per_layer = 2 * T * M * (3 * M + M) * 2 + 2 * T * M * 8 * M + 2 * T * 4 * M * M + 2 * 4 * B * HEADS * N * N * D
    return layers * per_layer + 2 * 2 * T * C_IN * M


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def graphed(fn, iters):
    """fn captured `iters` times in one graph: a replay is `iters` launches with no host work between them."""
    fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer1d_timing.txt"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer1d_time: no ROCm device; nothing is measured and nothing is estimated")
    from guassianhand_amd import transformer1d as X
    dev = torch.device("cuda:0")
    lines = [f"Transformer1D forward, in_channels {C_IN}, {HEADS} heads of {D}, GEGLU, attn2 present, N = {N}, float32, no_grad, {torch.cuda.get_device_name(0)}",
             f"device events around {args.iters} calls, median [min .. max] of {args.repeat} windows, the paths alternating; fused = the module's forward (cached weights);",
             f"floor = FLOP / {PEAK / 1e12:.0f} TFLOP/s, derived, not measured", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spread(ms):
        return f"{statistics.median(ms):9.4f} ms [{min(ms):.4f} .. {max(ms):.4f}]"

    module = make_module(LAYERS, dev)
    p = X.params_of(module)
    for B in BATCHES:
        x = torch.randn(B, C_IN, N, generator=torch.Generator().manual_seed(B)).to(dev)
        with torch.no_grad():
            assert X.kernel_reason(module, x) is None
            paths = {"fused (gh_xf_forward)": lambda: module(x), "restatement (explicit softmax)": lambda: X.transformer1d(p, x, ops="torch"),
                     "restatement with SDPA": lambda: sdpa_forward(p, x)}
            outs = {k: f() for k, f in paths.items()}           # warm-up, and the outputs
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            for _ in range(args.repeat):
                for k, f in paths.items():
                    ms[k].append(timed(f, args.iters))
        flop = stack_flop(B, LAYERS)
        say(f"B = {B}, {LAYERS} layers: {flop / 1e9:.1f} GFLOP, floor {flop / PEAK * 1e3:.3f} ms")
        for k in paths:
            say(f"  {k:32s} {spread(ms[k])}  {flop / statistics.median(ms[k]) / 1e9:7.1f} TFLOP/s")
        ref = outs["restatement (explicit softmax)"]
        for k in ("fused (gh_xf_forward)", "restatement with SDPA"):
            say(f"  max|{k} - restatement| / max|restatement| = {float((outs[k] - ref).abs().max() / ref.abs().max()):.2e}")
        say()
        del outs

    # ---- the launch kinds of one layer ----
    M = HEADS * D
    blk = p["blocks"][0]
    wqkv = torch.cat([blk["attn1"]["q"], blk["attn1"]["k"], blk["attn1"]["v"]], dim=0)
    for B in BATCHES:
        T = B * N
        g = torch.Generator().manual_seed(10 + B)
        h, att, ff = (torch.randn(T, w, generator=g).to(dev) for w in (M, M, 4 * M))
        qkv = torch.randn(T, 3 * M, generator=g).to(dev)
        xin = torch.randn(B, C_IN, N, generator=g).to(dev)
        mom = X.group_moments(xin, 32)
        kinds = [
            ("group moments (2 launches)", 0, lambda: X.group_moments(xin, 32)),
            ("GN . proj_in + bias", 2 * T * C_IN * M, lambda: X.linear(xin, p["proj_in"][0], prologue="gn", epilogue="bias_res", bias=p["proj_in"][1],
                                                                      gamma=p["norm"][0], beta=p["norm"][1], eps=1e-6, groups=32, moments=mom)),
            ("LN moments + LN . [Wq;Wk;Wv]", 2 * T * M * 3 * M, lambda: X.linear(h, wqkv, prologue="ln", gamma=blk["norm1"][0], beta=blk["norm1"][1])),
            ("attention", 4 * B * HEADS * N * N * D, lambda: X.attention(qkv, B, N, HEADS, D)),
            ("to_out + bias + residual", 2 * T * M * M, lambda: X.linear(att, blk["attn1"]["o_w"], epilogue="bias_res", bias=blk["attn1"]["o_b"], res=h)),
            ("LN moments + LN . W1, GEGLU", 2 * T * M * 8 * M, lambda: X.linear(h, blk["ff1"][0], prologue="ln", epilogue="geglu", bias=blk["ff1"][1],
                                                                               gamma=blk["norm3"][0], beta=blk["norm3"][1])),
            ("W2 + bias + residual", 2 * T * 4 * M * M, lambda: X.linear(ff, blk["ff2"][0], epilogue="bias_res", bias=blk["ff2"][1], res=h)),
            ("proj_out + bias + x, channel first", 2 * T * M * C_IN, lambda: X.linear(h, p["proj_out"][0], epilogue="bias_res_cf", bias=p["proj_out"][1],
                                                                                      res=xin, rows_per_batch=N)),
        ]
        say(f"B = {B}: one launch kind at a time, {args.iters} launches per HIP-graph replay")
        with torch.no_grad():
            for name, flop, fn in kinds:
                replay = graphed(fn, args.iters)
                replay()
                torch.cuda.synchronize()
                ms = [timed(replay, 1) / args.iters for _ in range(args.repeat)]
                rate = f"{flop / statistics.median(ms) / 1e9:7.1f} TFLOP/s, floor {flop / PEAK * 1e3:.4f} ms" if flop else ""
                say(f"  {name:36s} {spread(ms)}  {rate}")
        say()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
