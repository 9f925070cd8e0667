"""Time the point encoders' ResNet blocks (guassianhand_amd.res_block, include/gh_res.h) at the reference's size — T = 98 562 points,
hidden width 128, 1024 cells populated as the bench scene's two hands populate them — next to the statements they replace, in the same
process:

    rows_fwd           the row kernel alone: res_rows over net (T,128) with ready (1025,128) tables, no gradient
    block_fwd          one block 1..4: the two table GEMMs over the 1025 cell rows, then res_rows; no gradient
    block_fwd_bwd      the same, forward + backward to net (tables and weights frozen)
    block0_fwd_bwd     block 0: res_rows over the (T,256) rows with one table row, forward + backward
    texture_encoder    LocalPoolPointnet(53 -> 128) over PointRows(uv, code): forward + backward to the code, parameters frozen
    shade_encoder      LocalPoolPointnet(1587 -> 128) over PointRows(uv, xyz, flag, two broadcast vectors): forward + backward to the
                       broadcast vectors, parameters frozen

    fused    the row kernels / blocks="folded"
    torch    ResnetBlockFC over the materialised (T,256) concatenation / blocks="torch" (the pooling kernels with torch's blocks)

Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows
alternating fused / torch / fused / torch; median, p10 and p90 per window. Each window runs under an alarm (`--step-timeout` seconds)
that ends the process. The row kernel's FLOP/s are 2 T H (2 Cin + H) per forward (as many again per backward) over the fused median,
against the 157.3 TFLOP/s float32 matrix peak. Prints one line per window and ONE JSON line at the end; `--out FILE` also writes them
there (meant for profiles/res_block_timing.txt).
usage: python tools/bench_res_block.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import cond, pool, res_block  # noqa: E402
from guassianhand_amd.scenes import make_scene  # noqa: E402

T, H, PLANE, RADIUS, DE, CC = 98562, 128, 32, 0.2, 768, 33
PEAK = 157.3e12


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
    sc = make_scene("two_hands", n_views=1, P=T)
    uv = (sc.xyz[None, :, :2] / RADIUS).contiguous().to(dev)               # the encoders clamp to their radius of 1
    xyz = sc.xyz[None].contiguous().to(dev)
    flag = (torch.rand(1, T, 1, generator=g) < 0.4).to(dev)
    code = (2 * torch.rand(1, T, CC, generator=g) - 1).to(dev).requires_grad_(True)
    pose, cam = (torch.randn(1, 1, DE, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    plan = pool.PoolPlan(pool.cell_index(uv, 1.0, PLANE)[0], PLANE * PLANE)
    counts = plan.counts()
    row_of = res_block.row_index(plan)

    torch.manual_seed(0)
    block = pool.ResnetBlockFC(2 * H, H).to(dev)
    torch.nn.init.normal_(block.fc_1.weight, std=H ** -0.5)
    encoders = {"texture_encoder": pool.LocalPoolPointnet(input_channels=20 + CC, hidden_dim=H, c_dim=H, plane_size=PLANE).to(dev),
                "shade_encoder": pool.LocalPoolPointnet(input_channels=51 + 2 * DE, hidden_dim=H, c_dim=H, plane_size=PLANE).to(dev)}
    for m in (block, *encoders.values()):
        for q in m.parameters():
            q.requires_grad_(False)
    for m in encoders.values():
        for b in m.blocks:
            torch.nn.init.normal_(b.fc_1.weight, std=H ** -0.5)
    net = torch.randn(T, H, generator=g).to(dev).requires_grad_(True)
    x0 = torch.randn(T, 2 * H, generator=g).to(dev).requires_grad_(True)
    cells = torch.cat([torch.randn(PLANE * PLANE, H, generator=g), torch.zeros(1, H)]).to(dev)
    cot, cot_plane = torch.randn(T, H, generator=g).to(dev), torch.randn(1, H, PLANE, PLANE, generator=g).to(dev)

    def one_block(which, x, m):
        if which == "fused":
            return res_block.folded_block(block, x, m, row_of if m is not None else None, plan=plan if m is not None else None)
        return block(x if m is None else torch.cat([x, m.index_select(0, row_of.long())], dim=1))

    with torch.no_grad():
        u_tab = torch.nn.functional.linear(torch.relu(cells), block.fc_0.weight[:, H:], block.fc_0.bias)
        s_tab = torch.nn.functional.linear(cells, block.shortcut.weight[:, H:], block.fc_1.bias)

    def rows_fwd(which):
        with torch.no_grad():
            if which == "fused":
                res_block.res_rows(net, u_tab, s_tab, row_of, block.fc_0.weight[:, :H], block.shortcut.weight[:, :H], block.fc_1.weight, plan=plan)
            else:
                one_block(which, net, cells)

    def block_fwd(which):
        with torch.no_grad():
            one_block(which, net, cells)

    def block_fwd_bwd(which):
        torch.autograd.backward([one_block(which, net, cells)], [cot])
        net.grad = None

    def block0_fwd_bwd(which):
        torch.autograd.backward([one_block(which, x0, None)], [cot])
        x0.grad = None

    def encoder(name):
        m = encoders[name]

        def run(which):
            rows = cond.PointRows(uv=uv, code=code) if name == "texture_encoder" else cond.PointRows(uv=uv, xyz=xyz, flag=flag, broadcast=(pose, cam))
            plane = pool.pointnet_forward(m, rows, blocks="folded" if which == "fused" else "torch")
            torch.autograd.backward([plane], [cot_plane])
            code.grad = pose.grad = cam.grad = None
        return run

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

    fwd_flop = lambda cin: 2.0 * T * H * (2 * cin + H)
    kernel_flop = {"rows_fwd": fwd_flop(H), "block_fwd": fwd_flop(H), "block_fwd_bwd": 2 * fwd_flop(H), "block0_fwd_bwd": 2 * fwd_flop(2 * H)}
    lines = [f"res block timing: T={T} H={H} cells={PLANE * PLANE} (empty {int((counts == 0).sum())}, largest {int(counts.max())}, without a cell "
             f"{T - int(counts.sum())}), {args.warmup} warm-up + {args.iters} timed iterations per window, device {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    result = {"T": T, "H": H, "n_cells": PLANE * PLANE, "cells_empty": int((counts == 0).sum()), "cell_max": int(counts.max()),
              "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": {}}
    for case, fn in (("rows_fwd", rows_fwd), ("block_fwd", block_fwd), ("block_fwd_bwd", block_fwd_bwd), ("block0_fwd_bwd", block0_fwd_bwd),
                     ("texture_encoder", encoder("texture_encoder")), ("shade_encoder", encoder("shade_encoder"))):
        res = {"fused": [], "torch": []}
        for which in ("fused", "torch", "fused", "torch"):
            med, p10, p90 = window(fn, which)
            res[which].append({"median_ms": round(med, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4)})
            lines.append(f"{case:16s} {which:5s} window {len(res[which])}: median {med:.4f} ms  p10 {p10:.4f}  p90 {p90:.4f}")
            print(lines[-1], flush=True)
        f = statistics.mean(w["median_ms"] for w in res["fused"])
        t = statistics.mean(w["median_ms"] for w in res["torch"])
        entry = {"fused_ms": round(f, 4), "torch_ms": round(t, 4), "torch_over_fused": round(t / f, 3),
                 "fused_windows": res["fused"], "torch_windows": res["torch"],
                 "fused_window_spread_ms": round(abs(res["fused"][0]["median_ms"] - res["fused"][1]["median_ms"]), 4),
                 "torch_window_spread_ms": round(abs(res["torch"][0]["median_ms"] - res["torch"][1]["median_ms"]), 4)}
        if case in kernel_flop:
            entry["row_kernel_tflops"] = round(kernel_flop[case] / (f * 1e-3) / 1e12, 2)
            entry["row_kernel_fraction_of_f32_matrix_peak"] = round(kernel_flop[case] / (f * 1e-3) / PEAK, 3)
        result["cases"][case] = entry
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
