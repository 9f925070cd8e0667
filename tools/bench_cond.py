"""Time the point conditioning (guassianhand_amd.cond, include/gh_cond.h) at the reference's size — N = 98 562 points, one batch
element — next to the reference's statements in TGS._forward (infer_one_shot.py:241-274), in eval() mode, in the same process:

    addfeat_fwd          additional_features: the (N, 852) concatenation + additional_features_fc(852, 51), no gradient
    addfeat_fwd_bwd      the same, forward + backward to identity_code_vert (everything else frozen)
    shade_fc_pos_fwd     the shade encoder's first layer: Linear(1587, 256) over its concatenation, no gradient
    texture_fc_pos       the texture encoder's first layer: Linear(53, 256), forward + backward to the code and to the layer

    fused    cond.additional_features / PointRows.linear: the rows from gh_cond_rows or built in LDS, the broadcast columns folded
    torch    SpatialEncoder's statements, torch.cat with pose_feats.repeat(1, N, 1), the module / the nn.Linear

Device events around every iteration after `--warmup` (>= 5) untimed ones; `--iters` (>= 20) timed iterations per window, windows
alternating fused / torch / fused / torch; median, p10 and p90 per window. Each window runs under an alarm (`--step-timeout`
seconds) that ends the process. Prints one line per window and ONE JSON line at the end; `--out FILE` also writes them there (meant
for profiles/cond_timing.txt).
usage: python tools/bench_cond.py [--iters 20] [--warmup 5] [--step-timeout 120] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import cond  # noqa: E402

N, CC, DE, HD = 98562, 33, 768, 51


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
    uv = torch.rand(1, N, 2, generator=g).to(dev)
    xyz = (0.1 * torch.randn(1, N, 3, generator=g)).to(dev)
    flag = (torch.rand(1, N, 1, generator=g) < 0.4).to(dev)
    code = (2 * torch.rand(1, N, CC, generator=g) - 1).to(dev).requires_grad_(True)
    pose, cam = torch.randn(1, 1, DE, generator=g).to(dev), torch.randn(1, 1, DE, generator=g).to(dev)
    torch.manual_seed(0)
    fc = cond.AdditionalFeaturesFC(84 + DE, HD).to(dev).eval()
    with torch.no_grad():
        fc.ff1.layer_norm.weight.add_(0.3 * torch.randn(84 + DE, device=dev))
        fc.ff1.layer_norm.bias.add_(0.2 * torch.randn(84 + DE, device=dev))
    for p_ in fc.parameters():
        p_.requires_grad_(False)
    shade_fc, texture_fc = torch.nn.Linear(51 + 2 * DE, 256).to(dev), torch.nn.Linear(53, 256).to(dev)
    for p_ in shade_fc.parameters():
        p_.requires_grad_(False)
    cot_a, cot_t = torch.randn(1, N, HD, device=dev), torch.randn(1, N, 256, device=dev)

    def addfeat(which):
        if which == "fused":
            return cond.additional_features(fc, uv, xyz, flag, code, pose)
        feats = torch.cat([uv, cond.spatial_encode(uv, 4), xyz, cond.spatial_encode(xyz, 4), flag, code, pose.repeat(1, N, 1)], dim=-1)
        return fc(feats)

    def addfeat_fwd(which):
        with torch.no_grad():
            addfeat(which)

    def addfeat_fwd_bwd(which):
        torch.autograd.backward([addfeat(which)], [cot_a])
        code.grad = None

    def shade(which):
        with torch.no_grad():
            rows = cond.PointRows(uv=uv, xyz=xyz, flag=flag, broadcast=(pose, cam))
            return rows.linear(shade_fc) if which == "fused" else shade_fc(rows.dense())

    def texture(which):
        rows = cond.PointRows(uv=uv, code=code)
        out = rows.linear(texture_fc) if which == "fused" else texture_fc(rows.dense())
        torch.autograd.backward([out], [cot_t])
        code.grad = None
        for p_ in texture_fc.parameters():
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

    dense_bytes = {"addfeat_fwd": 4 * N * (84 + DE), "addfeat_fwd_bwd": 4 * N * (84 + DE), "shade_fc_pos_fwd": 4 * N * (51 + 2 * DE),
                   "texture_fc_pos": 4 * N * 53}
    lines = [f"cond timing: N={N} B=1 Cc={CC} De={DE} Hd={HD} levels=4, {args.warmup} warm-up + {args.iters} timed iterations per window, "
             f"device {torch.cuda.get_device_name(0)}"]
    result = {"N": N, "B": 1, "Cc": CC, "De": DE, "Hd": HD, "iters": args.iters, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "cases": {}}
    for case, fn in (("addfeat_fwd", addfeat_fwd), ("addfeat_fwd_bwd", addfeat_fwd_bwd), ("shade_fc_pos_fwd", shade), ("texture_fc_pos", texture)):
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
                                 "concatenation_bytes_not_written": dense_bytes[case]}
    lines.append(json.dumps(result))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    signal.signal(signal.SIGALRM, lambda *_: os._exit(124))
    main()
