"""Time the per-cell pooling (guassianhand_amd.pool, include/gh_pool.h) at the reference's size — T = 98 562 points, 1024 cells —
next to what a user without torch_scatter has today, the plain-torch stand-in in the same run:
    max pool     zeros.scatter_reduce(0, index, x, 'amax', include_self=False) then index_select back to the points
    plane mean   zeros.index_add(0, index, c) / count, transposed
both on (T, C) rows (the reference permutes to (B, C, T) and back around every call; the stand-in is spared that).

Timed: the plan build; one max pool forward and one backward at C = 128; the plane mean forward and backward at C = 512; the whole
encoder (input 53, hidden 128, c_dim 512, plane 32, 5 blocks) forward + backward with the fused ops and with the stand-in ops.
Device events around windows of `--iters` calls after a warm-up of every shape, the median of `--windows` windows, fused and
stand-in windows alternating. Each step runs under an alarm (`--step-timeout` seconds) that ends the process.
bytes/s: the one-read-one-write minimum of the operation (T*C*4 each way for a pool; T*C*4 + C*n_cells*4 for a plane) over the
median time. Prints one JSON line.   usage: python tools/bench_pool.py [--iters 20] [--windows 9] [--step-timeout 120]"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from guassianhand_amd import pool  # noqa: E402
from guassianhand_amd.scenes import make_scene  # noqa: E402

T, N_CELLS, PLANE = 98562, 1024, 32
dev = torch.device("cuda:0")


def standin_pool_max(x, plan):
    idx = plan.index.long()
    cells = x.new_zeros(plan.n_cells, x.shape[1]).scatter_reduce(0, idx.unsqueeze(1).expand(-1, x.shape[1]), x, "amax", include_self=False)
    return cells.index_select(0, idx)


def standin_plane_mean(c, plan):
    idx = plan.index.long()
    cnt = torch.bincount(idx, minlength=plan.n_cells).clamp(min=1).to(c.dtype).unsqueeze(1)
    return (c.new_zeros(plan.n_cells, c.shape[1]).index_add(0, idx, c) / cnt).t()


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, args):
    """{name: median ms per call}: warm-up, then `windows` rounds in which every fn gets one window."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.windows):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    return {k: statistics.median(v) for k, v in times.items()}


def step(name, args, fn):
    signal.alarm(args.step_timeout)
    try:
        return fn()
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()

    def on_alarm(*_):
        sys.stderr.write("bench_pool: a step ran past --step-timeout\n")
        os._exit(3)
    signal.signal(signal.SIGALRM, on_alarm)

    sc = make_scene("two_hands", n_views=1, P=T)
    index = pool.cell_index(sc.xyz[None], 0.2, PLANE)[0].to(dev)
    counts = torch.bincount(index, minlength=N_CELLS)
    g = torch.Generator().manual_seed(0)
    res = {"T": T, "n_cells": N_CELLS, "cells_empty": int((counts == 0).sum()), "cell_max": int(counts.max()), "ops": {}}

    def record(name, t, min_bytes):
        row = {"fused_ms": round(t["fused"], 5)}
        if "standin" in t:
            row["standin_ms"] = round(t["standin"], 5)
            row["speedup"] = round(t["standin"] / t["fused"], 3)
        if min_bytes:
            row["min_bytes"] = min_bytes
            row["fused_GBps"] = round(min_bytes / t["fused"] / 1e6, 1)
        res["ops"][name] = row

    record("plan_build", step("plan", args, lambda: alternate({"fused": lambda: pool.PoolPlan(index, N_CELLS)}, args)), 0)
    plan = pool.PoolPlan(index, N_CELLS)
    plan.check()

    def pool_step():
        C = 128
        x = torch.randn(T, C, generator=g).to(dev).requires_grad_(True)
        cot = torch.randn(T, C, generator=g).to(dev)
        fwd = alternate({"fused": lambda: pool.pool_local(x, plan, "max"), "standin": lambda: standin_pool_max(x, plan)}, args)
        of, os_ = pool.pool_local(x, plan, "max"), standin_pool_max(x, plan)
        assert torch.equal(of, os_)
        bwd = alternate({"fused": lambda: torch.autograd.grad(of, x, cot, retain_graph=True),
                         "standin": lambda: torch.autograd.grad(os_, x, cot, retain_graph=True)}, args)
        record("max_pool_forward_C128", fwd, 2 * T * C * 4)
        record("max_pool_backward_C128", bwd, 2 * T * C * 4)
        xc = x.detach().clone().requires_grad_(True)
        cat = pool.pool_cat(xc, plan, "max")
        cot2 = torch.randn(T, 2 * C, generator=g).to(dev)
        record("max_pool_cat_forward_C128", alternate({"fused": lambda: pool.pool_cat(xc, plan, "max"),
                                                       "standin": lambda: torch.cat([xc, standin_pool_max(xc, plan)], dim=1)}, args), 3 * T * C * 4)
        cs = torch.cat([xc, standin_pool_max(xc, plan)], dim=1)
        record("max_pool_cat_backward_C128", alternate({"fused": lambda: torch.autograd.grad(cat, xc, cot2, retain_graph=True),
                                                        "standin": lambda: torch.autograd.grad(cs, xc, cot2, retain_graph=True)}, args), 3 * T * C * 4)
    step("pool", args, pool_step)

    def plane_step():
        C = 512
        c = torch.randn(T, C, generator=g).to(dev).requires_grad_(True)
        cot = torch.randn(C, N_CELLS, generator=g).to(dev)
        fwd = alternate({"fused": lambda: pool.plane_mean(c, plan), "standin": lambda: standin_plane_mean(c, plan)}, args)
        pf, ps = pool.plane_mean(c, plan), standin_plane_mean(c, plan)
        assert (pf - ps).abs().max().item() < 1e-4
        bwd = alternate({"fused": lambda: torch.autograd.grad(pf, c, cot, retain_graph=True),
                         "standin": lambda: torch.autograd.grad(ps, c, cot, retain_graph=True)}, args)
        record("plane_mean_forward_C512", fwd, T * C * 4 + C * N_CELLS * 4)
        record("plane_mean_backward_C512", bwd, T * C * 4 + C * N_CELLS * 4)
    step("plane", args, plane_step)

    def encoder_step():
        m = pool.LocalPoolPointnet(input_channels=53, c_dim=512, hidden_dim=128, plane_size=PLANE, n_blocks=5, radius=0.2).to(dev)
        p = torch.cat([sc.xyz, torch.randn(T, 50, generator=g)], dim=1)[None].to(dev)
        cot = torch.randn(1, 512, PLANE, PLANE, generator=g).to(dev)

        def run(ops):
            def f():
                m.zero_grad(set_to_none=True)
                m.pool_ops = ops
                pool.pointnet_forward(m, p).backward(cot)
            return f

        # the stand-in encoder: the same module with the restatement's two functions swapped for the lean stand-ins above
        ref_pool, ref_plane = pool._pool_local_ref, pool._plane_mean_ref
        pool._pool_local_ref = lambda x, plan, reduce="max", acc=None: standin_pool_max(x, plan)
        pool._plane_mean_ref = lambda c, plan, acc=None: standin_plane_mean(c, plan)
        try:
            t = alternate({"fused": run("fused"), "standin": run("torch")}, args)
        finally:
            pool._pool_local_ref, pool._plane_mean_ref = ref_pool, ref_plane
        record("encoder_forward_backward", t, 0)
    step("encoder", args, encoder_step)

    print(json.dumps(res))


if __name__ == "__main__":
    main()
