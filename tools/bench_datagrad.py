#!/usr/bin/env python3
"""Cost of the data gradients: the cfg2 training step (64 x 1 x 256 x 256, K = 30, M = 64, P = 7; forward, MSE,
backward) with and without y.requires_grad_(), alternated in one process after warming both, timed with device events.

    python tools/bench_datagrad.py --steps 10 --warmup 2 [--out profiles/datagrad_cfg2.json]

Prints one JSON line: median ms per step of each form, the overhead, and the spread of the plain step.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--P", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva

    torch.manual_seed(0)
    net = cva.CDLNet(K=a.K, M=a.M, P=a.P, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    gen = torch.Generator().manual_seed(1)
    x = cva.utils.synthetic_clip((a.batch, 1, a.size, a.size), seed=2).cuda()
    sigma = torch.full((a.batch, 1, 1, 1), 25.0, device="cuda")
    y = (x.cpu() + torch.randn(x.shape, generator=gen) * 25 / 255).cuda()

    def step(want_y):
        for p in net.parameters():
            p.grad = None
        yy = y.detach().requires_grad_(want_y)
        xhat, _ = net(yy, sigma)
        torch.mean((xhat - x) ** 2).backward()

    for _ in range(a.warmup):
        step(False)
        step(True)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for i in range(a.steps):
        for want_y in ((False, True) if i % 2 == 0 else (True, False)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            step(want_y)
            t1.record()
            t1.synchronize()
            times[want_y].append(t0.elapsed_time(t1))
    plain, with_y = statistics.median(times[False]), statistics.median(times[True])
    res = {"workload": f"cfg2 train step {a.batch}x1x{a.size}x{a.size} K{a.K} M{a.M} P{a.P}",
           "steps": a.steps, "ms_plain": round(plain, 3), "ms_with_dy": round(with_y, 3),
           "overhead_pct": round(100.0 * (with_y / plain - 1.0), 2),
           "plain_spread_pct": round(100.0 * (max(times[False]) - min(times[False])) / plain, 2),
           "ms_plain_all": [round(t, 3) for t in times[False]], "ms_with_dy_all": [round(t, 3) for t in times[True]]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
