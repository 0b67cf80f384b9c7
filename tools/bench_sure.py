#!/usr/bin/env python3
"""Cost of the exact SURE objective (net.jvp) at the cfg2 shape (64 x 1 x 256 x 256, K = 30, M = 64, P = 7): forward +
backward of three objectives and the two forward sweeps alone, alternated in one process after warming all of them,
timed with device events:

    a        supervised: MSE(xhat, x)                                       one forward, one reverse sweep
    b        finite-difference MC-SURE (train.mcsure_loss, h = 1e-3)          two forward, two reverse sweeps
    c        exact SURE (train.sure_loss: the divergence from net.jvp)       two forward, two reverse sweeps
    primal   the primal forward sweep alone (ops.fused_forward, nothing kept)
    tangent  the tangent forward sweep alone (ops.fused_tangent at the primal's bit maps, nothing kept)

    python tools/bench_sure.py --steps 10 --warmup 2 [--out profiles/sure_cfg2.json]

Prints one JSON line: the median ms of each form, the run-to-run spread of b and of the primal sweep measured here, and
the two gates: c no slower than b within b's spread; the tangent sweep within the primal sweep's spread of it.
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
    from cdlnet_video_amd import loop, ops

    torch.manual_seed(0)
    net = cva.CDLNet(K=a.K, M=a.M, P=a.P, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    gen = torch.Generator().manual_seed(1)
    x = cva.utils.synthetic_clip((a.batch, 1, a.size, a.size), seed=2).cuda()
    sigma = torch.full((a.batch, 1, 1, 1), 25.0, device="cuda")
    y = (x.cpu() + torch.randn(x.shape, generator=gen) * 25 / 255).cuda()
    b = torch.randn(x.shape, generator=gen).cuda()

    # the two sweeps alone: the operands of one call of each, prepared once
    yp, _, _, _ = ops.preprocess(y, 1, None)
    bp, _, _, _ = ops.preprocess(b, 1, None)
    g = ops.Geometry.make(a.batch, 1, a.M, yp.shape[2:], (a.P, a.P), (a.P // 2, a.P // 2), 1)
    assert ops.fused_supported(g), "this benchmark times the fused 2-D sweeps"
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    tau = ops.thresholds(net.t.detach(), (sigma.reshape(-1) / 255.0), a.batch)
    maps = ops.fused_forward(g, yp, None, tau, A, B, False, loop.PRECISION, loop.CODE_LAYOUT, keep_maps=True)[4]

    def step(loss_of):
        for p in net.parameters():
            p.grad = None
        loss_of().backward()

    def supervised():
        return torch.mean((net(y, sigma)[0] - x) ** 2)

    def fd():
        return cva.mcsure_loss(net, y, net(y, sigma)[0], sigma, b=b)

    def exact():
        return cva.sure_loss(net, y, sigma, b=b)[0]

    forms = {"a": lambda: step(supervised), "b": lambda: step(fd), "c": lambda: step(exact),
             "primal": lambda: ops.fused_forward(g, yp, None, tau, A, B, False, loop.PRECISION, loop.CODE_LAYOUT),
             "tangent": lambda: ops.fused_tangent(g, bp, None, A, B, maps, False, loop.PRECISION, loop.CODE_LAYOUT)}
    names = list(forms)
    for _ in range(a.warmup):
        for f in names:
            forms[f]()
    torch.cuda.synchronize()
    times = {f: [] for f in names}
    for i in range(a.steps):
        for f in (names if i % 2 == 0 else names[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            forms[f]()
            t1.record()
            t1.synchronize()
            times[f].append(t0.elapsed_time(t1))
    med = {f: statistics.median(t) for f, t in times.items()}
    spread = {f: (max(times[f]) - min(times[f])) / med[f] for f in ("b", "primal")}
    res = {"workload": f"cfg2 {a.batch}x1x{a.size}x{a.size} K{a.K} M{a.M} P{a.P}", "steps": a.steps, "warmup": a.warmup,
           "ms": {f: round(v, 3) for f, v in med.items()},
           "b_spread_pct": round(100.0 * spread["b"], 2), "primal_spread_pct": round(100.0 * spread["primal"], 2),
           "c_over_b_pct": round(100.0 * (med["c"] / med["b"] - 1.0), 2),
           "c_within_b_spread": med["c"] <= med["b"] * (1.0 + spread["b"]),
           "tangent_over_primal_pct": round(100.0 * (med["tangent"] / med["primal"] - 1.0), 2),
           "tangent_within_primal_spread": med["tangent"] <= med["primal"] * (1.0 + spread["primal"]),
           "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
