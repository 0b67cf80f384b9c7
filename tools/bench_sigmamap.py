#!/usr/bin/env python3
"""Cost of a noise-level map at the cfg2 shape (64 x 1 x 256 x 256, K = 30, M = 64, P = 7), forward and forward + backward
(MSE), the four forms alternated in one process after warming all of them, timed with device events:

    a  set_backend("generic"), one sigma per sample          the baseline (the kernels a map call runs, without the map)
    b  the same with a full (N,1,H,W) map
    c  b with sigma.requires_grad                             (adds the channel-reduction kernel cdl_sigma_grad)
    d  the default fused path, one sigma per sample           what a map call gives up today

    python tools/bench_sigmamap.py --steps 10 --warmup 2 [--out profiles/sigmamap_cfg2.json]

Prints one JSON line: median ms of each form, the gate for b -- a times (1 + the map's byte share 4/(8M) + the run-to-run
spread of a measured here) -- and whether b is within it.
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
    from cdlnet_video_amd import loop

    torch.manual_seed(0)
    net = cva.CDLNet(K=a.K, M=a.M, P=a.P, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    gen = torch.Generator().manual_seed(1)
    x = cva.utils.synthetic_clip((a.batch, 1, a.size, a.size), seed=2).cuda()
    per = torch.full((a.batch, 1, 1, 1), 25.0, device="cuda")
    amap = (20.0 + 10.0 * torch.rand((a.batch, 1, a.size, a.size), generator=gen)).cuda()
    y = (x.cpu() + torch.randn(x.shape, generator=gen) * 25 / 255).cuda()
    forms = {"a": ("generic", per, False), "b": ("generic", amap, False), "c": ("generic", amap, True),
             "d": ("auto", per, False)}

    def run(form, backward):
        backend, sigma, want = forms[form]
        loop.set_backend(backend)
        try:
            if not backward:
                with torch.no_grad():
                    net(y, sigma)
                return
            for p in net.parameters():
                p.grad = None
            xhat, _ = net(y, sigma.detach().requires_grad_(want))
            torch.mean((xhat - x) ** 2).backward()
        finally:
            loop.set_backend("auto")

    res = {"workload": f"cfg2 {a.batch}x1x{a.size}x{a.size} K{a.K} M{a.M} P{a.P}", "steps": a.steps,
           "byte_share_pct": round(100.0 * 4 / (8 * a.M), 3)}
    for mode, backward in (("fwd", False), ("fwd_bwd", True)):
        names = [f for f in forms if backward or f != "c"]          # c differs from b in the backward only
        for _ in range(a.warmup):
            for f in names:
                run(f, backward)
        torch.cuda.synchronize()
        times = {f: [] for f in names}
        for i in range(a.steps):
            order = names if i % 2 == 0 else names[::-1]
            for f in order:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(f, backward)
                t1.record()
                t1.synchronize()
                times[f].append(t0.elapsed_time(t1))
        med = {f: statistics.median(t) for f, t in times.items()}
        spread = (max(times["a"]) - min(times["a"])) / med["a"]
        gate = med["a"] * (1.0 + 4 / (8 * a.M) + spread)
        res[mode] = {"ms": {f: round(v, 3) for f, v in med.items()},
                     "a_spread_pct": round(100.0 * spread, 2), "b_gate_ms": round(gate, 3),
                     "b_over_a_pct": round(100.0 * (med["b"] / med["a"] - 1.0), 2), "b_within_gate": med["b"] <= gate,
                     "b_over_d": round(med["b"] / med["d"], 3),
                     "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}
        if backward:
            res[mode]["c_over_b_pct"] = round(100.0 * (med["c"] / med["b"] - 1.0), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
