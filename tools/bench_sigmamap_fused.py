#!/usr/bin/env python3
"""The fused map route against the other three ways to run the cfg2 shape (64 x 1 x 256 x 256, K = 30, M = 64, P = 7;
DESIGN.md section 31), the forms alternated in one process after warming all of them, timed with device events, medians:

    a  the fused map route       loop.map_tier_scope("fused"), a full (N,1,H,W) map
    b  the generic map route     the default for a map
    c  the fused per-sample route (one sigma per sample: the flagship path)
    d  the generic per-sample route (set_backend("generic"))

in three rows: forward, training step (forward + backward of an MSE), training step with sigma.requires_grad.

    python tools/bench_sigmamap_fused.py --steps 10 --warmup 2 [--out profiles/sigmamap_fused_cfg2.json]

Prints one JSON line: per row the medians, each form's run-to-run spread (max - min over the median), whether a beats b by
more than b's spread, and a's excess over c beyond the map's byte share 4/(8M) plus c's spread.
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
    ap.add_argument("--only", default=None, help="run this one form, timings only: for a kernel trace of the form on its own")
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
    forms = {"a": ("auto", "fused", amap), "b": ("auto", "generic", amap), "c": ("auto", "generic", per),
             "d": ("generic", "generic", per)}
    if a.only:
        forms = {a.only: forms[a.only]}

    def run(form, backward, want):
        backend, tier, sigma = forms[form]
        loop.set_backend(backend)
        try:
            with loop.map_tier_scope(tier):
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

    share = 4 / (8 * a.M)
    res = {"workload": f"cfg2 {a.batch}x1x{a.size}x{a.size} K{a.K} M{a.M} P{a.P}", "steps": a.steps,
           "forms": {"a": "fused map", "b": "generic map", "c": "fused per-sample", "d": "generic per-sample"},
           "byte_share_pct": round(100.0 * share, 3)}
    for row, backward, want in (("fwd", False, False), ("step", True, False), ("step_sigma_grad", True, True)):
        for _ in range(a.warmup):
            for f in forms:
                run(f, backward, want)
        torch.cuda.synchronize()
        times = {f: [] for f in forms}
        for i in range(a.steps):
            order = list(forms) if i % 2 == 0 else list(forms)[::-1]
            for f in order:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(f, backward, want)
                t1.record()
                t1.synchronize()
                times[f].append(t0.elapsed_time(t1))
        med = {f: statistics.median(t) for f, t in times.items()}
        spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
        if a.only:
            res[row] = {"ms": {f: round(v, 3) for f, v in med.items()}}
            continue
        res[row] = {"ms": {f: round(v, 3) for f, v in med.items()},
                    "spread_pct": {f: round(100.0 * v, 2) for f, v in spread.items()},
                    "a_under_b_pct": round(100.0 * (1.0 - med["a"] / med["b"]), 2),
                    "a_beats_b_by_more_than_b_spread": med["a"] < med["b"] * (1.0 - spread["b"]),
                    "a_over_c_pct": round(100.0 * (med["a"] / med["c"] - 1.0), 2),
                    "a_excess_over_c_pct": round(100.0 * (med["a"] / med["c"] - 1.0 - share - spread["c"]), 2),
                    "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
