#!/usr/bin/env python3
"""Per-frame noise levels on the fused generic tier against the other three ways to run the cfg3 shape (8 x 1 x 8 x 128 x 128,
K = 20, M = 48, P = 5 x 5 x 5), the forms alternated in one process after warming all of them, timed
with device events, medians:

    a  frame levels, loop.frame_tier_scope("fused")   an (N,1,D,1,1) sigma on k_stage_g, a threshold row per plane
    b  frame levels, the default                      the same sigma expanded to a dense map: the generic three-launch tier
                                                      (launch for launch what the commit before the knob runs)
    c  one level per sample, fused                    the path k_stage_g was built for
    d  one level per sample, generic                  set_backend("generic")

in three rows: forward, training step (forward + backward of an MSE), training step with sigma.requires_grad.

    python tools/bench_frame_levels.py --steps 10 --warmup 2 [--out profiles/frame_levels_cfg3.json]

Prints one JSON line: per row the medians, each form's run-to-run spread (max - min over the median), whether a beats b by
more than b's spread, and a over c with c's spread beside it (the only added work is D times the threshold rows).
--forms bd runs those forms only (b and d exist on the commit before the knob: b can be confirmed there).
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--P", type=int, default=5)
    ap.add_argument("--forms", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import contextlib
    import torch
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop

    torch.manual_seed(0)
    shape = (a.batch, 1, a.depth, a.size, a.size)
    net = cva.CDLNetVideo(K=a.K, M=a.M, P=[a.P] * 3, s=1, C=1, t0=5e-3, adaptive=True, depth=a.depth, init=True).cuda()
    gen = torch.Generator().manual_seed(1)
    x = cva.utils.synthetic_clip(shape, seed=2).cuda()
    per = torch.full((a.batch, 1, 1, 1, 1), 25.0, device="cuda")
    frames = (20.0 + 10.0 * torch.rand((a.batch, 1, a.depth, 1, 1), generator=gen)).cuda()
    y = (x.cpu() + torch.randn(shape, generator=gen) * frames.cpu() / 255).cuda()
    knob = getattr(loop, "frame_tier_scope", None)            # absent on the commit before the knob: forms b and d only
    forms = {"a": ("auto", "fused", frames), "b": ("auto", "generic", frames), "c": ("auto", "generic", per),
             "d": ("generic", "generic", per)}
    forms = {f: v for f, v in forms.items() if f in a.forms}
    if knob is None and "a" in forms:
        raise SystemExit("this commit has no frame tier: run --forms bcd")

    def run(form, backward, want):
        backend, tier, sigma = forms[form]
        loop.set_backend(backend)
        try:
            with (knob(tier) if knob is not None else contextlib.nullcontext()):
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

    res = {"workload": f"cfg3 {'x'.join(str(d) for d in shape)} K{a.K} M{a.M} P{a.P}x{a.P}x{a.P}", "steps": a.steps,
           "forms": {"a": "frame levels, fused", "b": "frame levels, generic (dense map)", "c": "per-sample, fused",
                     "d": "per-sample, generic"},
           "threshold_rows": {"a": a.batch * a.depth, "c": a.batch}}
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
        res[row] = {"ms": {f: round(v, 3) for f, v in med.items()},
                    "spread_pct": {f: round(100.0 * v, 2) for f, v in spread.items()},
                    "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}
        if "a" in med and "b" in med:
            res[row]["b_over_a"] = round(med["b"] / med["a"], 3)
            res[row]["a_beats_b_by_more_than_b_spread"] = med["a"] < med["b"] * (1.0 - spread["b"])
        if "a" in med and "c" in med:
            res[row]["a_over_c_pct"] = round(100.0 * (med["a"] / med["c"] - 1.0), 2)
            res[row]["c_spread_pct"] = round(100.0 * spread["c"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
