#!/usr/bin/env python3
"""Windowed inference against plain net(y) at a user's frame and clip size, the forms alternated
in one process after warming all of them, timed with device events, medians:

    --case flagship   CDLNet K = 30, M = 64, P = 7 on 1 x 1 x 2160 x 4096:
                        plain     net(y)
                        windowed  denoise_windowed, automatic windows, exact halo
    --case video      CDLNetVideo K = 20, M = 48, 5 x 5 x 5 on 1 x 1 x 16 x 1080 x 1920:
                        plain     net(y)
                        windowed  automatic windows, exact halo (the depth stays whole: its exact halo is 80 frames)
                        t2 t4 t8  temporal cores of 4 frames with temporal halos of 2, 4 and 8 frames (8: the whole depth),
                                  spatial halo exact, the largest height core a fused tier then accepts, crop blend; their
                                  PSNR against t8

    python tools/bench_windowed.py --case flagship --steps 10 --warmup 2 [--out profiles/windowed.json]

For each form: median ms, all times, the stage kernels and source files of its launch trace (which tier ran), the plan
and its overhead factor (pixels swept over pixels of the frame).  A form that cannot run at the size records its error
instead of a time.  A form whose single call takes more than --slow seconds is timed over fewer runs (recorded).  The
result is merged into --out under the case's name and printed as one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TIERS = (("cdl_fused2d.hip", "fused 2-D"), ("cdl_strip.hip", "fused generic (strip)"), ("cdl_stripg.hip", "fused generic (stripg)"),
         ("cdl_fusedg.hip", "fused generic (tile)"))


def tier_of(files):
    for f, name in TIERS:
        if f in files:
            return name
    mfma = sorted(f for f in files if f.endswith("_mfma.hip"))
    valu = sorted(f for f in files if f in ("cdl_generic.hip", "cdl_generic_tiled.hip"))
    return "three-launch: " + ", ".join(mfma + valu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["flagship", "video"], required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow", type=float, default=6.0, help="seconds per call above which a form gets fewer runs")
    ap.add_argument("--size", type=int, nargs="+", default=None, help="spatial extents (default: the case's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import windowed as W

    torch.manual_seed(0)
    if a.case == "flagship":
        K, M, P, size = 30, 64, (7, 7), tuple(a.size or (2160, 4096))
        net = cva.CDLNet(K=K, M=M, P=P[0], s=1, C=1, t0=5e-3, adaptive=True, init=True)
    else:
        K, M, P, size = 20, 48, (5, 5, 5), tuple(a.size or (16, 1080, 1920))
        net = cva.CDLNetVideo(K=K, M=M, P=list(P), s=1, C=1, t0=5e-3, adaptive=True, depth=3, init=True)
    net = net.cuda()
    shape = (1, 1) + size
    x = cva.utils.synthetic_clip(shape, seed=2)
    y = (x + torch.randn(shape, generator=torch.Generator().manual_seed(1)) * 25 / 255).cuda()
    del x
    sigma = 25.0
    R = W.exact_halo(K, P, 1)
    accepts = W.fused_accepts(1, M, P, 1)

    forms = {"plain": None, "windowed": dict(window=None, halo="exact")}
    plans = {"windowed": W.plan_windows(size, 1, W.auto_cores(size, 1, R, accepts), R)}
    if a.case == "video":
        for ht in (2, 4, 8):
            halo = (ht,) + R[1:]
            cores = [4, None, None]
            cores[1] = W.largest_core(size, 1, halo, accepts, 1, cores)
            forms[f"t{ht}"] = dict(window=tuple(cores), halo=halo)
            plans[f"t{ht}"] = W.plan_windows(size, 1, cores, halo)

    def run(form):
        with torch.no_grad():
            if forms[form] is None:
                return net(y, sigma)[0]
            return cva.denoise_windowed(net, y, sigma, **forms[form])

    res = {"workload": f"{a.case} 1x1x{'x'.join(map(str, size))} K{K} M{M} P{'x'.join(map(str, P))}", "steps": a.steps,
           "warmup": a.warmup, "whole_sample_accepted_by_a_fused_tier": bool(accepts(size)), "forms": {}}
    outs, steps = {}, {}
    for form in list(forms):                           # first call of each form: its trace, its result, its cost
        entry = {"plan": plans[form].describe()} if form in plans else {}
        t0 = time.time()
        try:
            with cva.ops.trace() as t:
                out = run(form)
                torch.cuda.synchronize()
        except (torch.cuda.OutOfMemoryError, cva.HipKernelError, NotImplementedError, ValueError) as e:
            entry["error"] = f"{type(e).__name__}: {e}"
            del forms[form]
            res["forms"][form] = entry
            continue
        first = time.time() - t0
        entry.update(tier=tier_of(t.files()), files=sorted(t.files()), launches=len(t), first_call_s=round(first, 2))
        steps[form] = a.steps if first <= a.slow else max(2, min(a.steps, int(60.0 / first)))
        outs[form] = out.cpu()
        res["forms"][form] = entry
        print(f"# {form}: first call {first:.2f} s, tier {entry['tier']}", flush=True)
    for form in forms:
        for _ in range(max(0, a.warmup - 1)):          # the first call was a warm-up too
            run(form)
    torch.cuda.synchronize()
    times = {f: [] for f in forms}
    names = list(forms)
    for i in range(a.steps):
        for f in (names if i % 2 == 0 else names[::-1]):
            if len(times[f]) >= steps[f]:
                continue
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run(f)
            t1.record()
            t1.synchronize()
            times[f].append(t0.elapsed_time(t1))
        print(f"# round {i + 1}/{a.steps}", flush=True)
    for f in forms:
        e = res["forms"][f]
        e.update(ms=round(statistics.median(times[f]), 3), runs=len(times[f]), all_ms=[round(v, 3) for v in times[f]])
    ref = "plain" if "plain" in outs else "windowed"
    for f, out in outs.items():
        e = res["forms"][f]
        if f != ref:
            e[f"rel_err_vs_{ref}"] = float((out - outs[ref]).abs().max() / outs[ref].abs().max())
            if "ms" in res["forms"].get("plain", {}):
                e["plain_over_this"] = round(res["forms"]["plain"]["ms"] / e["ms"], 3)
        if a.case == "video" and f in ("t2", "t4") and "t8" in outs:
            e["psnr_vs_t8_db"] = round(cva.psnr(outs["t8"], out), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged[a.case] = res
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
