#!/usr/bin/env python3
"""Time of the blind noise-level estimators on the device: nle_mad, one Gram pass of nle_pca (cdl_nle_pca_gram,
all patches and the weak-texture subset), and the whole nle_pca (both passes plus the host eigenvalue problems and
copies), at 1 x 1 x 256 x 256 and at cfg2's batch 64 x 1 x 256 x 256, after warm-up, with device events.

    python tools/bench_nle.py --reps 20 --warmup 3 [--out profiles/nle_pca.json]

Prints one JSON line per shape: median ms of each, the Gram passes' GFLOP/s (2 x 32 x 32 x K per 32 x 32 output tile,
3 tiles for p = 7, K = every patch) and the fraction of the 157.3 TF fp32 matrix peak.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TF = 157.3


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    nle = cva.nle

    rows = []
    for N in (1, 64):
        H = W = 256
        p = 7
        x = cva.utils.synthetic_clip((N, 1, H, W), seed=2, waves=3)
        y = (x + torch.randn(x.shape, generator=torch.Generator().manual_seed(1)) * 25 / 255).cuda()
        sig = nle.nle_pca(y)[0]
        tau = float(sig) ** 2 * nle.pca_constants(p)[0]
        patches = N * (H - p + 1) * (W - p + 1)
        flop = 3 * 2 * 32 * 32 * patches
        r = {"shape": [N, 1, H, W], "patches": patches, "kept_weak": nle.pca_gram(y, 0, p, tau)[1]}
        for key, fn in (("mad", lambda: nle.nle_mad(y)),
                        ("gram_all", lambda: nle.pca_gram(y, 0, p, math.inf)),
                        ("gram_weak", lambda: nle.pca_gram(y, 0, p, tau)),
                        ("nle_pca", lambda: nle.nle_pca(y))):
            med, lo, hi = timed(fn, a.reps, a.warmup)
            r[key + "_ms"] = round(med, 4)
            r[key + "_ms_range"] = [round(lo, 4), round(hi, 4)]
        for key in ("gram_all", "gram_weak"):
            gf = flop / (r[key + "_ms"] * 1e-3) / 1e9
            r[key + "_gflops"] = round(gf, 1)
            r[key + "_frac_peak"] = round(gf / (PEAK_TF * 1e3), 4)
        r["both_passes_ms"] = round(r["gram_all_ms"] + r["gram_weak_ms"], 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f)
            f.write("\n")


if __name__ == "__main__":
    main()
