#!/usr/bin/env python3
"""Time of the windowed weak-texture PCA noise-level map (cva.nle.nle_pca_map: DESIGN.md section 25) on one
1080 x 1920 frame, window 64 / step 32 (33 x 59 cells), patchsize 7, itr 3, against the only way to the same numbers
without the cell form -- a Python loop of nle_pca over the contiguous crops, timed on one row of 59 crops and scaled
by the 33 rows -- and against nle_mad_map on the same frame; plus the parts of the call: one Gram pass over all cells
and one batched float64 eigvalsh on the device and on the host.

    python tools/bench_nle_pca_map.py [--rounds 5] [--out FILE]

Wall clock around each call with a device synchronisation, after one warm-up call; every repetition is listed and the
median quoted.  Prints one JSON object."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def frame(H, W, seed=0):
    """A clean image with smooth and sharp structure plus noise whose level ramps from 5/255 to 25/255 across the
    width: (1, 1, H, W) float32."""
    import torch
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    clean = (0.5 + 0.25 * torch.sin(2 * math.pi * (r / 37 + c / 53))
             + 0.15 * torch.sign(torch.sin(2 * math.pi * c / 29 + r / 11)))
    ramp = torch.linspace(5.0, 25.0, W, dtype=torch.float64) / 255
    noise = torch.randn(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return (clean + noise * ramp).float()[None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    nle = cva.nle
    H, W = a.size
    w, q, p = a.window, a.window // 2, 7
    y = frame(H, W).cuda()
    ys, xs = nle.cell_starts(H, w, q), nle.cell_starts(W, w, q)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.rounds):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return ts

    tau = torch.full((1, len(ys), len(xs)), math.inf, device="cuda")
    gram, cnt = nle.pca_gram_cells(y, 0, p, w, q, tau)
    cov = gram / (cnt - 1)[..., None, None]
    host = torch.linalg.eigvalsh(cov.cpu())[..., 0]
    dev = torch.linalg.eigvalsh(cov)[..., 0]
    out = {"frame": [H, W], "window": w, "step": q, "patchsize": p, "itr": 3, "cells": [len(ys), len(xs)],
           "rounds": a.rounds, "s": {}}
    s = out["s"]
    s["nle_pca_map"] = timed(lambda: nle.nle_pca_map(y, w, q))
    s["gram_pass_all_cells"] = timed(lambda: nle.pca_gram_cells(y, 0, p, w, q, tau))
    s["eigvalsh_device"] = timed(lambda: torch.linalg.eigvalsh(cov)[..., 0])
    s["eigvalsh_host_with_copies"] = timed(lambda: torch.linalg.eigvalsh(cov.cpu())[..., 0].cuda())
    s["nle_pca_loop_one_row_of_crops"] = timed(
        lambda: [nle.nle_pca(y[:, :, 0:min(w, H), x0:x0 + min(w, W)].contiguous())[0] for x0 in xs])
    s["nle_mad_map"] = timed(lambda: nle.nle_mad_map(y))
    med = {k: statistics.median(v) for k, v in s.items()}
    out["median_s"] = med
    out["nle_pca_loop_all_rows_s"] = len(ys) * med["nle_pca_loop_one_row_of_crops"]
    out["crop_loop_over_nle_pca_map"] = out["nle_pca_loop_all_rows_s"] / med["nle_pca_map"]
    out["nle_pca_map_over_nle_mad_map"] = med["nle_pca_map"] / med["nle_mad_map"]
    out["eigvalsh_device_vs_host_max_rel"] = float(((dev.cpu() - host).abs() / host.abs()).max())
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
