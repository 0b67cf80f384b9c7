#!/usr/bin/env python3
"""Time of the local MAD noise-level estimate on the device (cdl_nle_mad_cells: DESIGN.md section 19) against the same
definition composed from device torch ops (conv2d, unfold, index_select, median), the two alternated in one process,
and against nle_mad on the same batch; at cfg2's batch 64 x 1 x 256 x 256 and at cfg3's frames 8 x 1 x 8 x 128 x 128,
window 32, step 16, after warm-up, with device events.

    python tools/bench_nle_map.py --rounds 30 --warmup 5 [--out profiles/nle_map.json]

Prints one JSON line per shape: median ms of each form, the kernel path's speed-up over the torch composition, and the
bytes model (y read once, the band written once at a quarter of y's size and read once per cell that covers a sample,
four times at most with step = window / 2) with the time those bytes take at the 8 TB/s peak.  Kernel times come
from a separate kernel-trace run of this script (--rounds 5 under the profiler)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TBS = 8.0


def torch_cells(y, hh, sy, sx, window):
    """The definition from device torch ops: (B, ny, nx) for images y (B,C,H,W); sy, sx the cells' first samples
    (device index tensors, built once outside the timed region)."""
    import torch
    B, C = y.shape[:2]
    band = torch.nn.functional.conv2d(y, hh.expand(C, 1, 10, 10), stride=2, groups=C).abs()
    Hb, Wb = band.shape[2:]
    rows = band.unfold(2, min(window, Hb), 1).index_select(2, sy)               # (B, C, ny, Wb, h)
    win = rows.unfold(3, min(window, Wb), 1).index_select(3, sx)                # (B, C, ny, nx, h, w)
    flat = win.permute(0, 2, 3, 1, 4, 5).reshape(B, sy.numel(), sx.numel(), -1)
    return flat.median(dim=-1)[0] / 0.6745


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    from oracle import cdl_oracle as O
    nle = cva.nle
    w, q = a.window, a.window // 2
    hh = O.hh_filter().cuda()

    rows = []
    for shape in ((64, 1, 256, 256), (8, 1, 8, 128, 128)):
        x = cva.utils.synthetic_clip(shape, seed=2, waves=3)
        y = (x + torch.randn(shape, generator=torch.Generator().manual_seed(1)) * 25 / 255).cuda()
        imgs = y if y.dim() == 4 else y.transpose(1, 2).reshape((-1, shape[1]) + shape[3:]).contiguous()
        B, C, H, W = imgs.shape
        Hb, Wb = nle.band_length(H), nle.band_length(W)
        sy, sx = nle.cell_starts(Hb, w, q), nle.cell_starts(Wb, w, q)
        dev_sy, dev_sx = torch.tensor(sy).cuda(), torch.tensor(sx).cuda()
        forms = {"cells_hip": lambda: nle.nle_mad_cells(y, w, q),
                 "cells_torch": lambda: torch_cells(imgs, hh, dev_sy, dev_sx, w),
                 "map_hip": lambda: nle.nle_mad_map(y, w, q),
                 "global_mad": lambda: nle.nle_mad(imgs)}
        if y.dim() == 5:
            forms["frames_hip"] = lambda: nle.nle_mad_frames(y)
        got, ref = forms["cells_hip"]().reshape(B, -1), forms["cells_torch"]().reshape(B, -1)
        err = float(((got - ref).abs() / ref).max())
        assert err < 1e-5, err                      # faster and different is not faster
        for _ in range(a.warmup):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.rounds):                   # the forms alternate within every round
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        cell_reads = B * C * len(sy) * len(sx) * min(w, Hb) * min(w, Wb)
        nbytes = 4 * (B * C * H * W + B * C * Hb * Wb + cell_reads + B * len(sy) * len(sx))
        r = {"shape": list(shape), "window": w, "step": q, "cells": [len(sy), len(sx)], "max_rel_err_vs_torch": err}
        for k, v in times.items():
            r[k + "_ms"] = round(statistics.median(v), 4)
            r[k + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        r["speedup_cells_hip_over_torch"] = round(r["cells_torch_ms"] / r["cells_hip_ms"], 2)
        r["model_bytes"] = nbytes
        r["model_us_at_peak"] = round(nbytes / (PEAK_TBS * 1e12) * 1e6, 3)
        r["cells_hip_over_model"] = round(r["cells_hip_ms"] * 1e3 / r["model_us_at_peak"], 1)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "rows": rows}, f)
            f.write("\n")


if __name__ == "__main__":
    main()
