#!/usr/bin/env python3
"""Time of the binned noise-level estimate on the device (cdl_nle_nlf_bins: DESIGN.md section 29) against the same
definition composed from device torch ops (conv2d for the two bands, bucketize for the bins, one sort by value and one
stable sort by bin for the medians of all bins), the two alternated in one process, at cfg2's batch 64 x 1 x 256 x 256
and at one 1 x 3 x 1080 x 1920 frame, 32 bins on [0, 1), after warm-up, with device events.  nlf_fit (bins, the MAD
fallback and the batched fit) and nlf_map are timed beside them.

    python tools/bench_nlf.py --rounds 30 --warmup 5 [--out profiles/nlf.json]

Prints one JSON line per shape: median ms of each form, the kernel path's speed-up over the torch composition (below 1:
it loses), and the bytes model with the time those bytes take at the 8 TB/s peak: y read once, the two bands written
once, and per (image, bin) workgroup the key band read by the counting pass plus, when the members are staged in LDS,
only the members' values; otherwise both bands again on each of the three radix passes (mostly from L2 / MALL: every
workgroup of an image reads the same two bands)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
STAGE_MAX = 12288                       # CELL_STAGE_MAX of cdl_nle.hip


def torch_bins(y, hh, box, edges, bins, lo, hi):
    """The definition from device torch ops: (sigma (B, bins), count (B, bins)) for images y (B,C,H,W).  hh, box: the
    10 x 10 diagonal filter and the 7 x 7 mean laid into 10 x 10 taps; edges: the bins + 1 bin edges."""
    import torch
    B, C = y.shape[:2]
    d = torch.nn.functional.conv2d(y, hh.expand(C, 1, 10, 10), stride=2, groups=C).abs().reshape(B, -1)
    m = torch.nn.functional.conv2d(y, box.expand(C, 1, 10, 10), stride=2, groups=C).reshape(B, -1)
    k = torch.bucketize(m, edges, right=True) - 1
    k = torch.where((m >= lo) & (m < hi), k, torch.full_like(k, bins)).clamp_(0, bins)      # outsiders: a bin of their own
    by_value = d.argsort(dim=1)
    by_bin = k.gather(1, by_value).argsort(dim=1, stable=True)
    ranked = d.gather(1, by_value).gather(1, by_bin)                  # bin after bin, each sorted by value
    count = torch.zeros((B, bins + 1), device=y.device, dtype=torch.int64).scatter_add_(1, k, torch.ones_like(k))
    first = count.cumsum(1) - count
    med = ranked.gather(1, (first + (count - 1).clamp(min=0) // 2).clamp(max=d.shape[1] - 1))
    sigma = torch.where(count > 0, med / 0.6745, torch.zeros_like(med))
    return sigma[:, :bins], count[:, :bins]


def model_bytes(B, C, H, W, Hb, Wb, bins):
    band = B * C * Hb * Wb
    staged = C * Hb * Wb <= STAGE_MAX
    select = bins * band * (1 if staged else 7) + (band if staged else 0)
    return 4 * (B * C * H * W + 2 * band + select + 2 * B * bins), staged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    from oracle import cdl_oracle as O
    nle = cva.nle
    bins, lo, hi = a.bins, 0.0, 1.0
    hh = O.hh_filter().cuda()
    box = torch.zeros(1, 1, 10, 10)
    box[:, :, 2:9, 2:9] = 1.0 / 49
    box = box.cuda()
    edges = (lo + torch.arange(bins + 1, dtype=torch.float64) * ((hi - lo) / bins)).float().cuda()

    rows = []
    for shape in ((64, 1, 256, 256), (1, 3, 1080, 1920)):
        x = cva.utils.synthetic_clip(shape, seed=2, waves=3)
        sd = torch.sqrt(0.01 * x + (5 / 255) ** 2)
        y = (x + torch.randn(shape, generator=torch.Generator().manual_seed(1)) * sd).cuda()
        B, C, H, W = shape
        Hb, Wb = nle.band_length(H), nle.band_length(W)
        forms = {"bins_hip": lambda: nle.nlf_bins(y, bins, lo, hi)[:2],
                 "bins_torch": lambda: torch_bins(y, hh, box, edges, bins, lo, hi),
                 "fit_hip": lambda: nle.nlf_fit(y, bins, lo, hi),
                 "map_hip": lambda: nle.nlf_map(y, bins=bins, lo=lo, hi=hi),
                 "global_mad": lambda: nle.nle_mad(y)}
        (s_hip, c_hip), (s_ref, c_ref) = forms["bins_hip"](), forms["bins_torch"]()
        s_hip, c_hip = s_hip.reshape(B, bins), c_hip.reshape(B, bins).long()
        # the two form their bands with different roundings, so a sample within an ulp of an edge may change bins: the
        # counts agree to a few samples and the medians of the well-filled bins to the spacing of the samples around them
        moved = int((c_hip - c_ref).abs().sum())
        full = (c_hip >= 64) & (c_ref >= 64)
        err = float(((s_hip - s_ref).abs() / s_ref.clamp(min=1e-12))[full].max())
        assert moved <= 1e-4 * B * C * Hb * Wb + 2 and err < 1e-2, (moved, err)      # faster and different is not faster
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
        nbytes, staged = model_bytes(B, C, H, W, Hb, Wb, bins)
        r = {"shape": list(shape), "bins": bins, "band": [Hb, Wb], "staged_in_lds": staged, "workgroups": B * bins,
             "samples_moved_vs_torch": moved, "max_rel_err_vs_torch": err}
        for k, v in times.items():
            r[k + "_ms"] = round(statistics.median(v), 4)
            r[k + "_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        r["speedup_bins_hip_over_torch"] = round(r["bins_torch_ms"] / r["bins_hip_ms"], 2)
        r["model_bytes"] = nbytes
        r["model_us_at_peak"] = round(nbytes / (PEAK_TBS * 1e12) * 1e6, 3)
        r["bins_hip_over_model"] = round(r["bins_hip_ms"] * 1e3 / r["model_us_at_peak"], 1)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "rows": rows}, f)
            f.write("\n")


if __name__ == "__main__":
    main()
