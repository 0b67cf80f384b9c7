#!/usr/bin/env python3
"""Time of the device SSIM (cdl_ssim_fwd / cdl_ssim_bwd) against the same math composed from torch ops (depthwise
conv2d along H then W, as pytorch_msssim builds it), alternating in one process, after warm-up, with device events:

* `ssim` at 64 x 1 x 256 x 256 (pytorch_msssim defaults, data_range 1);
* `ssim_frames` on the frames of cfg3's clip, 8 x 1 x 8 x 128 x 128 (the reference's default data_range).

    python tools/bench_ssim.py --reps 20 --warmup 5 [--out profiles/ssim.json] [--only-device]

Prints one JSON line per shape: median ms of forward and forward + backward (dx only, as a loss uses it) for both
paths, their ratio, the agreement of values and gradients, and the kernel time against the bytes model (forward
reads x and y, 8 bytes per pixel; backward reads x and y and writes dx, 12).  --only-device skips the torch path
(for a kernel-trace run of its own).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_TBS = 6.3          # what a float4 copy reaches on one MI355X, TB/s


def torch_ssim_per_plane(X, Y, R, win):
    """(N, C, H, W), R (N, C) -> (N, C) mean SSIM: pytorch_msssim's _ssim in torch ops."""
    import torch.nn.functional as F
    C, T = X.shape[1], win.numel()
    wh = win.reshape(1, 1, T, 1).expand(C, 1, T, 1)
    ww = win.reshape(1, 1, 1, T).expand(C, 1, 1, T)

    def f(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)

    C1 = ((0.01 * R) ** 2)[..., None, None]
    C2 = ((0.03 * R) ** 2)[..., None, None]
    mu1, mu2 = f(X), f(Y)
    s1, s2, s12 = f(X * X) - mu1 * mu1, f(Y * Y) - mu2 * mu2, f(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs).flatten(2).mean(-1)


def torch_ssim(X, Y):
    import torch
    import cdlnet_video_amd as cva
    win = torch.tensor(cva.metrics._gaussian_window(11, 1.5), device=X.device)
    R = torch.ones(X.shape[:2], device=X.device)
    return torch_ssim_per_plane(X, Y, R, win).mean()


def torch_ssim_frames(o, t):
    import torch
    import cdlnet_video_amd as cva
    N, C, D, H, W = o.shape
    win = torch.tensor(cva.metrics._gaussian_window(11, 1.5), device=o.device)
    R_t = o.amax(dim=(0, 1, 3, 4)) - o.amin(dim=(0, 1, 3, 4))
    X = o.permute(0, 2, 1, 3, 4).reshape(N * D, C, H, W)
    Y = t.permute(0, 2, 1, 3, 4).reshape(N * D, C, H, W)
    R = R_t.repeat(N)[:, None].expand(N * D, C)
    per = torch_ssim_per_plane(X, Y, R, win).reshape(N, D, C).mean(dim=(0, 2))
    return (1 - per).mean()


def timed_pair(fns, reps, warmup):
    """fns: {name: fn}; alternates them rep by rep; median / min ms of each."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-device", action="store_true")
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    m = cva.metrics

    cases = [("ssim", (64, 1, 256, 256), m.ssim, torch_ssim),
             ("ssim_frames", (8, 1, 8, 128, 128), m.ssim_frames, torch_ssim_frames)]
    rows = []
    for name, shape, dev_fn, ref_fn in cases:
        x = cva.utils.synthetic_clip(shape, seed=2, waves=3)
        y = (x + torch.randn(x.shape, generator=torch.Generator().manual_seed(1)) * 25 / 255).cuda()
        x = x.cuda()
        if name == "ssim":
            dev_v = lambda o: dev_fn(o, x, data_range=1.0)          # noqa: E731
        else:
            dev_v = lambda o: dev_fn(o, x)                            # noqa: E731
        ref_v = lambda o: ref_fn(o, x)                                # noqa: E731
        yg = y.clone().requires_grad_()

        def fb(fn):
            def run():
                yg.grad = None
                fn(yg).backward()
            return run

        fns = {"hip_fwd": lambda: dev_v(y), "hip_fwd_bwd": fb(dev_v)}
        if not a.only_device:
            fns.update({"torch_fwd": lambda: ref_v(y), "torch_fwd_bwd": fb(ref_v)})
        with torch.no_grad():
            t = timed_pair({k: v for k, v in fns.items() if k.endswith("_fwd")}, a.reps, a.warmup)
        t.update(timed_pair({k: v for k, v in fns.items() if k.endswith("_bwd")}, a.reps, a.warmup))
        pix = x.numel()
        r = {"case": name, "shape": list(shape), "planes": pix // (shape[-1] * shape[-2])}
        for k, (med, lo) in t.items():
            r[k + "_ms"] = round(med, 4)
            r[k + "_ms_min"] = round(lo, 4)
        r["fwd_bytes_model_us"] = round(8 * pix / (COPY_TBS * 1e12) * 1e6, 2)
        r["bwd_bytes_model_us"] = round(12 * pix / (COPY_TBS * 1e12) * 1e6, 2)
        if not a.only_device:
            r["ratio_torch_over_hip_fwd"] = round(r["torch_fwd_ms"] / r["hip_fwd_ms"], 2)
            r["ratio_torch_over_hip_fwd_bwd"] = round(r["torch_fwd_bwd_ms"] / r["hip_fwd_bwd_ms"], 2)
            yg.grad = None
            vh = dev_v(yg)
            vh.backward()
            gh = yg.grad.clone()
            yg.grad = None
            vt = ref_v(yg)
            vt.backward()
            r["value_hip"], r["value_torch"] = float(vh), float(vt)
            r["value_abs_diff"] = float((vh - vt).abs())
            r["grad_rel_diff"] = float((gh - yg.grad).abs().max() / yg.grad.abs().max())
            assert r["value_abs_diff"] < 1e-4 and r["grad_rel_diff"] < 1e-3, r
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}, f)
            f.write("\n")


if __name__ == "__main__":
    main()
