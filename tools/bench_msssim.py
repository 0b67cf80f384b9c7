#!/usr/bin/env python3
"""Time of the device MS-SSIM (cdl_msssim_fwd / cdl_msssim_bwd) against the same math composed from torch ops
(depthwise conv2d + avg_pool2d, the restatement in fp32 on the device), alternating in one process, after warm-up, with
device events:

    python tools/bench_msssim.py --reps 20 --warmup 5 [--out profiles/msssim.json] [--parent-lib PATH]

Prints one JSON line per row:
* `ms_ssim` at 64 x 1 x 256 x 256, default arguments (five levels, win 11), data_range 1: median ms of forward and of
  forward + backward (dx only, as a loss uses it) for both paths, their ratio, the agreement of values and gradients;
* with --parent-lib (a libcdlnet_hip.so built from the parent commit): `cdl_ssim_fwd` and `cdl_ssim_fwd` + `cdl_ssim_bwd`
  (dx only) at the same shape through both libraries, alternated call by call: medians, and the spread
  (max - min of five medians of reps/5 calls each) of the parent's own runs;
* the bytes of five levels against the algorithmic count (forward reads x_i, y_i and writes a quarter of each: 10 bytes
  per pixel of level i; reverse, dx only, reads x_i, y_i and a quarter-size gradient and writes dx_i: 13 bytes).  The
  forward count assumes the pooling's second read of x_i, y_i hits the cache; no counter run has shown it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_TBS = 6.3          # what a float4 copy reaches on one MI355X, TB/s
SHAPE = (64, 1, 256, 256)


def torch_ms_ssim(X, Y, weights, win):
    """pytorch_msssim's ms_ssim in torch ops, data_range 1; weights and win are device tensors."""
    import torch
    import torch.nn.functional as F
    C, T = X.shape[1], win.numel()
    wh = win.reshape(1, 1, T, 1).expand(C, 1, T, 1)
    ww = win.reshape(1, 1, 1, T).expand(C, 1, 1, T)

    def f(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)

    C1, C2 = 0.01 ** 2, 0.03 ** 2
    v = []
    L = weights.numel()
    for i in range(L):
        mu1, mu2 = f(X), f(Y)
        s1, s2, s12 = f(X * X) - mu1 * mu1, f(Y * Y) - mu2 * mu2, f(X * Y) - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        if i < L - 1:
            v.append(torch.relu(cs.flatten(2).mean(-1)))
            pad = [X.shape[-2] % 2, X.shape[-1] % 2]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
        else:
            v.append(torch.relu((((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs).flatten(2).mean(-1)))
    return torch.prod(torch.stack(v) ** weights.view(-1, 1, 1), dim=0).mean()


def timed(fns, reps, warmup):
    """fns: {name: fn}; alternates them call by call, the order reversed every other rep so that no form always runs
    behind the same predecessor; {name: [ms]}."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for rep in range(reps):
        for k, fn in (list(fns.items()) if rep % 2 == 0 else list(fns.items())[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def _spread(ms):
    """max - min of the medians of five consecutive chunks: what one library's own runs differ by."""
    n = max(1, len(ms) // 5)
    meds = [statistics.median(ms[i:i + n]) for i in range(0, n * 5, n) if ms[i:i + n]]
    return max(meds) - min(meds)


def ssim_through(lib, x, y, R, win, scratch, n, outs, bwd):
    import torch
    P, H, W = x.shape
    s, g, dx = outs
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731

    def run():
        rc = lib.cdl_ssim_fwd(p(x), p(y), P, H, W, win, 11, 0.01, 0.03, 1.0, p(R), p(s), None, p(scratch), n, st)
        assert rc == 0, rc
        if bwd:
            rc = lib.cdl_ssim_bwd(p(x), p(y), P, H, W, win, 11, 0.01, 0.03, 1.0, p(R), p(g), p(dx), None, None, p(scratch),
                                  n, st)
            assert rc == 0, rc
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    import cdlnet_video_amd as cva
    m = cva.metrics
    rows = []

    x = cva.utils.synthetic_clip(SHAPE, seed=2, waves=3)
    y = (x + torch.randn(x.shape, generator=torch.Generator().manual_seed(1)) * 25 / 255).cuda()
    x = x.cuda()
    weights = list(m.MS_WEIGHTS)
    win = torch.tensor(m._gaussian_window(11, 1.5), device="cuda")
    dev_v = lambda o: m.ms_ssim(o, x, data_range=1.0)               # noqa: E731
    wdev = torch.tensor(weights, device="cuda")
    ref_v = lambda o: torch_ms_ssim(o, x, wdev, win)                # noqa: E731
    yg = y.clone().requires_grad_()

    def fb(fn):
        def run():
            yg.grad = None
            fn(yg).backward()
        return run

    with torch.no_grad():
        t = timed({"hip_fwd": lambda: dev_v(y), "torch_fwd": lambda: ref_v(y)}, a.reps, a.warmup)
    t.update(timed({"hip_fwd_bwd": fb(dev_v), "torch_fwd_bwd": fb(ref_v)}, a.reps, a.warmup))
    r = {"case": "ms_ssim", "shape": list(SHAPE), "levels": len(weights)}
    for k, v in t.items():
        r[k + "_ms"] = round(statistics.median(v), 4)
        r[k + "_ms_min"] = round(min(v), 4)
    r["ratio_torch_over_hip_fwd"] = round(r["torch_fwd_ms"] / r["hip_fwd_ms"], 2)
    r["ratio_torch_over_hip_fwd_bwd"] = round(r["torch_fwd_bwd_ms"] / r["hip_fwd_bwd_ms"], 2)
    sizes = m._level_sizes(SHAPE[2], SHAPE[3], len(weights))
    pix = [SHAPE[0] * SHAPE[1] * h * w for h, w in sizes]
    fwd_bytes = sum(8 * p for p in pix) + sum(8 * p for p in pix[1:])           # read x_i, y_i; write the next level's pair
    bwd_bytes = sum(12 * p for p in pix) + sum(4 * p for p in pix[1:])          # read x_i, y_i, write dx_i; read dx_{i+1}
    r["fwd_bytes"], r["bwd_bytes"] = fwd_bytes, bwd_bytes
    r["fwd_bytes_model_us"] = round(fwd_bytes / (COPY_TBS * 1e12) * 1e6, 2)
    r["bwd_bytes_model_us"] = round(bwd_bytes / (COPY_TBS * 1e12) * 1e6, 2)
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
    assert r["ratio_torch_over_hip_fwd"] > 1 and r["ratio_torch_over_hip_fwd_bwd"] > 1, r
    rows.append(r)
    print(json.dumps(r), flush=True)

    if a.parent_lib:
        this, parent = cva._lib.lib(), ctypes.CDLL(os.path.abspath(a.parent_lib))
        P, H, W = SHAPE[0] * SHAPE[1], SHAPE[2], SHAPE[3]
        for fn in (parent.cdl_ssim_fwd, parent.cdl_ssim_bwd):
            fn.argtypes, fn.restype = cva._lib.SIGNATURES[fn.__name__], ctypes.c_int
        xp, yp = x.reshape(P, H, W), y.reshape(P, H, W)
        R = torch.ones(P, device="cuda")
        n = int(this.cdl_ssim_scratch_floats(P, H, W, 11))
        scratch = torch.empty(n, device="cuda")
        w = m._window_arg(m._gaussian_window(11, 1.5))
        g = torch.full((P,), 1.0 / P, device="cuda")
        res = {}
        for lib_name, lib in (("parent", parent), ("this", this)):
            outs = (torch.empty(P, device="cuda"), g, torch.empty_like(xp))
            res[lib_name] = outs
            for bwd in (False, True):
                res[(lib_name, bwd)] = ssim_through(lib, xp, yp, R, w, scratch, n, outs, bwd)
        r = {"case": "ssim parent vs this", "shape": list(SHAPE)}
        for bwd, key in ((False, "fwd"), (True, "fwd_bwd")):
            t = timed({"parent": res[("parent", bwd)], "this": res[("this", bwd)]}, 5 * a.reps, a.warmup)
            for k, v in t.items():
                r[f"{k}_{key}_ms"] = round(statistics.median(v), 4)
            r[f"parent_{key}_spread_ms"] = round(_spread(t["parent"]), 4)
            r[f"{key}_diff_ms"] = round(r[f"this_{key}_ms"] - r[f"parent_{key}_ms"], 4)
        r["same_bits"] = bool(torch.equal(res["parent"][0], res["this"][0]) and torch.equal(res["parent"][2], res["this"][2]))
        rows.append(r)
        print(json.dumps(r), flush=True)

    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}, f)
            f.write("\n")


if __name__ == "__main__":
    main()
