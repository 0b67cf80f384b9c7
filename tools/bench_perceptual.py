#!/usr/bin/env python3
"""Times `metrics.perceptual_frames` (forward, forward + backward) against the same math composed from torch ops
(F.conv2d / relu / max_pool2d, the same weights), the two alternating in one process after warm-up, device events.
Also one `train_step` of CDLNetVideo at the args3dmri geometry (K=30, M=169, P=[9,9,5], s=2, depth 16; crop 128,
depth 30) with the MSE and with CombinedLossWithSSIM.  Writes profiles/perceptual.json.

    python tools/bench_perceptual.py [--steps 10] [--warmup 3] [--out profiles/perceptual.json] [--no-train]

Kernel times: run it under `rocprofv3 --kernel-trace --stats` (--steps 3 --no-train)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cdlnet_video_amd as cva                                        # noqa: E402

CONVS = (0, 2, 5, 7, 10, 12, 14)
SHAPES = {0: (64, 3), 2: (64, 64), 5: (128, 64), 7: (128, 128), 10: (256, 128), 12: (256, 256), 14: (256, 256)}


def weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in CONVS:
        o, c = SHAPES[i]
        sd[f"{i}.weight"] = torch.randn((o, c, 3, 3), generator=g) * (2.0 / (o * 9)) ** 0.5
        sd[f"{i}.bias"] = torch.randn((o,), generator=g) * 0.05
    return {k: v.cuda() for k, v in sd.items()}


def torch_features(x, sd):
    h = x.repeat(1, 3, 1, 1)
    for i in CONVS:
        h = F.relu(F.conv2d(h, sd[f"{i}.weight"], sd[f"{i}.bias"], padding=1))
        if i in (2, 7):
            h = F.max_pool2d(h, 2, 2)
    return h


def torch_perceptual(o, t, sd):
    B, C, T, H, W = o.shape
    op = o.permute(0, 2, 1, 3, 4).reshape(B * T, 1, H, W)
    tp = t.permute(0, 2, 1, 3, 4).reshape(B * T, 1, H, W)
    return torch.mean((torch_features(op, sd) - torch_features(tp, sd)) ** 2)


def timed(fn, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def bench_shape(shape, sd, steps, warmup):
    g = torch.Generator(device="cuda").manual_seed(1)
    o = torch.rand(shape, device="cuda", generator=g).requires_grad_()
    t = torch.rand(shape, device="cuda", generator=g)

    def dev_f():
        with torch.no_grad():
            cva.metrics.perceptual_frames(o, t, sd)

    def ref_f():
        with torch.no_grad():
            torch_perceptual(o, t, sd)

    def dev_fb():
        o.grad = None
        cva.metrics.perceptual_frames(o, t, sd).backward()

    def ref_fb():
        o.grad = None
        torch_perceptual(o, t, sd).backward()

    for fn in (dev_f, ref_f, dev_fb, ref_fb):
        timed(fn, warmup)
    res = {"dev_fwd": [], "torch_fwd": [], "dev_fwd_bwd": [], "torch_fwd_bwd": []}
    for _ in range(3):                                   # alternate the two paths
        res["dev_fwd"].append(timed(dev_f, steps))
        res["torch_fwd"].append(timed(ref_f, steps))
        res["dev_fwd_bwd"].append(timed(dev_fb, steps))
        res["torch_fwd_bwd"].append(timed(ref_fb, steps))
    out = {k: min(v) for k, v in res.items()}
    out["speedup_fwd"] = out["torch_fwd"] / out["dev_fwd"]
    out["speedup_fwd_bwd"] = out["torch_fwd_bwd"] / out["dev_fwd_bwd"]
    B, C, T, H, W = shape
    flop = 2 * 184896 * B * T * H * W * 3            # F(target) + F(output) + the data backward of F (about one F)
    out["flop_model_tflop"] = flop / 1e12
    out["tflops_fwd_bwd_model"] = flop / (out["dev_fwd_bwd"] * 1e-3) / 1e12
    with torch.no_grad():
        a = float(cva.metrics.perceptual_frames(o, t, sd))
        b = float(torch_perceptual(o, t, sd))
    out["value_rel_diff_vs_torch"] = abs(a - b) / abs(b)
    return out


def bench_train(sd, steps, warmup):
    torch.manual_seed(0)
    net = cva.CDLNetVideo(K=30, M=169, P=[9, 9, 5], s=2, C=1, t0=0, adaptive=True, depth=16, init=True).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=7e-5)
    batch = cva.utils.synthetic_clip((1, 1, 30, 128, 128), seed=1).cuda()
    loss_fn = cva.CombinedLossWithSSIM(1.0, 0.01, 0.1, vgg_weights={k: v.cpu() for k, v in sd.items()}).cuda()
    gen = torch.Generator().manual_seed(2)
    res = {}
    for name, lf in (("mse", None), ("combmse", loss_fn)):
        fn = lambda: cva.train_step(net, opt, batch, (5, 50), clip_grad=1, generator=gen, loss_fn=lf)  # noqa: E731
        timed(fn, warmup)
        res[name] = min(timed(fn, steps) for _ in range(2))
    return {"train_step_ms": res, "geometry": "CDLNetVideo K=30 M=169 P=[9,9,5] s=2 depth=16, batch 1x1x30x128x128"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual.json"))
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    sd = weights()
    report = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "ms": {}}
    for shape in ((1, 1, 30, 128, 128), (64, 1, 1, 256, 256)):
        report["ms"]["x".join(map(str, shape))] = bench_shape(shape, sd, a.steps, a.warmup)
        print(shape, json.dumps(report["ms"]["x".join(map(str, shape))]), flush=True)
    if not a.no_train:
        report["train"] = bench_train(sd, max(2, a.steps // 3), 1)
        print(json.dumps(report["train"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
