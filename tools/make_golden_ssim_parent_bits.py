#!/usr/bin/env python3
"""Bits of `ssim` and `ssim_frames` (values and input gradients) on fixed inputs, recorded on the commit BEFORE the
MS-SSIM entry points share the SSIM kernels:

    python tools/make_golden_ssim_parent_bits.py tests/golden/ms0_ssim_parent_bits.npz      # on that commit, on the device

tests/test_gpu_msssim.py calls `compute()` on the current commit and compares bit for bit.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [((2, 3, 37, 53), 11, 2), ((3, 1, 71, 130), 7, 1)]          # (N, C, H, W), win of `ssim`, D of the clip


def _images(cva, shape, seed):
    import torch
    x = cva.utils.synthetic_clip(shape, seed=seed)
    y = x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 100))
    return x, y


def compute():
    """{name: numpy array} of every recorded quantity."""
    import torch
    import cdlnet_video_amd as cva
    out = {}
    for i, (shape, win, D) in enumerate(CASES):
        x, y = _images(cva, shape, seed=61 + i)
        w = torch.rand(shape[0], generator=torch.Generator().manual_seed(5)) + 0.5
        xd, yd, rd = x.cuda().requires_grad_(), y.cuda().requires_grad_(), torch.tensor(1.2).cuda().requires_grad_()
        v = cva.metrics.ssim(xd, yd, data_range=rd, win_size=win, size_average=False)
        (v * w.cuda()).sum().backward()
        for name, t in (("v", v), ("dx", xd.grad), ("dy", yd.grad), ("dR", rd.grad)):
            out[f"ssim{i}_{name}"] = t.detach().cpu().numpy()
        N, C, H, W = shape
        o, t = _images(cva, (N, C, D, H, W), seed=71 + i)
        od, td = o.cuda().requires_grad_(), t.cuda().requires_grad_()
        loss = cva.metrics.ssim_frames(od, td)
        loss.backward()
        for name, t_ in (("v", loss), ("do", od.grad), ("dt", td.grad)):
            out[f"frames{i}_{name}"] = t_.detach().cpu().numpy()
    return out


if __name__ == "__main__":
    import numpy as np
    np.savez_compressed(sys.argv[1], **compute())
    print("wrote", sys.argv[1])
