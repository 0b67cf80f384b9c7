#!/usr/bin/env python3
"""Generate tests/golden/n*_nle_pca.npz by running the UNMODIFIED reference `model.nle.nle_pca` on CPU.

Runs only where the reference checkout is available.  The import goes through make_golden.import_reference (its
torchvision shim) plus an empty `pywt` module: model/nle.py imports PyWavelets only through model/wvlt.py, which
the MAD estimator uses and nle_pca never touches.  Fixtures are data only: the noisy input y, the reference's
(nlevel, th, num) and the constants of the patch size (tau0, r = rank(DD), tr(DD)).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_nle_pca.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_golden                     # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden")


def reference_nle():
    sys.modules.setdefault("pywt", types.ModuleType("pywt"))
    make_golden.import_reference()
    import model.nle as nle             # noqa: E402
    return nle


def smooth(shape, seed, cycles=1.5):
    """Slowly varying content in [0.2, 0.8]: a few 2-D sinusoids of at most `cycles` periods across the image."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    i, j = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    out = torch.zeros(shape)
    for n in range(N):
        for c in range(C):
            acc = torch.zeros(H, W)
            for _ in range(3):
                fi, fj = (torch.rand(2, generator=g) * cycles).tolist()
                ph = float(torch.rand(1, generator=g)) * 6.283
                acc += torch.sin(6.283 * (fi * i + fj * j) + ph)
            out[n, c] = 0.2 + 0.6 * (acc - acc.min()) / (acc.max() - acc.min())
    return out


def textured(shape, seed):
    """Smooth content plus a fine oriented grating and a checkerboard patch: strong texture in part of the image."""
    x = smooth(shape, seed=seed, cycles=3.0)
    H, W = shape[2:]
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    grating = 0.25 * torch.sin(0.9 * i + 0.4 * j)
    checker = 0.3 * (((i // 3) + (j // 3)) % 2) * (j < W // 2)
    return x + grating + checker


CASES = [
    # name, clean image, sigma (of 255), patchsize, conf, itr
    ("n1", lambda: smooth((1, 1, 64, 64), seed=11), 25, 7, 1 - 1e-6, 3),
    ("n2", lambda: smooth((4, 1, 96, 80), seed=12, cycles=1.0), 5, 7, 1 - 1e-6, 3),
    ("n3", lambda: textured((2, 1, 256, 256), seed=13), 50, 7, 1 - 1e-6, 3),
    ("n4", lambda: smooth((1, 1, 10, 12), seed=14), 15, 7, 1 - 1e-6, 3),
    ("n5", lambda: smooth((2, 1, 72, 64), seed=15, cycles=2.0), 15, 5, 1 - 1e-6, 4),
    ("n6", lambda: smooth((2, 1, 80, 72), seed=16, cycles=4.0), 10, 7, 0.99, 3),
]


def main():
    nle = reference_nle()
    for i, (name, clean, sigma, p, conf, itr) in enumerate(CASES):
        x = clean()
        g = torch.Generator().manual_seed(100 + i)
        y = (x + torch.randn(x.shape, generator=g) * sigma / 255).float()
        nlevel, th, num = nle.nle_pca(y, patchsize=p, conf=conf, itr=itr)
        # the constants nle_pca derives from the patch size, the same way it does
        kh = torch.tensor([1 / 2, 0, -1 / 2]).float().reshape(1, 1, 1, 3)
        Dh, Dv = nle.convmtx2(kh, p, p), nle.convmtx2(kh.transpose(2, 3), p, p)
        DD = Dh.T @ Dh + Dv.T @ Dv
        r = int(torch.linalg.matrix_rank(DD, hermitian=True))
        tr = float(torch.trace(DD))
        tau0 = float(nle.gamma.ppf(conf, r / 2.0, scale=2.0 * tr / float(r)))
        path = os.path.join(OUT, f"{name}_nle_pca.npz")
        np.savez_compressed(path, y=y.numpy(), nlevel=np.float64(nlevel), th=np.float64(th), num=np.float64(num),
                            tau0=np.float64(tau0), r=np.int64(r), trDD=np.float64(tr), patchsize=np.int64(p),
                            conf=np.float64(conf), itr=np.int64(itr), sigma=np.float64(sigma))
        print(f"{name}: y {tuple(y.shape)} sigma {sigma}: nlevel*255 {255 * float(nlevel):.4f} th {float(th):.6g} "
              f"num {float(num):.0f} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
