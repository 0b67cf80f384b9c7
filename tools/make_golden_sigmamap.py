#!/usr/bin/env python3
"""Generate tests/golden/s*.npz: the reference run with a noise-level MAP as `sigma` -- a tensor that broadcasts against
the codes (one level per frame (N,1,D,1,1), or a full map on the code grid) instead of one level per sample -- by
running the UNMODIFIED reference on CPU (same import shim as tools/make_golden.py; this script holds none of its text).

Each fixture reuses the net and the inputs of an existing fixture (f1, f2, f3, f4a, f4c, f5b, r1) and records sigma,
xhat, z, the loss
    L = mean((xhat - x)^2) + mean(w * xhat),     w seeded per fixture (as the d-fixtures),
every parameter gradient, dL/dy and dL/dsigma (sr1, the residual chain: xhat, z and parameter gradients only).
Maps are a smooth field plus seeded noise, in [10, 40], so that neighbouring thresholds differ.

Near-ties: a code whose |u| is within rounding of its threshold lands on either side of the shrinkage depending on
summation order, and takes the gradients with it.  The map's seed is therefore screened (as make_golden_residual.py
screens its ReLU margins): an observer around the reference's ST() records the smallest | |u| - tau | / tau of the run,
and the first seed whose margin exceeds 1e-6 is kept.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sigmamap.py
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save, smooth, grads_of   # noqa: E402
from make_golden_datagrad import build                              # noqa: E402

MARGIN = 1e-6

# new fixture, source fixture, kind, shape of sigma as a function of (N, spatial extent of x, stride)
def _code(sp, s):
    return tuple(-(-d // s) for d in sp)


SOURCES = [
    ("s1_2d_s1", "f1_2d_s1", "2d", lambda N, sp, s: (N, 1) + sp),                       # image grid (s = 1)
    ("s2_2d_s2_odd", "f2_2d_s2_odd", "2d", lambda N, sp, s: (N, 1) + _code(sp, s)),     # code grid of an odd image
    ("s3_jdd_c3_mask", "f3_jdd_c3_mask", "2d", lambda N, sp, s: (N, 1) + sp),
    ("s4a_3d_frames", "f4a_3d_p555", "3d", lambda N, sp, s: (N, 1, sp[0], 1, 1)),       # one level per frame
    ("s4a_3d_map", "f4a_3d_p555", "3d", lambda N, sp, s: (N, 1) + sp),
    ("s4c_3d_s2_odd", "f4c_3d_s2_odd", "3d", lambda N, sp, s: (N, 1) + _code(sp, s)),
    ("s5b_gabor", "f5b_gabor_plain", "gabor", lambda N, sp, s: (N, 1) + sp),
    ("sr1_video_residual", "r1_video_residual", "residual", lambda N, sp, s: (N, 1) + sp),
]


class Margin:
    """Observer around the reference's ST(x, t): smallest | |x| - t | / |t| seen (the function itself is called as is)."""

    def __init__(self, net_mod):
        self.net_mod, self.orig, self.value = net_mod, net_mod.ST, float("inf")

    def __enter__(self):
        def watched(x, t):
            rel = ((x.detach().abs() - t.detach()).abs() / t.detach().abs().clamp_min(1e-30)).min()
            self.value = min(self.value, float(rel))
            return self.orig(x, t)
        self.net_mod.ST = watched
        return self

    def __exit__(self, *exc):
        self.net_mod.ST = self.orig
        return False


def sigma_map(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    nd = len(shape) - 2
    if all(d == 1 for d in shape[3:]):                      # per frame: a ramp plus noise
        field = torch.linspace(0.0, 1.0, shape[2]).reshape((1, 1, shape[2]) + (1,) * (nd - 1)).expand(shape)
    elif min(shape[2:]) >= 5:
        field = smooth(shape, gen)
    else:
        field = smooth((shape[0], 1) + tuple(max(d, 5) for d in shape[2:]), gen)[
            (slice(None), slice(None)) + tuple(slice(0, d) for d in shape[2:])]
    noise = torch.rand(shape, generator=gen)
    return (10.0 + 30.0 * (0.8 * field + 0.2 * noise)).contiguous()


def build_net(net_mod, f, kind):
    if kind in ("2d", "3d"):
        return build(net_mod, f, kind)
    sd = {k[3:]: v for k, v in f.items() if k.startswith("sd/")}
    hyper = [int(v) for v in f["hyper"]]
    if kind == "gabor":
        K, M, P, s, C = hyper
        net = net_mod.GDLNet(K=K, M=M, P=P, s=s, C=C, t0=0.0, order=int(f["order"]), adaptive=True, shared="",
                             init=False)
        for mod in list(net.A) + list(net.B):               # torch >= 2: the private call wants num_spatial_dims
            mod._output_padding = functools.partial(mod._output_padding, num_spatial_dims=2)
    else:
        K, M, Pd, Ph, Pw, s, C = hyper
        net = net_mod.CDLNetVideo(K=K, M=M, P=(Pd, Ph, Pw), s=s, C=C, t0=0.0, adaptive=True,
                                  depth=int(f["x"].shape[2]), init=False, residual=True)
    net.load_state_dict(sd, strict=True)
    return net


def main():
    net_mod, _ = import_reference()
    for i, (name, src, kind, shape_of) in enumerate(SOURCES):
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", src + ".npz"))
        f = {k: (torch.from_numpy(d[k].copy()) if d[k].dtype.kind == "f" else d[k]) for k in d.files}
        x = f["x"]
        s = int(f["hyper"][-2])
        shape = shape_of(x.shape[0], tuple(x.shape[2:]), s)
        w = torch.randn(x.shape, generator=torch.Generator().manual_seed(300 + i))
        kw = {"mask": f["mask"]} if "mask" in f else {}
        for seed in range(500 + i, 500 + i + 100 * 40, 100):
            net = build_net(net_mod, f, kind)
            sigma = sigma_map(shape, seed).requires_grad_(True)
            y = f["y"].clone().requires_grad_(True)
            with Margin(net_mod) as watch:
                xhat, z = net(y, sigma, **kw)
            print(f"{name} seed {seed}: smallest | |u| - tau | / tau = {watch.value:.2e}")
            if watch.value > MARGIN:
                break
        else:
            raise SystemExit(f"{name}: no seed with a safe shrinkage margin")
        assert 10.0 <= float(sigma.detach().min()) and float(sigma.detach().max()) <= 40.0
        loss = torch.mean((xhat - x) ** 2) + torch.mean(w * xhat)
        loss.backward()
        assert sigma.grad.shape == sigma.shape
        data = {} if kind == "residual" else {"dy": y.grad, "dsigma": sigma.grad}
        extra = {k: f[k] for k in ("P3", "order", "shared", "mask") if k in f}
        save(name, x=x, y=f["y"], w=w, sigma=sigma.detach(), xhat=xhat, z=z, loss=loss, **data, **grads_of(net),
             **{k: v for k, v in f.items() if k.startswith("sd/")}, hyper=f["hyper"], **extra,
             source=np.array(src), margin=np.float32(watch.value))


if __name__ == "__main__":
    main()
