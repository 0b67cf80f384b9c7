#!/usr/bin/env python3
"""Generate tests/golden/j*.npz: the reference's Jacobian-vector product in the observation and the parameter
gradients of a loss on it, by running the UNMODIFIED reference on CPU under torch.autograd.forward_ad (a dual y, backward
through the dual outputs; same import shim as tools/make_golden.py).

Each fixture reuses the inputs and parameters of an existing forward fixture:
    j1_2d_s2_odd    f2_2d_s2_odd      2-D, stride 2, odd size, per-sample sigma
    j2_jdd_c3_mask  f3_jdd_c3_mask    C = 3 with a Bayer mask
    j3_3d_p555      f4a_3d_p555       3-D
and records y, v (the direction, seeded), sigma, mask, the state_dict, xhat, xdot = J(y) v, and the gradients of
    L = mean(w * xdot) + mean((xhat - y)^2),     w seeded per fixture.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_tangent.py
"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwad

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save   # noqa: E402
from make_golden_datagrad import build, load      # noqa: E402

SOURCES = [  # new fixture, forward fixture, kind
    ("j1_2d_s2_odd", "f2_2d_s2_odd", "2d"),
    ("j2_jdd_c3_mask", "f3_jdd_c3_mask", "2d"),
    ("j3_3d_p555", "f4a_3d_p555", "3d"),
]


def main():
    net_mod, _ = import_reference()
    for i, (name, src, kind) in enumerate(SOURCES):
        f = load(src)
        net = build(net_mod, f, kind)
        y, sigma = f["y"], f["sigma"]
        gen = torch.Generator().manual_seed(300 + i)
        v = torch.randn(y.shape, generator=gen)
        w = torch.randn(y.shape, generator=gen)
        kw = {"mask": f["mask"]} if "mask" in f else {}
        if "mask" in f:                                   # a direction in the observation lives on the mask
            v = f["mask"] * v
        with fwad.dual_level():
            out, _ = net(fwad.make_dual(y.clone(), v), sigma, **kw)
            xhat, xdot = fwad.unpack_dual(out)
            loss = torch.mean(w * xdot) + torch.mean((xhat - y) ** 2)
            loss.backward()
        grads = {"grad/" + n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        save(name, y=y, v=v, w=w, sigma=sigma, xhat=xhat, xdot=xdot, loss=loss, **kw, **grads,
             **{k: t for k, t in f.items() if k.startswith("sd/")}, hyper=f["hyper"],
             **({"P3": f["P3"]} if "P3" in f else {}), source=np.array(src))


if __name__ == "__main__":
    main()
