#!/usr/bin/env python3
"""Generate tests/golden/d*_datagrad.npz: the reference's gradients with respect to the noisy input y and the noise
level sigma, by running the UNMODIFIED reference on CPU (same import shim as tools/make_golden.py).

Each fixture reuses the inputs and parameters of an existing forward fixture (f1, f2, f3, f3b, f4a, f4c), with a
per-sample sigma tensor that requires grad (adaptive=True), and records xhat, dL/dy and dL/dsigma for the fixed loss
    L = mean((xhat - x)^2) + mean(w * xhat),     w seeded per fixture (so dL/dxhat has a non-zero mean).
d0_adaptive_false: the f1 net with adaptive=False, whose sigma gradient is None (stored as has_dsigma = 0).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_datagrad.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, save   # noqa: E402

SOURCES = [  # new fixture, forward fixture, kind
    ("d1_2d_s1", "f1_2d_s1", "2d"),
    ("d2_2d_s2_odd", "f2_2d_s2_odd", "2d"),
    ("d3_jdd_c3_mask", "f3_jdd_c3_mask", "2d"),
    ("d3b_jdd_s2_odd", "f3b_jdd_s2_odd", "2d"),
    ("d4a_3d_p555", "f4a_3d_p555", "3d"),
    ("d4c_3d_s2_odd", "f4c_3d_s2_odd", "3d"),
]


def load(name):
    d = np.load(os.path.join(OUT, name + ".npz"))
    return {k: torch.from_numpy(d[k].copy()) for k in d.files}


def build(net_mod, f, kind, adaptive=True):
    K, M, P, s, C = [int(v) for v in f["hyper"]]
    if kind == "2d":
        net = net_mod.CDLNet(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=adaptive, init=False)
    else:
        P3 = [int(v) for v in f["P3"]]
        net = net_mod.CDLNetVideo(K=K, M=M, P=P3, s=s, C=C, t0=0.0, adaptive=adaptive, depth=int(f["x"].shape[2]),
                                  init=False)
    sd = {k[3:]: v for k, v in f.items() if k.startswith("sd/")}
    net.load_state_dict(sd, strict=True)
    return net


def run(net, f, sigma, seed):
    x = f["x"]
    y = f["y"].clone().requires_grad_(True)
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))
    kw = {"mask": f["mask"]} if "mask" in f else {}
    xhat, _ = net(y, sigma, **kw)
    loss = torch.mean((xhat - x) ** 2) + torch.mean(w * xhat)
    loss.backward()
    return xhat, loss, w, y.grad


def main():
    net_mod, _ = import_reference()
    for i, (name, src, kind) in enumerate(SOURCES):
        f = load(src)
        N = f["x"].shape[0]
        nd = f["x"].dim() - 2
        base = torch.tensor([12.0, 25.0, 40.0])[:N] if N <= 3 else torch.linspace(10.0, 40.0, N)
        sigma = base.reshape((N,) + (1,) * (nd + 1)).clone().requires_grad_(True)
        net = build(net_mod, f, kind)
        xhat, loss, w, dy = run(net, f, sigma, 100 + i)
        save(name, x=f["x"], y=f["y"], w=w, sigma=sigma.detach(), xhat=xhat, loss=loss, dy=dy,
             dsigma=sigma.grad, has_dsigma=1, **({"mask": f["mask"]} if "mask" in f else {}),
             **{k: v for k, v in f.items() if k.startswith("sd/")}, hyper=f["hyper"],
             **({"P3": f["P3"]} if "P3" in f else {}), source=np.array(src))
    # adaptive=False: sigma never reaches the graph (net.py:82), its gradient stays None
    f = load("f1_2d_s1")
    net = build(net_mod, f, "2d", adaptive=False)
    sigma = torch.tensor([12.0, 25.0]).reshape(2, 1, 1, 1).requires_grad_(True)
    xhat, loss, w, dy = run(net, f, sigma, 99)
    assert sigma.grad is None
    save("d0_adaptive_false", x=f["x"], y=f["y"], w=w, sigma=sigma.detach(), xhat=xhat, loss=loss, dy=dy,
         has_dsigma=0, **{k: v for k, v in f.items() if k.startswith("sd/")}, hyper=f["hyper"],
         source=np.array("f1_2d_s1"))


if __name__ == "__main__":
    main()
