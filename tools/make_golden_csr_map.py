#!/usr/bin/env python3
"""Generate tests/golden/cm*.npz and cd1*.npz: the CSR nets with a noise-level MAP as `sigma`, and with gradients with
respect to the data, by running the UNMODIFIED reference classes CDLNet_CSR / CDLNet_CSRf2 on CPU (same import shim as
tools/make_golden.py; this script holds none of the reference's text).  In the reference the map reaches all three
threshold families by broadcasting (t, g / g1, g2 against c = sigma / 255).

Each fixture reuses the net and the inputs of an existing c-fixture (tools/make_golden_csr.py):
    cm1  (c1)   CDLNet_CSR, the three-call chain, an (N,1,20,24) map per frame, y0 and y1 requiring grad
    cm1b (c1b)  CDLNet_CSR, stride 2 on 19 x 21, a code-grid map (1,1,10,11), a leaf z_prev
    cm2  (c2)   CDLNet_CSRf2, the chain over all four branches, one (1,1,18,22) map
    cd1  (c1)   no map: a per-sample (2,1,1,1) sigma and y requiring grad
and records every call's xhat and z, the loss (the c-fixture's, plus mean(w * xhat) per call as the s-fixtures have it),
every parameter gradient, dL/dy, dL/dsigma (in sigma's shape) and the neighbour-code gradients.

Maps come from make_golden_sigmamap.sigma_map, in [10, 40]; the seed is screened with its Margin observer at 1e-6 (a code
within rounding of a threshold would take its side of the shrinkage, and the gradients with it) and the margin stored.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_csr_map.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save, grads_of            # noqa: E402
from make_golden_sigmamap import MARGIN, Margin, sigma_map          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
mse = lambda a, b: torch.mean((a - b) ** 2)


def load(src):
    d = np.load(os.path.join(GOLDEN, src + ".npz"))
    return {k: (torch.from_numpy(d[k].copy()) if d[k].dtype.kind == "f" else d[k]) for k in d.files}


def build(net_mod, f, cls):
    K, M, P, s, C = [int(v) for v in f["hyper"]]
    net = getattr(net_mod, cls)(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=True, init=False)
    net.load_state_dict({k[3:]: v for k, v in f.items() if k.startswith("sd/")}, strict=True)
    return net


def leaf(t):
    return t.clone().requires_grad_(True)


def chain_csr(net, f, w, sig0, sig1):
    """The three calls of c1 (traincsr.py:203-204): frame 0 alone, frame 1 given z0, frame 0 again given z1."""
    y0, y1 = leaf(f["y0"]), leaf(f["y1"])
    xh0, z0 = net(y0, None, sig0)
    xh1, z1 = net(y1, z0, sig1)
    xh0b, z0b = net(y0, z1, sig0)
    z0.retain_grad()
    z1.retain_grad()
    loss = mse(f["x0"], xh0) + mse(f["x1"], xh1) + mse(f["x0"], xh0b) + torch.mean(w * xh0) + torch.mean(w * xh1) \
        + torch.mean(w * xh0b)
    return loss, dict(xh0=xh0, z0=z0, xh1=xh1, z1=z1, xh0b=xh0b, z0b=z0b), dict(dy0=y0, dy1=y1, grad_z0=z0, grad_z1=z1)


def chain_f2(net, f, w, sig):
    """The five calls of c2 (traincsr.py:257-261): all four branches of CDLNet_CSRf2."""
    ys = [leaf(f[k]) for k in ("y0", "y1", "y2")]
    xp, zp = net(ys[0], None, None, sig)
    xc, zc = net(ys[1], zp, None, sig)
    xa, za = net(ys[2], zc, None, sig)
    xc2, zc2 = net(ys[1], zp, za, sig)
    xp2, zp2 = net(ys[0], None, za, sig)
    for z in (zp, zc, za):
        z.retain_grad()
    outs = dict(xp=xp, zp=zp, xc=xc, zc=zc, xa=xa, za=za, xc2=xc2, zc2=zc2, xp2=xp2, zp2=zp2)
    loss = mse(f["x0"], xp) + mse(f["x1"], xc) + mse(f["x2"], xa) + mse(f["x1"], xc2) + mse(f["x0"], xp2) \
        + sum(torch.mean(w * outs[k]) for k in ("xp", "xc", "xa", "xc2", "xp2"))
    return loss, outs, dict(dy0=ys[0], dy1=ys[1], dy2=ys[2], grad_zp=zp, grad_zc=zc, grad_za=za)


def single_csr(net, f, w, sig):
    """The one call of c1b: a leaf neighbour code, the returned code in the loss."""
    y, zprev = leaf(f["y"]), leaf(f["zprev"])
    xh, z = net(y, zprev, sig)
    loss = mse(f["x"], xh) + 0.1 * z.abs().mean() + torch.mean(w * xh)
    return loss, dict(xhat=xh, z=z), dict(dy=y, grad_zprev=zprev)


def main():
    net_mod, _ = import_reference()
    jobs = [
        # name, source, class, shapes of the maps (None: the source's own per-sample sigma), runner
        ("cm1_csr_chain_map", "c1_csr_chain", "CDLNet_CSR", [(2, 1, 20, 24), (2, 1, 20, 24)], chain_csr),
        ("cm1b_csr_s2_odd_map", "c1b_csr_s2_odd", "CDLNet_CSR", [(1, 1, 10, 11)], single_csr),
        ("cm2_csrf2_chain_map", "c2_csrf2_chain", "CDLNet_CSRf2", [(1, 1, 18, 22)], chain_f2),
        ("cd1_csr_chain_datagrad", "c1_csr_chain", "CDLNet_CSR", None, chain_csr),
    ]
    for i, (name, src, cls, shapes, runner) in enumerate(jobs):
        f = load(src)
        xkey = "x0" if "x0" in f else "x"
        w = torch.randn(f[xkey].shape, generator=torch.Generator().manual_seed(700 + i))
        for seed in range(900 + i, 900 + i + 100 * 40, 100):
            net = build(net_mod, f, cls)
            if shapes is None:
                sigmas = [leaf(f["sigma"])] * 2                 # one leaf: both frames share the per-sample levels
            else:
                sigmas = [sigma_map(sh, seed + 7 * j).requires_grad_(True) for j, sh in enumerate(shapes)]
            with Margin(net_mod) as watch:
                loss, outs, leaves = runner(net, f, w, *sigmas)
            print(f"{name} seed {seed}: smallest | |u| - tau | / tau = {watch.value:.2e}")
            if watch.value > MARGIN:
                break
            if shapes is None:
                raise SystemExit(f"{name}: the source fixture's own margin is below {MARGIN}")
        else:
            raise SystemExit(f"{name}: no seed with a safe shrinkage margin")
        loss.backward()
        distinct = sigmas[:1] if shapes is None else sigmas
        for s_ in distinct:
            assert s_.grad.shape == s_.shape
            if shapes is not None:
                assert 10.0 <= float(s_.detach().min()) and float(s_.detach().max()) <= 40.0
        sig = {f"sigma{j}": s_.detach() for j, s_ in enumerate(distinct)}
        dsig = {f"dsigma{j}": s_.grad for j, s_ in enumerate(distinct)}
        inputs = {k: v for k, v in f.items() if k[0] in "xy" and k[1:].isdigit() or k in ("x", "y", "zprev")}
        save(name, **inputs, w=w, **sig, **dsig, **outs, loss=loss, **{k: v.grad for k, v in leaves.items()},
             **grads_of(net), **{k: v for k, v in f.items() if k.startswith("sd/")}, hyper=f["hyper"],
             source=np.array(src), margin=np.float32(watch.value))


if __name__ == "__main__":
    main()
