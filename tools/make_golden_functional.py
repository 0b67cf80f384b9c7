#!/usr/bin/env python3
"""Generate tests/golden/p*.npz (the differentiable building blocks) by running the UNMODIFIED
reference on CPU: prox_CSR / prox_CSR_f2 (model/net.py:229-262) with thresholds shaped like a noise-level map, and one
CDLNet_CSRf2 call (model/net.py:464-568) with `sigma` a map -- what the reference's torch expressions broadcast and this
package's CSR nets refuse.  Same shims and rules as tools/make_golden.py; its own script, so that the existing fixtures
(whose values depend on RNG call order) are untouched.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_functional.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save, smooth, state, grads_of   # noqa: E402
from make_golden_csr import detie                                          # noqa: E402


def main():
    net_mod, _ = import_reference()
    g = torch.Generator().manual_seed(2323)

    # ---- P0: the two maps with thresholds t0[m] + c[n,pix] * t1[m], c a map; a sixth of the base values negative ----
    N, M, H, W = 2, 3, 6, 7
    shape = (N, M, H, W)
    sparse = lambda: 0.05 * torch.randn(shape, generator=g) * (torch.rand(shape, generator=g) > 0.4)
    u = (0.05 * torch.randn(shape, generator=g) * (torch.rand(shape, generator=g) > 0.1)).requires_grad_(True)
    zp, za = sparse().requires_grad_(True), sparse().requires_grad_(True)
    c = (torch.rand(N, 1, H, W, generator=g) * 0.2).requires_grad_(True)
    fam = []
    for scale in (0.02, 1.2, 1.2):
        p = scale * torch.rand(2, 1, M, 1, 1, generator=g)
        p[0] = torch.where(torch.rand(p[0].shape, generator=g) < 1 / 6, -p[0], p[0])
        fam.append(p.requires_grad_(True))
    t, g1, g2 = fam
    thr = lambda p: p[0] + c * p[1]
    G = torch.randn(shape, generator=g)
    rec = {}
    for name, fn in (("csr", lambda: net_mod.prox_CSR(u, zp, thr(t), thr(g1))),
                     ("f2", lambda: net_mod.prox_CSR_f2(u, zp, za, thr(t), thr(g1), thr(g2)))):
        for v in (u, zp, za, c, t, g1, g2):
            v.grad = None
        out = fn()
        (out * G).sum().backward()
        rec[f"{name}_out"] = out
        for key, v in (("u", u), ("zp", zp), ("za", za), ("c", c), ("t", t), ("g1", g1), ("g2", g2)):
            if v.grad is not None:
                rec[f"{name}_d{key}"] = v.grad.clone()
    save("p0_prox_map_thresholds", u=u, zp=zp, za=za, c=c, t=t, g1=g1, g2=g2, G=G, **rec)

    # ---- P1: CDLNet_CSRf2 with both neighbours and a sigma map, every gradient the reference's graph gives ---------
    torch.manual_seed(29)
    K, M, P, s, C = 3, 6, 5, 1, 1
    net = net_mod.CDLNet_CSRf2(K=K, M=M, P=P, s=s, C=C, t0=5e-3, adaptive=True, init=True)
    detie(net, g, {"t": (2e-3, 1.5e-2), "g1": (0.2, 1.2), "g2": (0.2, 1.2)})
    x = smooth((2, 1, 20, 24), g)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 20), torch.linspace(0, 1, 24), indexing="ij")
    sigma = ((12 + 25 * yy * xx).expand(2, 1, 20, 24) + 6 * torch.arange(2).reshape(2, 1, 1, 1)).clone()
    ys = [x + torch.randn(x.shape, generator=g) * sigma / 255 for _ in range(3)]
    with torch.no_grad():
        _, zp = net(ys[0], None, None, sigma)
        _, za = net(ys[2], None, None, sigma)
    y = ys[1].clone().requires_grad_(True)
    sg = sigma.clone().requires_grad_(True)
    zp, za = zp.clone().requires_grad_(True), za.clone().requires_grad_(True)
    xhat, z = net(y, zp, za, sg)
    loss = torch.mean((x - xhat) ** 2) + 0.05 * z.abs().mean()
    loss.backward()
    save("p1_csrf2_sigma_map", x=x, y=y, sigma=sigma, zp=zp, za=za, xhat=xhat, z=z, loss=loss, dy=y.grad, dsigma=sg.grad,
         dzp=zp.grad, dza=za.grad, **state(net), **grads_of(net), hyper=np.array([K, M, P, s, C]))


if __name__ == "__main__":
    main()
