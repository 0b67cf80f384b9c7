#!/usr/bin/env python3
"""Generate tests/golden/c6m / c7m: the jvp of the CSR nets' clip chains under a noise-level MAP, by running the UNMODIFIED
reference classes CDLNet_CSR / CDLNet_CSRf2 (model/net.py) on CPU under forward-mode autograd.  The manner, the chain, the
gate recorder and the seed rule are those of tools/make_golden_csr_tangent.py (c6 / c7); this script holds none of the
reference's text.

    c6m_csr_jvp_chain_map     CDLNet_CSR's 4-call chain (traincsr.py:201-204), stride 2 on 2 x 1 x 17 x 19 frames
    c7m_csrf2_jvp_chain_map   CDLNet_CSRf2's 5-call chain (traincsr.py:257-261), stride 2 on one 1 x 13 x 15 frame per time step

Every frame has its own per-pixel noise level `noise{t}` (N,1,H,W) in [10, 40] (make_golden_sigmamap.sigma_map plus an
offset per sample, so the samples of a batch differ): the frame is x + n * noise / 255, the net takes the level on its code
grid, `sigma{t}` = utils.sigma_to_code_grid(noise{t}, 2) (the package's convention: the reflect padding of pre_process, then
the mean over each stride block), where it broadcasts against the codes and reaches all three threshold families.  The SURE
loss weighs the divergence at IMAGE resolution,
    sum_t mean((y_t - xhat_t)^2) + 2 mean((noise_t/255)^2 b_t xdot_t),
and every parameter gradient of it is stored beside the inputs, (xhat_t, xdot_t) and the loss.

Seed rule (that of c6 / c7): a seed is accepted only if the gate patterns (x != 0 and |x| - t > 0) of every shrinkage of the
chain agree in a float32 and a float64 run, and the jvp agrees with a float64 central difference (h = 1e-7) to 5e-7 of max.
The smallest | |x| - t | of the float32 run is stored as `gate_margin`.  One condition is added: the float32 outputs agree
to 1e-5 with the float64 ones and with those of a float32 run on frames moved by 1e-7 (the maps also read the sign of the
difference of the two neighbour codes, and a code element the map holds at its neighbour's value ties with it).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_csr_tangent_map.py
"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwad

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save, smooth, state, grads_of   # noqa: E402
from make_golden_csr import detie                                          # noqa: E402
from make_golden_csr_tangent import Recorder, chain                        # noqa: E402
from make_golden_sigmamap import sigma_map                                 # noqa: E402

STRIDE = 2


def noise_maps(shape, D, seed):
    """One image-resolution level map per frame, in [10, 40], another offset for every sample."""
    N = shape[0]
    offs = torch.linspace(-3.0, 3.0, N).reshape(N, 1, 1, 1) if N > 1 else torch.zeros(1, 1, 1, 1)
    return [(sigma_map((N, 1) + tuple(shape[2:]), seed + 13 * t) + offs).clamp(10.0, 40.0).contiguous() for t in range(D)]


def jvp_map_fixture(net_mod, name, variant, seed, shape, thr):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from cdlnet_video_amd.utils import sigma_to_code_grid
    D = 2 if variant == "csr" else 3
    cls = net_mod.CDLNet_CSR if variant == "csr" else net_mod.CDLNet_CSRf2
    hyper = dict(K=3, M=6, P=5, s=STRIDE, C=1)
    mse = lambda a, b: torch.mean((a - b) ** 2)
    for sd_ in range(seed, seed + 400):
        g = torch.Generator().manual_seed(sd_)
        torch.manual_seed(sd_)
        net = cls(**hyper, t0=5e-3, adaptive=True, init=True)
        detie(net, g, thr)
        xs = [smooth(shape, g)]
        for _ in range(D - 1):
            xs.append((0.9 * xs[-1] + 0.1 * smooth(shape, g)).clamp(0, 1))
        noise = noise_maps(shape, D, 5000 + sd_)
        sigmas = [sigma_to_code_grid(n, STRIDE).contiguous() for n in noise]
        ys = [x + torch.randn(shape, generator=g) * n / 255 for x, n in zip(xs, noise)]
        bs = [torch.randn(shape, generator=g) for _ in range(D)]
        with Recorder(net_mod) as r32, fwad.dual_level():
            outs = chain(net, variant, [fwad.make_dual(y.clone(), b) for y, b in zip(ys, bs)], sigmas)
            xh, xd = zip(*(fwad.unpack_dual(o) for o in outs))
            loss = sum(mse(y, a) + 2.0 * torch.mean((n / 255.0) ** 2 * b * d) for y, a, b, d, n in zip(ys, xh, bs, xd, noise))
            loss.backward()
        net64 = cls(**hyper, t0=5e-3, adaptive=True, init=False).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        sig64 = [s_.double() for s_ in sigmas]
        with Recorder(net_mod) as r64, fwad.dual_level():
            outs64 = chain(net64, variant, [fwad.make_dual(y.double(), b.double()) for y, b in zip(ys, bs)], sig64)
            xd64 = [fwad.unpack_dual(o).tangent.detach() for o in outs64]
            xh64 = [fwad.unpack_dual(o).primal.detach() for o in outs64]
        same = len(r32.gates) == len(r64.gates) and all(bool((a == b).all()) for a, b in zip(r32.gates, r64.gates))
        print(f"{name}: seed {sd_}: gates agree: {same}; margin {r32.margin:.3e}")
        if not same:
            continue
        # (beyond c6 / c7) a held code element equals its neighbour's to the last bit or the one before, and prox_CSR_f2 reads
        # sign(z_prev - z_after): the float64 outputs must be the float32 ones, and so must those of a float32 run whose
        # frames are moved by one part in 1e7 (another arithmetic's rounding), or a tie decides the fixture
        gp = torch.Generator().manual_seed(sd_)
        with torch.no_grad():
            moved = chain(net, variant, [y * (1.0 + 1e-7 * torch.randn(shape, generator=gp)) for y in ys], sigmas)
        tie_err = max(float((a.double() - c.double()).abs().max() / a.abs().max())
                      for a, c in list(zip(xh, xh64)) + list(zip(xh, moved)))
        print(f"{name}: float32 outputs vs float64 / vs moved frames: {tie_err:.2e}")
        if tie_err >= 1e-5:
            continue
        h = 1e-7
        with torch.no_grad():
            up = chain(net64, variant, [y.double() + h * b.double() for y, b in zip(ys, bs)], sig64)
            dn = chain(net64, variant, [y.double() - h * b.double() for y, b in zip(ys, bs)], sig64)
        fd_err = max(float(((a - c) / (2 * h) - d).abs().max() / d.abs().max()) for a, c, d in zip(up, dn, xd64))
        print(f"{name}: jvp vs float64 central difference (h = {h}): {fd_err:.2e}")
        if fd_err >= 5e-7:                              # a gate within h |tangent| of its threshold: the difference straddles it
            continue
        arrays = {}
        for t in range(D):
            arrays.update({f"x{t}": xs[t], f"y{t}": ys[t], f"b{t}": bs[t], f"noise{t}": noise[t], f"sigma{t}": sigmas[t],
                           f"xhat{t}": xh[t], f"xdot{t}": xd[t]})
        save(name, loss=loss, seed=sd_, gate_margin=r32.margin, fd_err=fd_err, tie_err=tie_err, **arrays, **state(net), **grads_of(net),
             hyper=np.array([hyper[k] for k in "KMPsC"]))
        return
    raise SystemExit(f"{name}: no seed with equal float32 / float64 gates")


def main():
    net_mod, _ = import_reference()
    only = set(sys.argv[1:])
    want = lambda tag: not only or tag in only
    csr_thr = {"t": (2e-3, 1.5e-2), "t2": (2e-3, 1.5e-2), "g": (0.2, 1.4)}
    f2_thr = {"t": (2e-3, 1.5e-2), "g1": (0.2, 1.4), "g2": (0.2, 1.4)}
    if want("c6m"):
        jvp_map_fixture(net_mod, "c6m_csr_jvp_chain_map", "csr", 161, (2, 1, 17, 19), csr_thr)
    if want("c7m"):
        jvp_map_fixture(net_mod, "c7m_csrf2_jvp_chain_map", "f2", 171, (1, 1, 13, 15), f2_thr)


if __name__ == "__main__":
    main()
