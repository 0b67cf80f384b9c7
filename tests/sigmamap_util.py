"""Shared by tests/test_sigmamap_cpu.py and tests/test_gpu_sigmamap.py: the oracle's autograd with a noise-level map
(oracle/cdl_oracle.py takes one as it stands: its thresholds are the reference's broadcast) for the loss of the s-fixtures,
    L = mean((xhat - x)^2) + mean(w * xhat)."""
import torch

from oracle import cdl_oracle as O

FIXTURES = [  # name, kind
    ("s1_2d_s1", "2d"), ("s2_2d_s2_odd", "2d"), ("s3_jdd_c3_mask", "2d"), ("s4a_3d_frames", "3d"),
    ("s4a_3d_map", "3d"), ("s4c_3d_s2_odd", "3d"), ("s5b_gabor", "gabor"),
]
RESIDUAL_FIXTURE = "sr1_video_residual"


def loss_of(xhat, x, w):
    return torch.mean((xhat - x) ** 2) + torch.mean(w * xhat)


def oracle_grads(sd, x, y, w, sigma, *, K, P, s, mask=None, ndim=2, gabor=False, supports=None):
    """(xhat, z, loss, {parameter: grad}, dL/dy, dL/dsigma) of the oracle, every leaf detached from the caller's."""
    keys = O.trainable(sd, K, gabor)
    work = dict(sd)
    leaves = {}
    for key in keys:
        leaves[key] = work[key] = sd[key].detach().clone().requires_grad_(True)
    yl = y.detach().clone().requires_grad_(True)
    sl = sigma.detach().clone().requires_grad_(True)
    xhat, z = O.ista(work, yl, K=K, P=P, s=s, sigma=sl, adaptive=True, mask=mask, ndim=ndim, gabor=gabor,
                     supports=supports)
    loss = loss_of(xhat, x, w)
    loss.backward()
    return xhat.detach(), z.detach(), float(loss.detach()), {k: leaves[k].grad for k in keys}, yl.grad, sl.grad


def fixture_args(g, kind):
    K, M, P, s, C = g["hyper"]
    nd = g["x"].dim() - 2
    P = tuple(g["P3"]) if "P3" in g else P
    return dict(K=K, P=P, s=s, mask=g.get("mask"), ndim=nd, gabor=kind == "gabor")


def smooth_map(shape, seed, lo=10.0, hi=40.0):
    """A noise-level map in [lo, hi]: a separable smooth field plus seeded noise, so that neighbouring thresholds
    differ."""
    gen = torch.Generator().manual_seed(seed)
    field = torch.ones(shape)
    for ax in range(2, len(shape)):
        n = shape[ax]
        ramp = 0.5 + 0.5 * torch.cos(torch.linspace(0.0, 3.0, n) + float(torch.rand((), generator=gen)) * 6.28)
        field = field * ramp.reshape([n if i == ax else 1 for i in range(len(shape))])
    noise = torch.rand(shape, generator=gen)
    return lo + (hi - lo) * (0.8 * field + 0.2 * noise)
