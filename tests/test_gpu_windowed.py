"""Windowed inference on the device (cva.denoise_windowed): windows with an exact halo against
net(y, sigma, mask)[0] and against the CPU oracle, with the tier that ran read from the launch trace; a halo of 0 must
show; an approximate temporal halo with the ramp; a noise-level map; one window; the batch grouping.

XTOL is the project's own for xhat (tests/test_gpu_sigmamap.py)."""
import functools

import pytest
import torch

from gpu_util import check, launch_sites, log, rel_err
from oracle import cdl_oracle as O
from sigmamap_util import smooth_map

pytestmark = pytest.mark.gpu

XTOL = 1e-5
FUSED_FILES = {"cdl_fused2d.hip", "cdl_fusedg.hip", "cdl_strip.hip", "cdl_stripg.hip"}
STAGES = {"k_stage": "cdl_fused2d.hip:k_stage<", "k_strip": "cdl_strip.hip:k_strip<",
          "k_stage_g": "cdl_fusedg.hip:k_stage_g<", "k_stripg": "cdl_stripg.hip:k_stripg<"}

CASES = {
    # kind, net kwargs, input shape, masked, window, halo, the stage kernel expected (None: not asserted)
    1: ("2d", dict(K=2, M=32, P=3, s=1), (2, 1, 96, 80), False, (32, 32), 4, ("k_stage",)),
    2: ("2d", dict(K=2, M=16, P=3, s=2), (1, 1, 71, 65), False, (24, 32), 4, ("k_strip",)),
    3: ("2d", dict(K=2, M=32, P=3, s=1), (1, 3, 64, 56), True, None, "exact", ("k_stage_g", "k_stripg")),
    4: ("3d", dict(K=2, M=16, P=[3, 3, 3], s=1), (1, 1, 20, 40, 36), False, (6, None, None), 4, None),
    5: ("gabor", dict(K=2, M=8, P=7, s=1), (1, 1, 64, 60), False, None, "exact", None),
}


@functools.lru_cache(maxsize=None)
def case(n):
    """(net on the device, y, sigma, mask | 1, net(y, sigma, mask)[0], the CPU oracle's xhat): built once, read-only."""
    import cdlnet_video_amd as cva
    kind, kw, shape, masked = CASES[n][:4]
    torch.manual_seed(40 + n)
    if kind == "2d":
        net = cva.CDLNet(C=shape[1], t0=5e-3, adaptive=True, init=True, **kw)
    elif kind == "3d":
        net = cva.CDLNetVideo(C=shape[1], t0=5e-3, adaptive=True, depth=shape[2], init=True, **kw)
    else:
        net = cva.GDLNet(C=shape[1], t0=5e-3, order=1, adaptive=True, shared="", init=True, **kw)
    with torch.no_grad():                              # de-tie the K identical banks and the thresholds
        for name, p in net.named_parameters():
            if name == "t":
                p.uniform_(2e-3, 2e-2)
            elif name != "g":
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = cva.utils.synthetic_clip(shape, seed=50 + n)
    gen = torch.Generator().manual_seed(60 + n)
    sigma = torch.linspace(20.0, 30.0, shape[0]).reshape((shape[0],) + (1,) * (len(shape) - 1))
    y = x + torch.randn(shape, generator=gen) * sigma / 255
    mask = O.bayer_mask(x) if masked else None
    if mask is not None:
        y = mask * y
    nd = len(shape) - 2
    P = tuple(kw["P"]) if nd == 3 else kw["P"]
    if kind == "gabor":
        sd = O.gabor_alias(dict(sd), kw["K"], "")
    with torch.no_grad():
        xo, _ = O.ista(sd, y, K=kw["K"], P=P, s=kw["s"], sigma=sigma, adaptive=True, mask=mask, ndim=nd,
                       gabor=kind == "gabor")
        net = net.cuda()
        yd, sd_, md = y.cuda(), sigma.cuda(), (mask.cuda() if mask is not None else 1)
        full = net(yd, sd_, mask=md)[0]
    return net, yd, sd_, md, full, xo


def stages(trace):
    sites = launch_sites(trace)
    return {name for name, prefix in STAGES.items() if any(k.startswith(prefix) for k in sites)}


@pytest.mark.parametrize("n", sorted(CASES))
def test_exact_halo_matches_the_untiled_net_and_the_oracle(n):
    import cdlnet_video_amd as cva
    window, halo, want = CASES[n][4:]
    net, y, sigma, mask, full, xo = case(n)
    with torch.no_grad(), cva.ops.trace() as t:
        got = cva.denoise_windowed(net, y, sigma, mask, window=window, halo=halo)
        torch.cuda.synchronize()
    ran = stages(t)
    log(f"windowed case {n}: stage kernels {sorted(ran)}; bit-identical to net(y): {torch.equal(got, full)}")
    assert got.shape == y.shape
    check(f"windowed case {n} vs net(y)", got, full, XTOL)
    check(f"windowed case {n} vs oracle", got, xo, XTOL)
    check(f"windowed case {n} net(y) vs oracle", full, xo, XTOL)
    if want is not None:
        assert len(ran) == 1 and ran <= set(want), (ran, sorted(launch_sites(t)))
    else:
        assert ran, sorted(launch_sites(t))                              # a fused tier, whichever
    if n == 1:                                                           # windows are really cut: no halo, a visible seam
        with torch.no_grad():
            bare = cva.denoise_windowed(net, y, sigma, mask, window=window, halo=0)
        seam = rel_err(bare, full)
        log(f"windowed case 1 halo=0 differs from net(y) by rel {seam:.3e}")
        assert seam > 1e-3


def test_approximate_temporal_halo_with_the_ramp():
    import cdlnet_video_amd as cva
    net, y, sigma, mask, full, _ = case(4)
    halo, R = (1, 4, 4), 4
    with torch.no_grad():
        got = cva.denoise_windowed(net, y, sigma, mask, window=(6, None, None), halo=halo, blend="ramp")
    assert bool(torch.isfinite(got).all())
    axis = cva.windowed.plan_axis(y.shape[2], 6, halo[0])
    L = y.shape[2]
    exact = []
    for d in range(L):
        inside = [a for a in axis if a.w0 <= d < a.w1]
        if len(inside) == 1 and all((a.w0 == 0 or d - a.w0 >= R) and (a.w1 == L or a.w1 - 1 - d >= R) for a in inside):
            exact.append(d)
    assert exact == [0, 1, 2, 3, 19]          # frames outside every overlap and at least R from their window's cut edges
    check("windowed case 4 ramp, frames off the seams", got[:, :, exact], full[:, :, exact], XTOL)
    log(f"windowed case 4 halo {halo} ramp: PSNR against net(y) {O.psnr(full.cpu(), got.cpu()):.2f} dB, "
        f"worst rel err {rel_err(got, full):.3e}")


def test_sigma_map_is_cropped_per_window_and_runs_the_generic_tier():
    import cdlnet_video_amd as cva
    net, y, _, _, _, _ = case(1)
    amap = smooth_map((2, 1, 96, 80), 7).cuda()
    with torch.no_grad():
        full = net(y, amap)[0]
        with cva.ops.trace() as t:
            got = cva.denoise_windowed(net, y, amap, window=(32, 32), halo=4)
            torch.cuda.synchronize()
    assert t and not (t.files() & FUSED_FILES), t.files()
    check("windowed map vs net(y, map)", got, full, XTOL)


def test_one_window_is_net_of_y_bit_for_bit():
    import cdlnet_video_amd as cva
    for n in (1, 2):
        net, y, sigma, mask, full, _ = case(n)
        with torch.no_grad():
            assert torch.equal(cva.denoise_windowed(net, y, sigma, mask), full)                  # the automatic plan
            assert torch.equal(cva.denoise_windowed(net, y, sigma, mask, window=(None, None), halo=0), full)


def test_batch_grouping_does_not_change_the_result():
    import cdlnet_video_amd as cva
    for n in (1, 4):
        window, halo = CASES[n][4:6]
        net, y, sigma, mask, _, _ = case(n)
        with torch.no_grad():
            one = cva.denoise_windowed(net, y, sigma, mask, window=window, halo=halo, max_batch=1)
            some = cva.denoise_windowed(net, y, sigma, mask, window=window, halo=halo, max_batch=5)
            every = cva.denoise_windowed(net, y, sigma, mask, window=window, halo=halo)
        log(f"windowed case {n} max_batch=1 vs one batch: bit-identical: {torch.equal(one, every)}")
        check(f"windowed case {n} max_batch=1 vs one batch", one, every, 1e-6)
        check(f"windowed case {n} max_batch=5 vs one batch", some, every, 1e-6)
