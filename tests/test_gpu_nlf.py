"""The blind noise-level function on the device (cdl_nle_nlf_bins, cva.nle.nlf_bins / nlf_fit / nlf_map; DESIGN.md
section 29) against tests/nlf_restate.py, in two stages so that no comparison depends on which side of a bin edge a
float lands: the two bands the device forms against the restated bands, then the device's selection against the restated
binning of the device's OWN bands, bit for bit.  Then the fit and the map on the device's bins, routing, and the map end
to end through CDLNet."""
import numpy as np
import pytest
import torch

import nlf_restate as R

pytestmark = pytest.mark.gpu

A0, B0 = 0.01, (5 / 255) ** 2


def _ramp(shape, seed=0):
    """The ramp content of the accuracy tests with signal-dependent noise, every channel and image its own seed."""
    N, C, H, W = shape
    imgs = [R.noisy(H, W, seed + i, A0, B0)[1] for i in range(N * C)]
    return torch.tensor(np.stack(imgs), dtype=torch.float32).reshape(shape)


SHAPES = [(1, 1, 10, 10),            # a band of one sample
          (2, 3, 37, 41), (1, 1, 64, 300),
          (1, 3, 150, 150)]          # 3 x 71 x 71 samples an image: too many for LDS, the bins read the band on every pass
CONSTANTS = {"edge": 0.5,            # every m is exactly the lower edge of bin 16 of 32: it belongs to bin 16
             "hi": 1.0}              # m == hi: no bin has a member
_INPUTS = {}


def _input(case):
    """Built once per case and never changed."""
    if case not in _INPUTS:
        _INPUTS[case] = torch.full((2, 1, 20, 24), CONSTANTS[case]) if case in CONSTANTS else _ramp(case, seed=sum(case))
    return _INPUTS[case]


def _device_bands(y, bins=32, lo=0.0, hi=1.0):
    """One cdl_nle_nlf_bins call on a scratch of the test's own: (d, m, sigma, count) on the host, d and m (N,C,Hb,Wb)
    the two bands the call left in its scratch."""
    import cdlnet_video_amd as cva
    N, C, H, W = y.shape
    n = int(cva._lib.lib().cdl_nle_nlf_bins_scratch_floats(N, C, H, W))
    scratch = torch.zeros(n, device="cuda")
    sigma = torch.full((N, bins), -1.0, device="cuda")
    count = torch.full((N, bins), -1, device="cuda", dtype=torch.int32)
    cva.ops._call("cdl_nle_nlf_bins", y.cuda(), sigma, count, scratch, n, N, C, H, W, bins, lo, hi)
    band = (N, C, (H - 10) // 2 + 1, (W - 10) // 2 + 1)
    return scratch[:n // 2].reshape(band).cpu(), scratch[n // 2:].reshape(band).cpu(), sigma.cpu(), count.cpu()


# ------------------------------------------------------------------------------------------------ stage 1: the bands
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_stage1_bands(shape):
    import cdlnet_video_amd as cva
    y = _input(shape)
    N, C, H, W = shape
    d, m, _, _ = _device_bands(y)
    # d is the band cdl_nle_mad_cells forms, bit for bit ...
    n1 = int(cva._lib.lib().cdl_nle_mad_cells_scratch_floats(N, C, H, W))
    scratch, cells = torch.zeros(n1, device="cuda"), torch.zeros(N, device="cuda")
    whole = max(d.shape[2], d.shape[3], 2)
    cva.ops._call("cdl_nle_mad_cells", y.cuda(), cells, scratch, n1, N, C, H, W, whole, whole)
    assert torch.equal(scratch.reshape(d.shape).cpu(), d)
    # ... and a whole-band window still returns nle_mad's bits, which are the lower median of this band
    glob = cva.nle.nle_mad(y.cuda())
    assert torch.equal(cells.reshape(-1, 1, 1, 1), glob) and torch.equal(cva.nle.nle_mad_cells(y.cuda(), whole), glob)
    assert torch.equal((torch.median(d.reshape(N, -1), dim=1)[0] / 0.6745).reshape(-1, 1, 1, 1), glob.cpu())
    for n in range(N):
        d_ref, m_ref = R.bands(y[n].numpy())
        err_m = float(np.abs(m[n].double().numpy() - m_ref).max())
        err_d = float(np.abs(d[n].double().numpy() - d_ref).max() / d_ref.max())
        print(f"nlf bands {shape} image {n}: max |m - restated| {err_m:.3e}, d rel err {err_d:.3e}")
        assert err_m < 1e-6
        assert err_d < 1e-5                                  # the tolerance of tests/test_nle.py for the same band


# ------------------------------------------------------------------------------------------------ stage 2: the selection
def _restated_bins(d, m, bins, lo, hi):
    """The restated binning of the device's own bands, the bin index in float32: (sigma (N, bins) float32, count int32)."""
    out = [R.bin_stats(d[n].numpy(), m[n].numpy(), bins, lo, hi, f32=True) for n in range(d.shape[0])]
    assert all(o[0].dtype == np.float32 for o in out)
    return torch.tensor(np.stack([o[0] for o in out])), torch.tensor(np.stack([o[1] for o in out]), dtype=torch.int32)


STAGE2 = [(s, 32, 0.0, 1.0) for s in SHAPES] + [("edge", 32, 0.0, 1.0), ("hi", 32, 0.0, 1.0),
                                                ((2, 3, 37, 41), 7, 0.1, 0.9), ((2, 3, 37, 41), 1, -1.0, 2.0),
                                                ((1, 3, 150, 150), 5, 0.25, 0.8)]


@pytest.mark.parametrize("case,bins,lo,hi", STAGE2,
                         ids=[f"{c if isinstance(c, str) else 'x'.join(map(str, c))}-{b}-{lo}-{hi}" for c, b, lo, hi in STAGE2])
def test_stage2_selection_equals_the_restated_bins_of_the_devices_bands(case, bins, lo, hi):
    import cdlnet_video_amd as cva
    y = _input(case)
    d, m, sigma, count = _device_bands(y, bins, lo, hi)
    ref_sigma, ref_count = _restated_bins(d, m, bins, lo, hi)
    assert sigma.shape == ref_sigma.shape == (y.shape[0], bins)          # every (image, bin) pair is compared
    assert torch.equal(count, ref_count)
    assert torch.equal(sigma, ref_sigma)
    per_image = d[0].numel()
    if case == "edge":
        assert count[:, 16].tolist() == [per_image] * 2 and int(count.sum()) == 2 * per_image
    elif case == "hi":
        assert not count.any() and not sigma.any()
    elif (lo, hi) == (-1.0, 2.0):
        assert count[:, 0].tolist() == [per_image] * y.shape[0]          # one bin holds the band: the MAD estimate
        assert torch.equal(sigma.reshape(-1, 1, 1, 1), cva.nle.nle_mad(y.cuda()).cpu())
    else:
        assert int(count.sum()) > 0
    s2, c2, centre = cva.nle.nlf_bins(y.cuda(), bins, lo, hi)            # the public call, and a second call: same bits
    assert s2.shape == c2.shape == (y.shape[0], 1, bins) and c2.dtype == torch.int32
    assert torch.equal(s2.cpu().reshape(sigma.shape), sigma) and torch.equal(c2.cpu().reshape(count.shape), count)
    assert torch.equal(centre.cpu(), torch.from_numpy(R.bin_stats(d[0].numpy(), m[0].numpy(), bins, lo, hi)[2]))


# ------------------------------------------------------------------------------------------------ fit and map
def test_fit_on_the_device_is_fit_bins_of_the_bins():
    import cdlnet_video_amd as cva
    y = _ramp((2, 1, 128, 192), seed=0).cuda()
    sigma, count, centre = cva.nle.nlf_bins(y)
    a, b = cva.nle.nlf_fit(y)
    mad2 = cva.nle.nle_mad(y).double().reshape(2, 1) ** 2
    a2, b2 = cva.nle.nlf_fit_bins(sigma, count, centre, fallback=mad2)
    assert a.shape == b.shape == (2, 1, 1, 1) and a.dtype == torch.float32
    assert torch.equal(a.reshape(2, 1), a2.float()) and torch.equal(b.reshape(2, 1), b2.float())
    for n in range(2):                                       # and the restated fit of the same bins, to fp32 rounding
        ra, rb = R.fit(sigma[n, 0].cpu().numpy(), count[n, 0].cpu().numpy(), centre.cpu().numpy())
        assert abs(float(a[n]) - ra) <= 1e-6 * ra and abs(float(b[n]) - rb) <= 1e-6 * max(rb, 1e-6)
        xs = np.linspace(0.1, 0.9, 9)
        rel = np.sqrt(float(a[n]) * xs + float(b[n])) / np.sqrt(A0 * xs + B0) - 1
        print(f"nlf_fit image {n}: a {float(a[n]):.5f} (true {A0}) b {float(b[n]):.3e} (true {B0:.3e}), worst sigma error {np.abs(rel).max():.3f}")
    few = cva.nle.nlf_fit(_input((1, 1, 10, 10)).cuda())     # one band sample: no usable bin, the MAD estimate squared
    assert float(few[0]) == 0.0
    assert torch.equal(few[1], cva.nle.nle_mad(_input((1, 1, 10, 10)).cuda()) ** 2)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("fit_kw", [{}, {"bins": 8, "min_count": 4}], ids=["defaults", "8bins"])
def test_map_agrees_with_the_restated_map(s, fit_kw):
    """The restated map of the device's (a, b): whatever side of an edge a sample of the device's band landed on, the
    map is compared on the same pair.  (Stage 2 and the fit tests tie the pair to the restatement.)"""
    import cdlnet_video_amd as cva
    from gpu_util import check
    shape = (2, 1, 37, 41)
    y = _ramp(shape, seed=5)
    yd = y.cuda()
    cva.nle.nlf_map(yd, s=s, **fit_kw)                       # first call: scratch allocation
    cva.nle.nlf_map(yd.reshape(1, 1, 2, 37, 41), s=s, **fit_kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                    # the hook is live: a device-to-host read is refused
            torch.ones(1, device="cuda").item()
        a, b = cva.nle.nlf_fit(yd, **fit_kw)
        got = cva.nle.nlf_map(yd, s=s, **fit_kw)
        given = cva.nle.nlf_map(yd, a, b, s=s)
        clip = cva.nle.nlf_map(yd.reshape(1, 1, 2, 37, 41), s=s, **fit_kw)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert got.shape == (2, 1, -(-37 // s), -(-41 // s)) and torch.equal(got, given)
    assert clip.shape == (1, 1, 1 if s == 2 else 2) + tuple(got.shape[2:])
    if s == 1:
        assert torch.equal(clip[0, 0], got[:, 0])            # a clip is its frames, each with its own fit
    if fit_kw:
        assert float(a.min()) > 0 or float(b.min()) > 0      # a fit, not the fallback
    maps = np.stack([R.image_map(y[n].numpy(), float(a[n]), float(b[n])) for n in range(2)])
    ref = cva.utils.sigma_to_code_grid(torch.from_numpy(maps)[:, None], s).float()
    check(f"nlf_map {shape} s={s} {fit_kw}", got, ref, 1e-6)
    assert float(((got.cpu() - ref).abs() / ref).max()) < 1e-6           # every pixel, not only the largest


def test_pooled_clip_is_the_fit_of_its_frames_as_channels():
    import cdlnet_video_amd as cva
    clip = _ramp((1, 3, 24, 28), seed=9).reshape(1, 1, 3, 24, 28).cuda()
    kw = dict(bins=8, min_count=4)
    stacked = clip.reshape(1, 3, 24, 28)
    sp, cp, _ = cva.nle.nlf_bins(clip, 8, pool_frames=True)
    ss, cs, _ = cva.nle.nlf_bins(stacked, 8)
    assert sp.shape == (1, 1, 8) and torch.equal(sp, ss) and torch.equal(cp, cs) and int(cp.sum()) > 0
    a, b = cva.nle.nlf_fit(clip, pool_frames=True, **kw)
    a2, b2 = cva.nle.nlf_fit(stacked, **kw)
    assert a.shape == b.shape == (1, 1, 1, 1, 1)
    assert torch.equal(a.reshape(-1), a2.reshape(-1)) and torch.equal(b.reshape(-1), b2.reshape(-1))
    assert float(a) > 0 or float(b) > 0
    per_frame = cva.nle.nlf_bins(clip, 8)                     # without pooling every frame has its own bins
    assert per_frame[0].shape == (1, 1, 3, 8) and torch.equal(per_frame[1].sum(dim=2).int(), cp)
    for d in range(3):
        one = cva.nle.nlf_bins(clip[:, :, d].contiguous(), 8)
        assert torch.equal(per_frame[0][:, :, d], one[0]) and torch.equal(per_frame[1][:, :, d], one[1])
    assert cva.nle.nlf_fit(clip, **kw)[0].shape == (1, 1, 3, 1, 1)
    assert cva.nle.nlf_map(clip, pool_frames=True, **kw).shape == (1, 1, 3, 24, 28)


# ------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("shape,staged", [((2, 3, 37, 41), "true"), ((1, 3, 150, 150), "false")])
def test_routing(shape, staged):
    import cdlnet_video_amd as cva
    from gpu_util import launch_sites
    y = _input(shape).cuda()
    with cva.ops.trace() as t:
        cva.nle.nlf_bins(y)
    sites = launch_sites(t)
    assert sorted(sites) == ["cdl_nle.hip:k_hh_abs#2", f"cdl_nle.hip:k_select_cells<{staged}>"]
    assert len(t) == 2 and "keyed" in t[1].note


def test_refusals_on_the_device():
    import cdlnet_video_amd as cva
    y = _input((2, 3, 37, 41)).cuda()
    for fn in (cva.nle.nlf_bins, cva.nle.nlf_fit, cva.nle.nlf_map):
        with pytest.raises(ValueError, match="smaller"):
            fn(y[:, :, :9])
        with pytest.raises(ValueError, match="expects"):
            fn(y[0])
        with pytest.raises(ValueError, match="expects"):
            fn(y[None, None])
        with pytest.raises(ValueError, match="bins"):
            fn(y, bins=0)
        with pytest.raises(ValueError, match="hi"):
            fn(y, lo=1.0, hi=0.0)
    with pytest.raises(ValueError, match="smooth"):
        cva.nle.nlf_map(y, smooth=6)
    with pytest.raises(ValueError, match="smooth"):
        cva.nle.nlf_map(y, 0.01, 0.0, smooth=99)             # a reflect padding wider than the image


# ------------------------------------------------------------------------------------------------ end to end
def test_blind_nlf_map_end_to_end():
    """net(y, 255 * nlf_map(y)) under signal-dependent noise: the result is closer (rms) to the one under the true map
    255 sqrt(a0 x + b0) than the result under the single nle_mad value is.  The same net, seed and input through the CPU
    oracle with the restated map: 9.37 x closer."""
    import cdlnet_video_amd as cva
    from gpu_util import log
    torch.manual_seed(6)
    net = cva.CDLNet(K=4, M=16, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    pairs = [R.noisy(128, 192, seed, A0, B0) for seed in (0, 1)]
    x = torch.tensor(np.stack([p[0] for p in pairs]), dtype=torch.float32)[:, None].cuda()
    y = torch.tensor(np.stack([p[1] for p in pairs]), dtype=torch.float32)[:, None].cuda()
    true_map = 255 * torch.sqrt(A0 * x + B0)
    with torch.no_grad():
        x_est, _ = net(y, 255 * cva.nle.nlf_map(y, s=net.s))
        x_true, _ = net(y, true_map)
        x_glob, _ = net(y, 255 * cva.nle.nle_mad(y))
    rms = lambda u, v: float((u - v).pow(2).mean().sqrt())
    d_est, d_glob = rms(x_est, x_true), rms(x_glob, x_true)
    line = (f"blind nlf map end to end: rms to the true-map result {d_est:.3e} (nlf map) {d_glob:.3e} (one MAD level), "
            f"ratio {d_glob / d_est:.2f}")
    log(line)
    print(line)
    assert x_est.shape == x.shape and torch.isfinite(x_est).all()
    assert d_est < d_glob
