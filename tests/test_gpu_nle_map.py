"""Local MAD noise-level estimates on the device (cdl_nle_mad_cells, cva.nle.nle_mad_cells / nle_mad_map /
nle_mad_frames) against the restatement tests/nle_map_restate.py, bit equality with nle_mad where
the definition promises it, and the blind map end to end through CDLNet."""
import pytest
import torch

import nle_map_restate as R
from sigmamap_util import smooth_map

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the tolerance tests/test_nle.py uses for the same band


def _noisy(shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.rand(shape, generator=g) + torch.randn(shape, generator=g) * 0.1


CASES = [  # shape, window, step
    ((3, 1, 64, 64), 32, None), ((2, 3, 37, 53), 32, None), ((1, 1, 10, 10), 32, None), ((2, 1, 256, 256), 32, None),
    ((5, 2, 11, 90), 32, None),
    ((3, 1, 64, 64), 8, None), ((2, 3, 37, 53), 6, 3), ((5, 2, 11, 90), 16, None),
    ((2, 1, 6, 40, 72), 8, None),                # a clip
    ((1, 3, 300, 300), 128, None),               # 3 x 128 x 128 samples a cell: too large for LDS, read from the band
    ((2, 1, 256, 256), 32, 11), ((2, 1, 120, 97), 20, 7),       # steps that are not w / 2
]


@pytest.mark.parametrize("shape,w,q", CASES, ids=[f"{'x'.join(map(str, c[0]))}-w{c[1]}-q{c[2]}" for c in CASES])
def test_cells_and_map_equal_the_restatement(shape, w, q):
    import cdlnet_video_amd as cva
    from gpu_util import check
    y = _noisy(shape)
    ref = R.cells(y, w, q)
    got = cva.nle.nle_mad_cells(y.cuda(), w, q)
    assert got.shape == ref.shape
    check(f"nle_mad_cells {shape} w={w} q={q}", got, ref, TOL)
    assert float(((got.cpu() - ref).abs() / ref).max()) < TOL            # every cell, not only the largest
    ref_map = R.image_map(y, w, q)
    got_map = cva.nle.nle_mad_map(y.cuda(), w, q)
    assert got_map.shape == ref_map.shape == (shape[0], 1) + tuple(shape[2:])
    check(f"nle_mad_map {shape} w={w} q={q}", got_map, ref_map, TOL)
    assert float(((got_map.cpu() - ref_map).abs() / ref_map).max()) < TOL
    assert torch.equal(got, cva.nle.nle_mad_cells(y.cuda(), w, q))       # a second call returns the same bits
    assert torch.equal(got_map, cva.nle.nle_mad_map(y.cuda(), w, q))


@pytest.mark.parametrize("shape,s", [((2, 1, 51, 77), 2), ((1, 3, 64, 40), 2), ((2, 1, 6, 40, 72), 2)])
def test_code_grid(shape, s):
    import cdlnet_video_amd as cva
    from gpu_util import check
    y = _noisy(shape)
    ref = R.code_map(y, 8, 4, s)
    got = cva.nle.nle_mad_map(y.cuda(), 8, 4, s=s)
    assert got.shape == ref.shape == (shape[0], 1) + tuple(-(-d // s) for d in shape[2:])
    check(f"nle_mad_map {shape} s={s}", got, ref, TOL)


@pytest.mark.parametrize("shape", [(3, 1, 64, 64), (2, 3, 37, 53), (1, 1, 10, 10), (2, 1, 256, 256), (5, 2, 11, 90),
                                   (1, 3, 300, 300)])
def test_whole_band_window_has_the_bits_of_nle_mad(shape):
    import cdlnet_video_amd as cva
    y = _noisy(shape).cuda()
    glob = cva.nle.nle_mad(y)
    w = max((shape[2] - 10) // 2 + 1, (shape[3] - 10) // 2 + 1, 2)
    for window in (w, w + 5, 4096):
        cells = cva.nle.nle_mad_cells(y, window)
        assert cells.shape == glob.shape and torch.equal(cells, glob)
        assert torch.equal(cva.nle.nle_mad_map(y, window), glob.expand(shape[0], 1, shape[2], shape[3]))
    assert torch.equal(cva.nle.nle_mad_map(y, window=None), glob)


@pytest.mark.parametrize("shape", [(2, 1, 6, 40, 72), (2, 3, 4, 33, 20), (1, 1, 3, 256, 256)])
def test_frames_have_the_bits_of_nle_mad(shape):
    import cdlnet_video_amd as cva
    clip = _noisy(shape).cuda()
    got = cva.nle.nle_mad_frames(clip)
    assert got.shape == (shape[0], 1, shape[2], 1, 1)
    for d in range(shape[2]):
        assert torch.equal(got[:, :, d], cva.nle.nle_mad(clip[:, :, d].contiguous()))
    assert torch.equal(got, cva.nle.nle_mad_frames(clip))
    assert torch.equal(got, cva.nle.nle_mad_map(clip, window=None))
    assert float(((got.cpu() - R.frames(clip.cpu())).abs() / R.frames(clip.cpu())).max()) < TOL
    cells = cva.nle.nle_mad_cells(clip, 8)                                 # frames are never mixed
    for d in range(shape[2]):
        assert torch.equal(cells[:, :, d], cva.nle.nle_mad_cells(clip[:, :, d].contiguous(), 8))


def test_refusals_and_unchanged_contracts():
    import cdlnet_video_amd as cva
    y = _noisy((2, 1, 40, 40)).cuda()
    for fn in (cva.nle.nle_mad_cells, cva.nle.nle_mad_map):
        with pytest.raises(ValueError, match="smaller"):
            fn(y[:, :, :9])
        with pytest.raises(ValueError, match="window"):
            fn(y, window=1)
        with pytest.raises(ValueError, match="step"):
            fn(y, window=8, step=0)
        with pytest.raises(ValueError, match="expects"):
            fn(y[0])
        with pytest.raises(ValueError, match="expects"):
            fn(y[None, None])
    with pytest.raises(ValueError):
        cva.nle.nle_mad_frames(y)
    with pytest.raises(ValueError, match="smaller"):
        cva.nle.nle_mad_frames(y[:, :, None, :, :9])
    clip = _noisy((2, 1, 3, 40, 40)).cuda()
    with pytest.raises(ValueError, match=r"nle_mad expects \(N, C, H, W\)"):   # nle_mad and noise_level stay 4-D only
        cva.nle.nle_mad(clip)
    with pytest.raises(ValueError):
        cva.nle.noise_level(clip)
    with pytest.raises(NotImplementedError):
        cva.nle.noise_level(y, method="PCA")


def test_no_host_synchronisation():
    import cdlnet_video_amd as cva
    y, clip = _noisy((2, 1, 96, 80)).cuda(), _noisy((2, 1, 4, 40, 72)).cuda()
    cva.nle.nle_mad_map(y, 16, s=2)                # first call: library load, scratch allocation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):          # the hook is live: a device-to-host read is refused
            torch.ones(1, device="cuda").item()
        a = cva.nle.nle_mad_map(y, 16, s=2)
        b = cva.nle.nle_mad_map(y, 24, 5)          # an interpolation plan not seen before
        c = cva.nle.nle_mad_cells(clip, 8)
        d = cva.nle.nle_mad_frames(clip)
        e = cva.nle.nle_mad_map(clip, 8, s=2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(bool(torch.isfinite(t).all()) for t in (a, b, c, d, e))


@pytest.mark.parametrize("s,shape", [(1, (2, 1, 256, 256)), (2, (2, 1, 255, 241))])
def test_blind_map_end_to_end(s, shape):
    """net(y, 255 * nle_mad_map(y, s=net.s)): the net takes the map's shape, and the result is closer (rms) to the
    one under the true map than the result under the single global estimate is.  The ratio and the PSNRs are logged.
    The same nets, seeds and inputs through the CPU oracle with the restated map: 2.16 x (s = 1) and 2.35 x (s = 2,
    255 x 241), PSNR equal to 0.005 dB between the three."""
    import cdlnet_video_amd as cva
    from gpu_util import log
    torch.manual_seed(6)
    net = cva.CDLNet(K=6, M=32, P=7, s=s, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    x = cva.utils.synthetic_clip(shape, seed=3)
    true_map = smooth_map(shape, 7)
    y = (x + torch.randn(shape, generator=torch.Generator().manual_seed(11)) * true_map / 255).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        est = 255 * cva.nle.nle_mad_map(y, s=net.s)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert est.shape == (shape[0], 1, -(-shape[2] // s), -(-shape[3] // s))
    with torch.no_grad():
        x_est, _ = net(y, est)
        x_true, _ = net(y, cva.utils.sigma_to_code_grid(true_map.cuda(), s))
        x_glob, _ = net(y, 255 * cva.nle.nle_mad(y))
    rms = lambda a, b: float((a - b).pow(2).mean().sqrt())
    d_est, d_glob = rms(x_est, x_true), rms(x_glob, x_true)
    psnr = [cva.utils.psnr(x.cuda(), v) for v in (x_true, x_est, x_glob)]
    line = (f"blind map end to end s={s} {shape}: rms to the true-map result {d_est:.3e} (local map) {d_glob:.3e} "
            f"(global), ratio {d_glob / d_est:.2f}; PSNR true/local/global {psnr[0]:.3f}/{psnr[1]:.3f}/{psnr[2]:.3f}")
    log(line)
    print(line)
    assert x_est.shape == x.shape and torch.isfinite(x_est).all()
    assert d_est < d_glob
