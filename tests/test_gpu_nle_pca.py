"""Weak-texture PCA noise estimate on the device: cdl_nle_pca_gram through the C ABI and nle_pca against the float64
restatement (nle_pca_restate.py) and the fixtures of the unmodified reference."""
import math

import numpy as np
import pytest
import torch

import nle_pca_restate as R

pytestmark = pytest.mark.gpu


def _gram(y, c, p, tau):
    import cdlnet_video_amd as cva
    g, n = cva.nle.pca_gram(y.cuda().contiguous(), c, p, tau)
    return g.cpu(), n


@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
@pytest.mark.parametrize("finite", [False, True])
def test_gram_entry_point_matches_restatement(name, finite):
    f = R.load(name)
    y, p = torch.from_numpy(f["y"]), int(f["patchsize"])
    tau = math.inf
    if finite:
        tau, _ = R.gap_threshold(R.texture(y[:, 0], p), 0.5)
    ref, nref = R.gram(y[:, 0], p, tau)
    got, n = _gram(y, 0, p, tau)
    assert n == nref
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < 1e-6, err
    assert torch.equal(got, got.T)


def _check_against_fixture(f, got):
    nlevel, th, num = float(f["nlevel"]), float(f["th"]), float(f["num"])
    if nlevel == 0.0:
        assert (float(got[0]), float(got[1]), float(got[2])) == (0.0, 0.0, 0.0)
        return
    assert abs(got[0] / nlevel - 1) < 1e-3 and abs(got[1] / th - 1) < 1e-3, (got, (nlevel, th, num))
    assert abs(got[2] - num) <= max(2, 1e-3 * num), (got[2], num)


@pytest.mark.parametrize("name", R.CASES)
def test_estimator_matches_restatement_and_reference(name):
    import cdlnet_video_amd as cva
    f = R.load(name)
    y, p, conf, itr = torch.from_numpy(f["y"]), int(f["patchsize"]), float(f["conf"]), int(f["itr"])
    got = cva.nle.nle_pca(y.cuda(), patchsize=p, conf=conf, itr=itr)
    assert all(type(v) is np.float64 for v in got)                 # the reference's types for C = 1
    ref = R.estimate(y, p, cva.nle.pca_constants(p, conf)[0], itr)[:, 0]
    if ref[0] == 0.0:
        assert tuple(got) == (0.0, 0.0, 0.0)
    else:
        assert abs(got[0] / ref[0] - 1) < 1e-5, (got, ref)
        assert abs(got[1] / ref[1] - 1) < 1e-5, (got, ref)
        assert abs(got[2] - ref[2]) <= max(2, 1e-3 * ref[2]), (got, ref)
    _check_against_fixture(f, got)


def test_itr_two_skips_refinement():
    import cdlnet_video_amd as cva
    f = R.load("n1")
    y = torch.from_numpy(f["y"])
    got = cva.nle.nle_pca(y.cuda(), itr=2)
    ref = R.estimate(y, 7, cva.nle.pca_constants(7)[0], 2)[:, 0]
    assert got[1] == math.inf and got[2] == 58 * 58
    assert abs(got[0] / ref[0] - 1) < 1e-5


def test_repeated_calls_are_bit_identical():
    import cdlnet_video_amd as cva
    y = torch.from_numpy(R.load("n3")["y"]).cuda()
    g1, n1 = cva.nle.pca_gram(y, 0, 7, math.inf)
    g2, n2 = cva.nle.pca_gram(y, 0, 7, math.inf)
    assert n1 == n2 and torch.equal(g1, g2)
    assert cva.nle.nle_pca(y) == cva.nle.nle_pca(y)


def test_channels_are_independent():
    import cdlnet_video_amd as cva
    y = torch.from_numpy(R.load("n6")["y"])
    y3 = torch.cat([y, 0.5 * y.flip(2), y.flip(3) + 0.1], dim=1).contiguous().cuda()
    got = cva.nle.nle_pca(y3)
    assert all(isinstance(v, np.ndarray) and v.shape == (3,) and v.dtype == np.float64 for v in got)
    for c in range(3):
        one = cva.nle.nle_pca(y3[:, c:c + 1].contiguous())
        assert tuple(v[c] for v in got) == one, c


def test_large_batch_count_is_exact():
    """N = 300 at 256 x 256: 18.7 M patches (> 2^24) in one pass."""
    import cdlnet_video_amd as cva
    N, H, W = 300, 256, 256
    g = torch.Generator().manual_seed(3)
    i, j = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.25 * torch.sin(3.0 * i + 2.0 * j)
    off = torch.rand(N, 1, 1, 1, generator=g) * 0.2
    y = (base + off + torch.randn(N, 1, H, W, generator=g) * 15 / 255).float()
    xtr = R.texture(y[:, 0], 7)
    assert xtr.numel() == N * 250 * 250 > 2 ** 24
    tau, nref = R.gap_threshold(xtr, 0.99, 0.9995)      # sparse enough for a clear gap
    del xtr
    yd = y.cuda()
    _, n_all = cva.nle.pca_gram(yd, 0, 7, math.inf)
    _, n = cva.nle.pca_gram(yd, 0, 7, tau)
    assert n_all == N * 250 * 250 and n == nref
    nlevel = cva.nle.nle_pca(yd)[0]
    assert abs(255 * nlevel / 15 - 1) < 0.05, 255 * nlevel


def test_estimate_feeds_an_adaptive_net():
    """The reference's blind inference with --blind PCA: sigma = 255 * nle_pca(y)[0] (its noise_level(y, "PCA"))."""
    import cdlnet_video_amd as cva
    torch.manual_seed(0)
    net = cva.CDLNet(K=3, M=16, P=7, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    y = torch.from_numpy(R.load("n1")["y"]).cuda()
    s = 255 * cva.nle.nle_pca(y)[0]
    assert type(s) is np.float64 and 15 < s < 30
    with torch.no_grad():
        a, _ = net(y, s)
        b, _ = net(y, float(s))
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match=r"nle_pca\(y\)\[0\]"):   # noise_level stays MAD-only
        cva.nle.noise_level(y, "PCA")


def test_bad_input():
    import cdlnet_video_amd as cva
    with pytest.raises(ValueError, match="smaller than"):
        cva.nle.nle_pca(torch.zeros(1, 1, 6, 32, device="cuda"))
    with pytest.raises(ValueError, match="smaller than"):
        cva.nle.nle_pca(torch.zeros(1, 1, 32, 10, device="cuda"), patchsize=11)
    with pytest.raises(ValueError, match="outside 3..11"):
        cva.nle.nle_pca(torch.zeros(1, 1, 32, 32, device="cuda"), patchsize=13)
    with pytest.raises(ValueError, match=r"\(N, C, H, W\)"):
        cva.nle.nle_pca(torch.zeros(1, 1, 4, 32, 32, device="cuda"))
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.nle.nle_pca(torch.zeros(1, 1, 32, 32))
    with pytest.raises(TypeError):
        cva.nle.nle_pca(torch.zeros(1, 1, 32, 32, device="cuda", dtype=torch.float64))


@pytest.mark.parametrize("p", [3, 4, 8, 9, 11])
def test_other_patch_sizes(p):
    """Odd and even p, both paddings (p^2 + 1 <= 64 and <= 128)."""
    import cdlnet_video_amd as cva
    y = torch.from_numpy(R.load("n5")["y"])
    for tau in (math.inf, R.gap_threshold(R.texture(y[:, 0], p), 0.4)[0]):
        ref, nref = R.gram(y[:, 0], p, tau)
        got, n = _gram(y, 0, p, tau)
        assert n == nref
        assert float((got - ref).abs().max() / ref.abs().max()) < 1e-6
    tau0 = cva.nle.pca_constants(p)[0]
    got, ref = cva.nle.nle_pca(y.cuda(), patchsize=p, itr=2), R.estimate(y, p, tau0, 2)[:, 0]
    assert abs(got[0] / ref[0] - 1) < 1e-5, (got, ref)
    # refined: the fp32 texture strengths may put one patch on the other side of tau than float64 does, and one patch
    # of ~5000 moves sig2 by ~1e-4, so the reference's own tolerances apply
    got, ref = cva.nle.nle_pca(y.cuda(), patchsize=p, itr=4), R.estimate(y, p, tau0, 4)[:, 0]
    assert abs(got[0] / ref[0] - 1) < 1e-3 and abs(got[2] - ref[2]) <= max(2, 1e-3 * ref[2]), (got, ref)
