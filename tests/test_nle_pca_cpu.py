"""Weak-texture PCA noise estimate (nle_pca), the parts that need no GPU: the float64 restatement in
nle_pca_restate.py against the fixtures of the unmodified reference (tools/make_golden_nle_pca.py), and the
package's cached constants of the patch size against the fixtures and scipy."""
import numpy as np
import pytest
import torch

import nle_pca_restate as R


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_reproduces_reference(name):
    f = R.load(name)
    got = R.estimate(torch.from_numpy(f["y"]), int(f["patchsize"]), float(f["tau0"]), int(f["itr"]))[:, 0]
    nlevel, th, num = float(f["nlevel"]), float(f["th"]), float(f["num"])
    if name == "n4":                                    # N (H-p+1) (W-p+1) = 24 < 49 patches: the zero path
        assert (nlevel, th, num) == (0.0, 0.0, 0.0) and tuple(got) == (0.0, 0.0, 0.0)
        return
    assert num >= int(f["patchsize"]) ** 2, "the fixture should exercise the refinement"
    assert abs(got[0] / nlevel - 1) < 1e-3, (got[0], nlevel)
    assert abs(got[1] / th - 1) < 1e-3, (got[1], th)
    assert abs(got[2] - num) <= max(2, 1e-3 * num), (got[2], num)


@pytest.mark.parametrize("name", R.CASES)
def test_package_constants_match_fixture(name):
    import cdlnet_video_amd as cva
    f = R.load(name)
    tau0, r, tr = cva.nle.pca_constants(int(f["patchsize"]), float(f["conf"]))
    assert r == int(f["r"]) and tr == float(f["trDD"])
    assert abs(tau0 / float(f["tau0"]) - 1) < 1e-10        # the fixture's tau0 is scipy's gamma.ppf


@pytest.mark.parametrize("p", [3, 4, 5, 6, 7, 8, 9, 10, 11])
@pytest.mark.parametrize("conf", [1 - 1e-9, 1 - 1e-6, 0.999, 0.99])
def test_tau0_equals_scipy_gamma_ppf(p, conf):
    """Confidence levels of a texture threshold (far upper tail).  Nearer the middle (conf = 0.9) torch's own
    gammaincc is ~1e-10 off scipy's, and so is the bisected quantile."""
    import cdlnet_video_amd as cva
    gamma = pytest.importorskip("scipy.stats").gamma
    tau0, r, tr = cva.nle.pca_constants(p, conf)
    assert abs(tau0 / gamma.ppf(conf, r / 2.0, scale=2.0 * tr / r) - 1) < 1e-10


def test_constants_follow_the_derivative_matrices():
    """tr(DD) = 2 p (p-2) (each row of Dh, Dv holds two entries of 1/2); for p = 7 the reference's r = 45."""
    import cdlnet_video_amd as cva
    for p in range(3, 12):
        assert cva.nle.pca_constants(p)[2] == 2 * p * (p - 2) * 0.5
    assert cva.nle.pca_constants(7)[1] == 45


def test_refusals_without_a_device():
    import cdlnet_video_amd as cva
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.nle.nle_pca(torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError):
        cva.nle.noise_level(torch.zeros(1, 1, 16, 16), method="bogus")
