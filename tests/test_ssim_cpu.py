"""The SSIM restatement on its own terms (identities, closed forms, a hand evaluation, gradcheck), and the argument
checks of cva.metrics, which raise before any device work."""
import numpy as np
import pytest
import torch

import ssim_restate as R


def _pair(shape, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=dtype)
    y = (x + 0.2 * torch.randn(shape, generator=g, dtype=dtype)).clamp(0, 1)
    return x, y


def test_identity_and_symmetry():
    x, y = _pair((2, 3, 24, 20), 0)
    assert torch.allclose(R.ssim_per_channel(x, x, data_range=1.0), torch.ones(2, 3, dtype=torch.float64),
                          atol=1e-12, rtol=0)
    assert torch.allclose(R.structural_similarity(x, x), torch.ones(2, 3, dtype=torch.float64), atol=1e-12, rtol=0)
    assert torch.allclose(R.ssim_per_channel(x, y, 1.0), R.ssim_per_channel(y, x, 1.0), atol=1e-14, rtol=0)
    assert torch.allclose(R.structural_similarity(x, y), R.structural_similarity(y, x), atol=1e-14, rtol=0)
    assert (R.ssim_per_channel(x, y, 1.0) < 1).all()


def test_constant_images_closed_form():
    # constant a and b: every variance vanishes, cs = 1, S = (2ab + C1) / (a^2 + b^2 + C1)
    a, b, rng = 0.3, 0.7, 1.0
    x = torch.full((1, 1, 16, 16), a, dtype=torch.float64)
    y = torch.full((1, 1, 16, 16), b, dtype=torch.float64)
    C1 = (0.01 * rng) ** 2
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    # 1e-12: the variances are E[x^2] - E[x]^2 of equal fp64 numbers, ~1e-17, divided by C2 ~ 1e-3
    assert abs(float(R.ssim(x, y, data_range=rng)) - want) < 1e-12
    assert abs(float(R.structural_similarity(x, y, data_range=rng)) - want) < 1e-12


def test_seven_by_seven_by_hand():
    # one valid position of the 7 x 7 uniform window: plain sample statistics of the 49 pixels
    rs = np.random.RandomState(3)
    x = rs.rand(7, 7)
    y = np.clip(x + 0.1 * rs.randn(7, 7), 0, 1)
    n = 49.0
    mx, my = x.sum() / n, y.sum() / n
    vx = ((x * x).sum() / n - mx * mx) * n / (n - 1)
    vy = ((y * y).sum() / n - my * my) * n / (n - 1)
    vxy = ((x * y).sum() / n - mx * my) * n / (n - 1)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    want = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    got = float(R.structural_similarity(torch.from_numpy(x), torch.from_numpy(y)))
    assert abs(got - want) < 1e-13
    # the Gaussian window of pytorch_msssim at win_size 7, one position
    w = R.gaussian_window(7, 1.5).numpy()
    W2 = np.outer(w, w)
    ex, ey = (W2 * x).sum(), (W2 * y).sum()
    sx, sy, sxy = (W2 * x * x).sum() - ex * ex, (W2 * y * y).sum() - ey * ey, (W2 * x * y).sum() - ex * ey
    want_g = (2 * ex * ey + C1) * (2 * sxy + C2) / ((ex * ex + ey * ey + C1) * (sx + sy + C2))
    got_g = float(R.ssim(torch.from_numpy(x)[None, None], torch.from_numpy(y)[None, None], data_range=1.0,
                         win_size=7))
    assert abs(got_g - want_g) < 1e-13


@pytest.mark.parametrize("win", [3, 7, 11])
def test_reflect_then_crop_equals_valid(win):
    x, y = _pair((2, 2, 19, 26), win)
    full, S = R.structural_similarity(x, y, win_size=win, full=True)
    assert S.shape[-2:] == x.shape[-2:]
    valid = R.structural_similarity_valid(x, y, win_size=win)
    assert torch.allclose(full, valid, atol=1e-14, rtol=0)


def test_scipy_reflect_padding():
    idx = R._reflect_index(4, 3).tolist()
    assert idx == [2, 1, 0, 0, 1, 2, 3, 3, 2, 1]


def test_gradcheck_restatement():
    x, y = _pair((1, 2, 13, 14), 5)
    x.requires_grad_()
    y.requires_grad_()
    rng = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b, r: R.ssim(a, b, data_range=r, win_size=5), (x, y, rng))
    clip_o = torch.rand((1, 1, 3, 12, 12), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    clip_t = torch.rand((1, 1, 3, 12, 12), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    assert torch.autograd.gradcheck(R.ssim_frames, (clip_o.requires_grad_(), clip_t.requires_grad_()))


def test_frames_repeat_is_neutral():
    o, t = _pair((2, 1, 3, 16, 16), 8)
    direct = sum(1 - R.ssim(o[:, :, k], t[:, :, k], data_range=o[:, :, k].max() - o[:, :, k].min())
                 for k in range(3)) / 3
    assert abs(float(direct - R.ssim_frames(o, t))) < 1e-14


def test_argument_checks_before_device():
    import cdlnet_video_amd as cva
    m = cva.metrics
    x4 = torch.rand(1, 1, 16, 16)
    with pytest.raises(ValueError):
        m.ssim(x4, x4, win_size=10)
    with pytest.raises(ValueError):
        m.ssim(x4, x4, win_size=17)                        # larger than the image
    with pytest.raises(ValueError):
        m.ssim(x4, torch.rand(1, 1, 16, 15))
    with pytest.raises(NotImplementedError, match="ssim_frames"):
        m.ssim(torch.rand(1, 1, 2, 16, 16), torch.rand(1, 1, 2, 16, 16))
    with pytest.raises(ValueError):
        m.structural_similarity(x4, x4, win_size=8)
    with pytest.raises(ValueError):
        m.structural_similarity(torch.rand(6, 6), torch.rand(6, 6))
    with pytest.raises(ValueError):
        m.structural_similarity(x4, torch.rand(1, 1, 16, 17))
    with pytest.raises(ValueError):
        m.ssim_frames(torch.rand(1, 1, 2, 16, 16), torch.rand(1, 1, 2, 16, 17))
    with pytest.raises(ValueError):
        m.ssim_frames(x4, x4)
    with pytest.raises(ValueError):
        m.video_ssim(x4, x4)
    assert cva.ssim is m.ssim


def test_cpu_tensors_refused():
    import cdlnet_video_amd as cva
    x4 = torch.rand(1, 1, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.metrics.ssim(x4, x4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.metrics.structural_similarity(x4, x4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.metrics.ssim_frames(torch.rand(1, 1, 2, 16, 16), torch.rand(1, 1, 2, 16, 16))
