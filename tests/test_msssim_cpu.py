"""MS-SSIM without a GPU: the pooling convention and the restatement (tests/msssim_restate.py), the refusals of
cva.ms_ssim / ms_ssim_frames that come before any device work, and the argument checks of the C entry points."""
import ctypes

import pytest
import torch

import cdlnet_video_amd as cva
import msssim_restate as M
import ssim_restate as R

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments


def _win(values):
    return (ctypes.c_float * len(values))(*values)


def test_public_surface():
    assert cva.ms_ssim is cva.metrics.ms_ssim and "ms_ssim" in cva.__all__
    assert callable(cva.metrics.ms_ssim_frames)
    assert list(cva.metrics.MS_WEIGHTS) == M.WEIGHTS


def test_pooling_convention():
    p = M.pool(torch.ones(1, 1, 5, 6))
    assert p.shape == (1, 1, 3, 3)
    assert torch.equal(p[0, 0, 0], torch.full((3,), 0.5)) and torch.equal(p[0, 0, 1:], torch.ones(2, 3))
    x = torch.arange(24.0).reshape(1, 1, 4, 6)
    q = M.pool(x)                                                    # even axes: pairs (2i, 2i + 1)
    assert q.shape == (1, 1, 2, 3)
    assert torch.equal(q[0, 0], (x[0, 0, 0::2, 0::2] + x[0, 0, 0::2, 1::2] + x[0, 0, 1::2, 0::2] + x[0, 0, 1::2, 1::2]) / 4)
    y = torch.arange(7.0).reshape(1, 1, 1, 7).expand(1, 1, 2, 7).contiguous()      # odd axis: (0 + x0) / 2, (x1 + x2) / 2, ..
    assert torch.equal(M.pool(y)[0, 0, 0], torch.tensor([0.0, 1.5, 3.5, 5.5]))


def test_level_sizes():
    want = [(177, 162), (89, 81), (45, 41), (23, 21), (12, 11)]
    assert M.level_sizes(177, 162, 5) == want
    assert cva.metrics._level_sizes(177, 162, 5) == want
    x = torch.zeros(1, 1, 177, 162)
    for hw in want:
        assert tuple(x.shape[-2:]) == hw
        x = M.pool(x)
    lib = cva._lib.lib()
    assert lib.cdl_msssim_pyramid_floats(3, 177, 162, 5) == 3 * sum(h * w for h, w in want[1:])
    assert lib.cdl_msssim_pyramid_floats(3, 177, 162, 1) == 0


def test_one_level_is_relu_of_ssim():
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 2, 20, 24, generator=g, dtype=torch.float64)
    y = x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)
    for b in (y, -y, 1 - y):
        got = M.ms_ssim(x, b, data_range=1.0, win_size=5, weights=[1.0], size_average=False)
        assert torch.equal(got, R.ssim(x, b, data_range=1.0, win_size=5, size_average=False, nonnegative_ssim=True))
    # x against -y has a POSITIVE SSIM (luminance and cs terms both change sign); 1 - y keeps the means positive and
    # turns the covariance: a negative mean, clipped to 0
    assert float(R.ssim(x, -y, data_range=1.0, win_size=5)) > 0.5 > 0 > float(R.ssim(x, 1 - y, data_range=1.0, win_size=5))
    assert float(M.ms_ssim(x, 1 - y, data_range=1.0, win_size=5, weights=[1.0])) == 0.0


def test_python_refusals_come_before_any_device_work():
    m = cva.metrics
    x = torch.zeros(1, 1, 176, 176)
    with pytest.raises(TypeError, match="expected tensors"):
        m.ms_ssim(x, [1.0])
    with pytest.raises(TypeError, match="expected tensors"):
        m.ms_ssim_frames(x.numpy(), x)
    with pytest.raises(ValueError, match="same dimensions"):
        m.ms_ssim(x, torch.zeros(1, 1, 176, 175))
    with pytest.raises(ValueError, match="same dimensions"):
        m.ms_ssim_frames(torch.zeros(1, 1, 2, 176, 176), torch.zeros(1, 1, 3, 176, 176))
    with pytest.raises(NotImplementedError, match="ms_ssim_frames"):
        m.ms_ssim(torch.zeros(1, 1, 2, 176, 176), torch.zeros(1, 1, 2, 176, 176))
    with pytest.raises(ValueError, match="4-D"):
        m.ms_ssim(x[0], x[0])
    with pytest.raises(ValueError, match=r"\(N, C, D, H, W\)"):
        m.ms_ssim_frames(x, x)
    for win in (4, 1, 17):                                          # the window checks of ssim
        with pytest.raises(ValueError, match="win_size"):
            m.ms_ssim(x, x, win_size=win)
    with pytest.raises(ValueError, match="exceeds the image extent"):
        m.ms_ssim(torch.zeros(1, 1, 8, 200), torch.zeros(1, 1, 8, 200))
    # pytorch_msssim's assertion smaller_side > (win_size - 1) * 2**4 = 160
    for shape, ok in (((1, 1, 200, 160), False), ((1, 1, 161, 200), True)):
        z = torch.zeros(shape)
        if ok:
            with pytest.raises(RuntimeError, match="is on cpu"):    # passes the shape checks, refused as a host tensor
                m.ms_ssim(z, z)
        else:
            with pytest.raises(ValueError, match=r"\(win_size - 1\) \* 2\*\*4 = 160"):
                m.ms_ssim(z, z)
    with pytest.raises(ValueError, match="smaller than win_size"):   # ... generalised: three levels, win 3 need > 8
        m.ms_ssim(torch.zeros(1, 1, 8, 30), torch.zeros(1, 1, 8, 30), win_size=3, weights=[0.3, 0.3, 0.4])
    with pytest.raises(RuntimeError, match="is on cpu"):
        m.ms_ssim(torch.zeros(1, 1, 9, 30), torch.zeros(1, 1, 9, 30), win_size=3, weights=[0.3, 0.3, 0.4])
    with pytest.raises(ValueError, match="smaller than win_size"):
        m.ms_ssim_frames(torch.zeros(1, 1, 2, 160, 200), torch.zeros(1, 1, 2, 160, 200))
    with pytest.raises(ValueError, match="1 to 8 levels"):
        m.ms_ssim(x, x, weights=[])
    with pytest.raises(ValueError, match="1 to 8 levels"):
        m.ms_ssim(x, x, weights=[0.1] * 9)


def test_scratch_sizes():
    lib = cva._lib.lib()
    assert lib.cdl_msssim_scratch_floats(2, 177, 162, 11, 5) > 0
    assert lib.cdl_msssim_scratch_floats(2, 160, 200, 11, 5) == 0      # the coarsest level is 10 x 13
    assert lib.cdl_msssim_scratch_floats(2, 160, 200, 11, 4) > 0
    assert lib.cdl_msssim_scratch_floats(2, 177, 162, 11, 0) == 0
    assert lib.cdl_msssim_scratch_floats(2, 4096, 4096, 3, 9) == 0
    assert lib.cdl_msssim_scratch_floats(2, 177, 162, 4, 1) == 0       # even window
    assert lib.cdl_msssim_scratch_floats(0, 177, 162, 11, 5) == 0
    # one level: room for cdl_ssim's partials (the reverse keeps two sums per workgroup)
    assert lib.cdl_msssim_scratch_floats(2, 64, 64, 5, 1) >= lib.cdl_ssim_scratch_floats(2, 64, 64, 5)
    assert lib.cdl_msssim_pyramid_floats(2, 64, 64, 0) == 0 and lib.cdl_msssim_pyramid_floats(2, 64, 64, 9) == 0


def _fwd(lib, *, x=_FAKE, y=_FAKE, P=2, H=64, W=64, w=None, taps=5, rng=_FAKE, levels=3, px=_FAKE, py=_FAKE, vals=_FAKE,
         scratch=_FAKE, n=None):
    w = _win([0.2] * 5) if w is None else w
    n = int(lib.cdl_msssim_scratch_floats(2, 64, 64, 5, 3)) if n is None else n
    return lib.cdl_msssim_fwd(x, y, P, H, W, w, taps, 0.01, 0.03, rng, levels, px, py, vals, scratch, n, None)


def _bwd(lib, *, x=_FAKE, y=_FAKE, px=_FAKE, py=_FAKE, P=2, H=64, W=64, w=None, taps=5, rng=_FAKE, levels=3, g=_FAKE,
         dx=_FAKE, dy=None, dr=None, work=_FAKE, scratch=_FAKE, n=None):
    w = _win([0.2] * 5) if w is None else w
    n = int(lib.cdl_msssim_scratch_floats(2, 64, 64, 5, 3)) if n is None else n
    return lib.cdl_msssim_bwd(x, y, px, py, P, H, W, w, taps, 0.01, 0.03, rng, levels, g, dx, dy, dr, work, scratch, n,
                              None)


def test_entry_points_refuse_bad_host_arguments():
    lib = cva._lib.lib()
    E = cva._lib.CDL_EINVAL
    n = int(lib.cdl_msssim_scratch_floats(2, 64, 64, 5, 3))
    assert n > 0
    for kw in (dict(x=None), dict(y=None), dict(rng=None), dict(vals=None), dict(scratch=None), dict(px=None),
               dict(py=None), dict(n=n - 1), dict(levels=0), dict(levels=9), dict(levels=5),      # 64 -> 4 at level 4
               dict(taps=4), dict(H=4), dict(P=0),
               dict(w=_win([0.25] * 5)), dict(w=_win([0.2, 0.2, 0.2, 0.2, 0.19]))):
        assert _fwd(lib, **kw) == E, kw
    for kw in (dict(x=None), dict(y=None), dict(rng=None), dict(g=None), dict(scratch=None), dict(px=None),
               dict(py=None), dict(work=None), dict(dx=None), dict(n=n - 1), dict(levels=0), dict(levels=9),
               dict(levels=5), dict(taps=4), dict(W=4), dict(w=_win([1.0] * 5))):
        assert _bwd(lib, **kw) == E, kw
