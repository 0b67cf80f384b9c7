"""Argument checks of the C entry points cdl_ssim_fwd / cdl_ssim_bwd that return before any device work."""
import ctypes

import cdlnet_video_amd as cva

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments


def _win(values):
    return (ctypes.c_float * len(values))(*values)


def test_window_must_sum_to_one():
    lib = cva._lib.lib()
    n = int(lib.cdl_ssim_scratch_floats(2, 32, 32, 5))
    assert n > 0
    for w in ([0.25] * 5, [1.0] * 5, [0.2, 0.2, 0.2, 0.2, 0.19]):       # sums 1.25, 5, 0.99
        rc_f = lib.cdl_ssim_fwd(_FAKE, _FAKE, 2, 32, 32, _win(w), 5, 0.01, 0.03, 1.0, _FAKE, _FAKE, None, _FAKE, n,
                                None)
        rc_b = lib.cdl_ssim_bwd(_FAKE, _FAKE, 2, 32, 32, _win(w), 5, 0.01, 0.03, 1.0, _FAKE, _FAKE, _FAKE, None,
                                None, _FAKE, n, None)
        assert rc_f == cva._lib.CDL_EINVAL and rc_b == cva._lib.CDL_EINVAL, (w, rc_f, rc_b)


def test_shape_and_taps_refused():
    lib = cva._lib.lib()
    assert lib.cdl_ssim_scratch_floats(1, 6, 6, 7) == 0          # image smaller than the window
    assert lib.cdl_ssim_scratch_floats(1, 32, 32, 4) == 0         # even
    assert lib.cdl_ssim_scratch_floats(1, 32, 32, 17) == 0        # more than 15 taps
    w = _win([1.0 / 7] * 7)
    assert lib.cdl_ssim_fwd(_FAKE, _FAKE, 1, 6, 6, w, 7, 0.01, 0.03, 1.0, _FAKE, _FAKE, None, _FAKE, 1 << 20,
                            None) == cva._lib.CDL_EINVAL
    assert lib.cdl_ssim_bwd(_FAKE, _FAKE, 1, 32, 32, w, 7, 0.01, 0.03, 1.0, _FAKE, _FAKE, None, None, None, _FAKE,
                            1 << 20, None) == cva._lib.CDL_EINVAL    # nothing to write
