"""Local MAD noise-level estimates without a GPU: the restatement tests/nle_map_restate.py
against the oracle's global estimate, the cell layout, the interpolation, the accuracy of the estimator itself, and
the host-side refusals of the C entry point."""
import ctypes
import math

import pytest
import torch

import cdlnet_video_amd as cva
import nle_map_restate as R
from oracle import cdl_oracle as O
from sigmamap_util import smooth_map

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments


@pytest.mark.parametrize("shape,w", [((3, 1, 64, 64), 32), ((2, 3, 37, 53), 22), ((1, 1, 10, 10), 2),
                                     ((2, 1, 41, 90), 64), ((2, 3, 75, 33), 33)])
def test_whole_band_window_is_the_global_estimate(shape, w):
    """A window at least as large as the band is one cell, and its value has the bits of O.nle_mad."""
    g = torch.Generator().manual_seed(sum(shape))
    y = torch.rand(shape, generator=g) + torch.randn(shape, generator=g) * 0.1
    Hb, Wb = (shape[2] - 10) // 2 + 1, (shape[3] - 10) // 2 + 1
    assert w >= max(Hb, Wb)
    c = R.cells(y, w)
    assert c.shape == (shape[0], 1, 1, 1)
    assert torch.equal(c, O.nle_mad(y))
    assert torch.equal(R.image_map(y, w), O.nle_mad(y).expand(shape[0], 1, shape[2], shape[3]))


def test_one_side_shorter_than_the_window():
    """L <= w along one axis only: one cell there, several along the other."""
    y = torch.rand((2, 1, 40, 200), generator=torch.Generator().manual_seed(3))
    c = R.cells(y, 32, 16)                                      # band 16 x 96
    assert c.shape == (2, 1, 1, 5)
    b = R.band(y)
    assert torch.equal(c[:, 0, 0, 1], torch.median(b[:, :, :, 16:48].reshape(2, -1), dim=1)[0] / 0.6745)


@pytest.mark.parametrize("L,w,q", [(124, 32, 16), (123, 32, 16), (33, 32, 16), (32, 32, 16), (5, 32, 16), (100, 16, 5),
                                   (60, 32, 7), (1, 2, 1), (47, 16, 8)])
def test_cell_layout(L, w, q):
    r = R.cell_ranges(L, w, q)
    assert len(r) == (1 if L <= w else math.ceil((L - w) / q) + 1)
    assert r[0][0] == 0 and r[-1][1] == L                       # first at the origin, last flush with the border
    assert all(i1 - i0 == min(w, L) for i0, i1 in r)
    assert all(a[0] < b[0] for a, b in zip(r, r[1:]))           # no cell repeated
    assert all(i0 == min(i * q, L - w) for i, (i0, _) in enumerate(r)) or L <= w
    assert R.centres(L, w, q) == [i0 + i1 - 1 + 4.5 for i0, i1 in r]
    # the centre is the middle of the pixels the cell sees: 2 i0 .. 2 (i1 - 1) + 9
    assert all(c == 0.5 * (2 * i0 + 2 * (i1 - 1) + 9) for c, (i0, i1) in zip(R.centres(L, w, q), r))
    assert cva.nle.cell_starts(L, w, q) == [i0 for i0, _ in r]  # the package lays its cells out the same way


def test_interpolation_between_centres():
    H, W, w, q = 101, 140, 16, 8                                 # bands 46 x 66: 5 x 8 cells, the last ones flush
    ry, rx = R.cell_ranges(46, w, q), R.cell_ranges(66, w, q)
    c = torch.rand((2, 1, len(ry), len(rx)), generator=torch.Generator().manual_seed(0)) + 0.5
    m = R.interpolate(c, H, W, w, q)
    assert m.shape == (2, 1, H, W)
    cy, cx = R.centres(46, w, q), R.centres(66, w, q)
    # centres are half-integers and at least 2 pixels apart: the two pixels after a centre lie on one linear piece (or
    # on the constant beyond the last centre), so extrapolating them back by half a pixel gives the map at the centre
    for iy, py in enumerate(cy):
        a = int(py + 0.5)
        row = 1.5 * m[:, 0, a] - 0.5 * m[:, 0, a + 1]
        for ix, px in enumerate(cx):
            b = int(px + 0.5)
            at_centre = 1.5 * row[:, b] - 0.5 * row[:, b + 1]
            assert torch.allclose(at_centre, c[:, 0, iy, ix], rtol=1e-5, atol=0)
    a0, a1, b0, b1 = int(cy[0] - 0.5), int(cy[-1] + 0.5), int(cx[0] - 0.5), int(cx[-1] + 0.5)
    assert torch.equal(m[:, :, :a0 + 1], m[:, :, a0:a0 + 1].expand(-1, -1, a0 + 1, -1))       # constant outside
    assert torch.equal(m[:, :, a1:], m[:, :, a1:a1 + 1].expand(-1, -1, H - a1, -1))
    assert torch.equal(m[:, :, :, :b0 + 1], m[:, :, :, b0:b0 + 1].expand(-1, -1, -1, b0 + 1))
    assert torch.equal(m[:, :, :, b1:], m[:, :, :, b1:b1 + 1].expand(-1, -1, -1, W - b1))
    for iy in range(len(cy) - 1):                                # between neighbouring cells elsewhere
        for ix in range(len(cx) - 1):
            blk = m[:, 0, int(cy[iy] + 0.5):int(cy[iy + 1] + 0.5), int(cx[ix] + 0.5):int(cx[ix + 1] + 0.5)]
            corners = c[:, 0, iy:iy + 2, ix:ix + 2].reshape(2, -1)
            assert torch.all(blk >= corners.min(dim=1)[0][:, None, None] * (1 - 1e-6))
            assert torch.all(blk <= corners.max(dim=1)[0][:, None, None] * (1 + 1e-6))
    one = R.interpolate(c[:, :, :1, :1], 20, 25, 32)            # one cell along an axis: constant along it
    assert torch.equal(one, c[:, :, :1, :1].expand(-1, -1, 20, 25))


def test_clip_frames_are_never_mixed():
    clip = torch.rand((2, 3, 4, 30, 44), generator=torch.Generator().manual_seed(1))
    c = R.cells(clip, 8, 4)
    assert c.shape == (2, 1, 4, 2, 4)
    for d in range(4):
        assert torch.equal(c[:, :, d], R.cells(clip[:, :, d], 8, 4))
        assert torch.equal(R.frames(clip)[:, :, d], O.nle_mad(clip[:, :, d]))
    assert R.frames(clip).shape == (2, 1, 4, 1, 1)
    assert R.code_map(clip, 8, 4, s=2).shape == (2, 1, 2, 15, 22)


# Measured with this restatement and these seeds (window 32, step 16, 7 x 7 cells, 4 x 1 x 256 x 256, map in [10, 40]):
# bias -2.71 %, 4.57 % rms, worst cell 12.51 %; the single global estimate 13.34 % rms (2.92 x).  Each gate is 1.5 x
# the measured figure: the sampling error of a 1024-sample median alone is 3.7 % for independent samples, and the
# overlapping stride-2 taps make it larger.
BIAS, RMS, WORST = 0.0271, 0.0457, 0.1251


@pytest.mark.parametrize("content", ["flat", "clip"])
def test_accuracy_of_the_local_estimate(content):
    shape = (4, 1, 256, 256)
    true_map = smooth_map(shape, 7)
    x = torch.full(shape, 0.5) if content == "flat" else cva.utils.synthetic_clip(shape, seed=3)
    y = x + torch.randn(shape, generator=torch.Generator().manual_seed(11)) * true_map / 255
    truth = R.cell_truth(true_map, 32, 16)
    assert truth.shape == (4, 1, 7, 7)
    local = 255 * R.cells(y, 32, 16) / truth - 1
    glob = 255 * O.nle_mad(y) / truth - 1
    bias, rms, worst = float(local.mean()), float(local.pow(2).mean().sqrt()), float(local.abs().max())
    grms = float(glob.pow(2).mean().sqrt())
    print(f"local MAD [{content}]: bias {bias:+.4f} rms {rms:.4f} worst {worst:.4f}; global rms {grms:.4f} "
          f"({grms / rms:.2f} x), worst {float(glob.abs().max()):.4f}")
    assert abs(bias) < 1.5 * BIAS and rms < 1.5 * RMS and worst < 1.5 * WORST
    assert grms >= 2 * rms


def test_abi_symbols_and_refusals():
    lib = cva._lib.lib()
    assert "cdl_nle_mad_cells" in cva._lib.SIGNATURES and "cdl_nle_mad_cells_scratch_floats" in cva._lib.SIZE_T_FUNCS
    n = int(lib.cdl_nle_mad_cells_scratch_floats(2, 3, 64, 40))
    assert n == 2 * 3 * 28 * 16 == int(lib.cdl_nle_mad_scratch_floats(2, 3, 64, 40))
    assert lib.cdl_nle_mad_cells_scratch_floats(1, 1, 9, 64) == 0          # smaller than the filter
    bad = cva._lib.CDL_EINVAL
    call = lambda y, c, sc, H, W, w, q: lib.cdl_nle_mad_cells(y, c, sc, 1 << 20, 2, 3, H, W, w, q, None)
    assert call(None, _FAKE, _FAKE, 64, 40, 32, 16) == bad
    assert call(_FAKE, None, _FAKE, 64, 40, 32, 16) == bad
    assert call(_FAKE, _FAKE, None, 64, 40, 32, 16) == bad
    assert call(_FAKE, _FAKE, _FAKE, 64, 40, 1, 1) == bad                  # window < 2
    assert call(_FAKE, _FAKE, _FAKE, 64, 40, 32, 0) == bad                 # step < 1
    assert call(_FAKE, _FAKE, _FAKE, 9, 40, 32, 16) == bad                 # image smaller than the filter
    assert call(_FAKE, _FAKE, _FAKE, 64, 9, 32, 16) == bad
    assert lib.cdl_nle_mad_cells(_FAKE, _FAKE, _FAKE, n - 1, 2, 3, 64, 40, 32, 16, None) == bad   # scratch too small


def test_python_surface_exists():
    for name in ("nle_mad_cells", "nle_mad_map", "nle_mad_frames"):
        assert callable(getattr(cva.nle, name))
