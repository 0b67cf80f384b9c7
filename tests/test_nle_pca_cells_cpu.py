"""Windowed weak-texture PCA estimate (nle_pca_cells / nle_pca_map / nle_pca_frames), the parts
that need no GPU: cell geometry and the interpolation plan against the float64 restatement
(nle_pca_cells_restate.py), the refusals of the host functions and of the two C entry points, the dispatcher, the
bindings, and the precondition of the device parity tests."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nle_pca_cells_restate as C
from conftest import ROOT

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments


@pytest.mark.parametrize("L,w,q", [(75, 40, 20), (83, 40, 20), (83, 48, 24), (64, 64, 32), (65, 64, 32), (40, 64, 32),
                                   (1080, 64, 32), (1920, 64, 32), (23, 8, 4), (100, 30, 7), (9, 7, 1)])
def test_cell_geometry(L, w, q):
    import cdlnet_video_amd as cva
    starts = cva.nle.cell_starts(L, w, q)
    ranges = C.cell_ranges(L, w, q)
    assert starts == [r0 for r0, _ in ranges]
    assert ranges[0][0] == 0 and ranges[-1][1] == L                  # flush with both borders
    assert all(r1 - r0 == min(w, L) for r0, r1 in ranges)
    assert all(b[0] - a[0] <= q for a, b in zip(ranges, ranges[1:]))  # no pixel between two cells is skipped
    assert len(set(starts)) == len(starts)
    assert (len(cva.nle.cell_starts(1080, 64, 32)), len(cva.nle.cell_starts(1920, 64, 32))) == (33, 59)


@pytest.mark.parametrize("H,W,w,q", [(75, 83, 40, 20), (75, 83, 48, 24), (40, 45, 64, 32), (33, 90, 16, 5), (20, 23, 8, 4)])
def test_interpolation_plan_matches_restatement(H, W, w, q):
    import cdlnet_video_amd as cva
    ny, nx = len(C.cell_ranges(H, w, q)), len(C.cell_ranges(W, w, q))
    cells = torch.rand(2, ny, nx, dtype=torch.float64, generator=torch.Generator().manual_seed(H + W))
    got = cva.nle._pca_interpolate(cells, H, W, w, q)
    ref = C.interpolate(cells.numpy(), H, W, w, q)
    assert got.shape == (2, H, W) and got.dtype == torch.float64
    assert float(np.abs(got.numpy() - ref).max()) < 1e-12
    cy, cx = C.centres(H, w, q), C.centres(W, w, q)                   # at a centre the map is the cell's value
    for iy, yy in enumerate(cy):
        for ix, xx in enumerate(cx):
            if yy == int(yy) and xx == int(xx):
                assert abs(float(got[0, int(yy), int(xx)] - cells[0, iy, ix])) < 1e-12
    assert torch.equal(got[:, 0, 0], cells[:, 0, 0]) and torch.equal(got[:, -1, -1], cells[:, -1, -1])   # constant beyond


def test_host_refusals_without_a_device():
    import cdlnet_video_amd as cva
    y = torch.zeros(1, 1, 32, 32)
    for fn in (cva.nle.nle_pca_cells, cva.nle.nle_pca_map):
        with pytest.raises(ValueError, match="window"):
            fn(y, window=6)                                           # below the default patch size 7
        with pytest.raises(ValueError, match="window"):
            fn(y, window=8, patchsize=9)
        with pytest.raises(ValueError, match="window"):
            fn(y, window=16.5)
        with pytest.raises(ValueError, match="step"):
            fn(y, window=16, step=0)
        with pytest.raises(ValueError, match="step"):
            fn(y, window=16, step=2.5)
        with pytest.raises(ValueError, match="expects"):
            fn(y[0])
        with pytest.raises(ValueError, match="expects"):
            fn(y[None, None])
        with pytest.raises(ValueError, match="outside 3..11"):
            fn(y, window=16, patchsize=13)
        with pytest.raises(ValueError, match="smaller than"):
            fn(y[:, :, :5])
        with pytest.raises(RuntimeError, match="ROCm device"):
            fn(y)
        with pytest.raises(RuntimeError, match="ROCm device"):
            fn(y, window=None)
    with pytest.raises(ValueError, match=r"\(N, C, D, H, W\)"):
        cva.nle.nle_pca_frames(y)
    with pytest.raises(RuntimeError, match="ROCm device"):
        cva.nle.nle_pca_frames(y[:, :, None])
    with pytest.raises(NotImplementedError, match=r"nle_pca\(y\)\[0\]"):           # noise_level stays MAD-only
        cva.nle.noise_level(y, "PCA")


def test_noise_level_map_dispatch(monkeypatch):
    import cdlnet_video_amd as cva
    seen = []
    monkeypatch.setattr(cva.nle, "nle_mad_map", lambda y, **kw: seen.append(("MAD", kw)) or "mad")
    monkeypatch.setattr(cva.nle, "nle_pca_map", lambda y, **kw: seen.append(("PCA", kw)) or "pca")
    y = torch.zeros(1, 1, 32, 32)
    assert cva.nle.noise_level_map(y) == "mad"
    assert cva.nle.noise_level_map(y, "MAD", window=16, s=2) == "mad"
    assert cva.nle.noise_level_map(y, method="PCA", window=48, patchsize=5) == "pca"
    assert seen == [("MAD", {}), ("MAD", {"window": 16, "s": 2}), ("PCA", {"window": 48, "patchsize": 5})]
    with pytest.raises(NotImplementedError, match="'MAD' or 'PCA'"):
        cva.nle.noise_level_map(y, "wvlt")


def test_c_entry_points_refuse_before_any_launch():
    import cdlnet_video_amd as cva
    lib, EINVAL = cva._lib.lib(), cva._lib.CDL_EINVAL
    size = lib.cdl_nle_pca_gram_cells_scratch_floats
    n = int(size(2, 1, 75, 83, 7, 40, 20))
    assert n > 0
    assert size(2, 1, 75, 83, 2, 40, 20) == 0 and size(2, 1, 75, 83, 12, 40, 20) == 0     # p outside 3..11
    assert size(2, 1, 75, 83, 7, 6, 3) == 0                                              # window < p
    assert size(2, 1, 75, 83, 7, 40, 0) == 0                                             # step < 1
    assert size(2, 1, 6, 83, 7, 40, 20) == 0 and size(0, 1, 75, 83, 7, 40, 20) == 0
    with cva.ops.trace() as t:
        call = lambda y=_FAKE, N=2, p=7, w=40, q=20, tau=_FAKE, g=_FAKE, c=_FAKE, s=_FAKE, ns=n, ch=0: \
            lib.cdl_nle_pca_gram_cells(y, N, 1, 75, 83, ch, p, w, q, tau, g, c, s, ns, None)
        for kw in (dict(y=None), dict(tau=None), dict(g=None), dict(c=None), dict(s=None), dict(p=2), dict(p=12),
                   dict(w=6), dict(q=0), dict(q=-3), dict(N=0), dict(ch=1), dict(ns=n - 1)):
            assert call(**kw) == EINVAL, kw
        n1 = int(lib.cdl_nle_pca_scratch_floats(2, 1, 75, 83, 7))
        assert n1 > 0
        for args in ((None, 2, 1, 75, 83, 0, 7, 1.0, _FAKE, _FAKE, _FAKE, n1),
                     (_FAKE, 2, 1, 75, 83, 0, 12, 1.0, _FAKE, _FAKE, _FAKE, n1),
                     (_FAKE, 2, 1, 75, 83, 0, 7, 1.0, _FAKE, _FAKE, _FAKE, n1 - 1)):
            assert lib.cdl_nle_pca_gram(*args, None) == EINVAL
    assert len(t) == 0                                                 # refused before any launch
    # a window that covers the image is one cell per sample: the whole-image plan of one sample, once per sample
    one = int(lib.cdl_nle_pca_scratch_floats(1, 1, 40, 45, 7))
    assert int(size(2, 1, 40, 45, 7, 64, 32)) - 64 == 2 * (one - 64)         # 64 floats of alignment slack in each


def test_header_declares_and_lib_binds_the_entry_points():
    import cdlnet_video_amd as cva
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    assert re.search(r"\bint cdl_nle_pca_gram_cells\(", header)
    assert re.search(r"\bsize_t cdl_nle_pca_gram_cells_scratch_floats\(", header)
    assert "cdl_nle_pca_gram_cells" in cva._lib.SIGNATURES
    assert "cdl_nle_pca_gram_cells_scratch_floats" in cva._lib.SIZE_T_FUNCS
    lib = ctypes.CDLL(cva._lib.LIB_PATH)
    assert hasattr(lib, "cdl_nle_pca_gram_cells") and hasattr(lib, "cdl_nle_pca_gram_cells_scratch_floats")
    for name in ("nle_pca_cells", "nle_pca_map", "nle_pca_frames", "noise_level_map", "pca_gram_cells"):
        assert callable(getattr(cva.nle, name))


@pytest.mark.parametrize("case", sorted(C.PARITY_CASES))
def test_parity_cases_keep_their_distance(case):
    """What lets the device tests demand equal counts: no refinement threshold of any cell lies within 5e-5
    (relative) of a texture strength of that cell, an order above the fp32 rounding of Xtr (~70 squares, worst
    case ~4e-6)."""
    import cdlnet_video_amd as cva
    (H, W), N, w, q, p, itr, seed = C.PARITY_CASES[case]
    y = C.noisy(N, H, W, seed)
    dist = C.closest_distance(y, w, q, p, cva.nle.pca_constants(p)[0], itr)
    assert dist >= C.MIN_DISTANCE, dist


def test_restated_cells_follow_the_ramp():
    """On the test input every cell's estimate stays at or below the true level of the cell's loud (right) edge --
    weak-texture selection favours the quiet side -- and grows along the ramp; p = 11 at window 48 stops every cell
    (fewer than 121 patches kept)."""
    import cdlnet_video_amd as cva
    y = C.noisy(1, 75, 83, 0)
    nlevel, th, num = C.cells(y, 40, 20, 7, cva.nle.pca_constants(7)[0], 3)
    assert nlevel.shape == (1, 1, 3, 4) and (num >= 49).all()
    true = 255 * C.ramp(83).numpy()
    for ix, (x0, x1) in enumerate(C.cell_ranges(83, 40, 20)):
        col = 255 * nlevel[0, 0, :, ix]
        assert (col <= true[x1 - 1]).all() and (col >= 0.5 * true[x0]).all(), (ix, col)
    assert (np.diff(nlevel[0, 0].mean(axis=0)) > 0).all()
    (H, W), N, w, q, p, itr, seed = C.PARITY_CASES["p11"]
    _, _, num = C.cells(C.noisy(N, H, W, seed), w, q, p, cva.nle.pca_constants(p)[0], itr)
    assert num.shape == (1, 1, 3, 3) and (num < 121).all()
