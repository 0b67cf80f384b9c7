"""The blind noise-level function var(y | x) = a x + b without a GPU: the accuracy of the
estimator as tests/nlf_restate.py restates it (never the HIP code), cva.nle.nlf_fit_bins on CPU tensors against the
restatement's fit, the host-side refusals of the C entry point and the launch statements of cdl_nle.hip."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import cdlnet_video_amd as cva
import nlf_restate as R
from conftest import ROOT

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments

PAIRS = {"mixed": (0.01, (5 / 255) ** 2), "low": (0.003, (2 / 255) ** 2), "flat": (0.0, (25 / 255) ** 2),
         "poisson": (0.02, 0.0)}
# Measured with this restatement on these inputs (seeds 0..7, 32 bins on [0, 1), min_count 64, 2 reweightings): the
# largest rms and the largest worst point of the relative error of the fitted sigma(x) over the span of the usable bin
# centres, 50 points.  Each gate is 1.5 x the measured figure, the factor tests/test_nle_map_cpu.py uses for the same
# kind of sampling error (a bin of a 60 x 92 band holds about 200 samples: a median of that many is 6 % off, rms).
MEASURED = {  # (H, W): {pair: (rms, worst, fewest usable bins)}
    (128, 192): {"mixed": (0.0308, 0.0991, 24), "low": (0.0295, 0.0932, 24), "flat": (0.0390, 0.0746, 24),
                 "poisson": (0.0331, 0.1148, 24)},
    (96, 96): {"mixed": (0.0750, 0.1130, 15), "low": (0.0517, 0.0668, 15), "flat": (0.0554, 0.0815, 15),
               "poisson": (0.0671, 0.1058, 15)},
}


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("shape", list(MEASURED), ids=lambda s: f"{s[0]}x{s[1]}")
def test_accuracy_of_the_restated_estimator(shape, pair):
    H, W = shape
    a0, b0 = PAIRS[pair]
    rms_gate, worst_gate, fewest = MEASURED[shape][pair]
    rms_all, worst_all = 0.0, 0.0
    for seed in range(8):
        _, y = R.noisy(H, W, seed, a0, b0)
        a, b, _, count, centre = R.nlf(y[None])
        assert a >= 0 and b >= 0, (seed, a, b)
        assert int((count >= 64).sum()) >= fewest
        xs = np.linspace(*R.usable_span(count, centre), 50)
        rel = np.sqrt(a * xs + b) / np.sqrt(a0 * xs + b0) - 1
        rms_all = max(rms_all, float(np.sqrt(np.mean(rel ** 2))))
        worst_all = max(worst_all, float(np.abs(rel).max()))
        if a0 == 0:                                         # flat noise comes back flat: sigma(x) against the one level
            assert float(np.abs(np.sqrt(a * xs + b) / np.sqrt(b0) - 1).max()) < 1.5 * worst_gate
    print(f"nlf [{H}x{W} {pair}]: largest rms {rms_all:.4f}, largest worst point {worst_all:.4f}")
    assert rms_all < 1.5 * rms_gate and worst_all < 1.5 * worst_gate


def test_restated_bins_pool_channels_and_leave_outsiders_out():
    rng = np.random.default_rng(0)
    d, m = rng.random((3, 6, 7)), rng.random((3, 6, 7)) * 1.4 - 0.2        # some m below lo, some at or above hi
    m[0, 0, 0], m[0, 0, 1], m[0, 0, 2] = 1.0, 0.0, 0.5
    sigma, count, centre = R.bin_stats(d, m, bins=8)
    k = R.bin_index(m, 8, 0.0, 1.0)
    assert k[0, 0, 0] == -1 and k[0, 0, 1] == 0 and k[0, 0, 2] == 4          # hi is outside, lo and an edge inside
    assert count.sum() == int(((m >= 0) & (m < 1)).sum()) and count.sum() < m.size
    assert np.allclose(centre, (np.arange(8) + 0.5) / 8)
    for b in range(8):
        members = d[(m >= b / 8) & (m < (b + 1) / 8)]
        assert count[b] == members.size
        assert sigma[b] == np.sort(members)[(members.size - 1) // 2] / 0.6745
    assert np.array_equal(R.bin_index(m, 8, 0.0, 1.0, f32=True), k)        # no sample of these sits within an ulp of an edge
    empty = R.bin_stats(d, np.full_like(d, 2.0), bins=4)
    assert not empty[0].any() and not empty[1].any()


def test_restated_bands_are_the_oracles():
    from oracle import cdl_oracle as O
    y = torch.rand((1, 2, 23, 31), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    d, m = R.bands(y[0].numpy())
    hh = torch.cat([O.hh_filter().double()] * 2)
    ref = torch.nn.functional.conv2d(y, hh, stride=2, groups=2).abs()[0].numpy()
    assert d.shape == ref.shape == (2, 7, 11) and np.abs(d - ref).max() < 1e-14
    assert abs(m[1, 3, 5] - y[0, 1, 8:15, 12:19].mean().item()) < 1e-15


# ------------------------------------------------------------------------------------------------ the fit
def _line_bins(a, b, bins=32, count=500, noise=0.0, seed=0):
    centre = (np.arange(bins) + 0.5) / bins
    v = np.maximum(a * centre + b, 1e-7) * (1 + noise * np.random.default_rng(seed).standard_normal(bins))
    return np.sqrt(np.abs(v)), np.full(bins, count), centre


def _fit_cases():
    cases = {}
    cases["clean line"] = _line_bins(0.01, 4e-4)
    cases["noisy line"] = _line_bins(0.01, 4e-4, noise=0.1, seed=1)
    cases["a < 0"] = _line_bins(-0.004, 6e-3, noise=0.05, seed=2)          # falling variances: a = 0, b the weighted mean
    cases["b < 0"] = _line_bins(0.02, -2e-3, noise=0.05, seed=3)           # a line through a negative intercept: b = 0
    s, c, x = _line_bins(0.01, 4e-4, noise=0.1, seed=4)
    c = c.copy()
    c[::3] = 10                                                            # some bins below min_count
    c[5] = 0
    cases["thin bins"] = (s, c, x)
    c1 = np.zeros(32, dtype=np.int64)
    c1[7] = 900
    cases["one usable bin"] = (s, c1, x)
    cases["no usable bin"] = (s, np.full(32, 3), x)
    return cases


@pytest.mark.parametrize("name", list(_fit_cases()))
def test_fit_bins_on_cpu_tensors_equals_the_restated_fit(name):
    s, c, x = _fit_cases()[name]
    fallback = 1.25e-3
    want = R.fit(s, c, x, fallback=fallback)
    got = cva.nle.nlf_fit_bins(torch.from_numpy(s)[None, None], torch.from_numpy(c)[None, None], torch.from_numpy(x),
                               fallback=fallback)
    assert got[0].shape == got[1].shape == (1, 1) and got[0].dtype == torch.float64
    a, b = float(got[0]), float(got[1])
    assert a >= 0 and b >= 0
    assert abs(a - want[0]) <= 1e-10 and abs(b - want[1]) <= 1e-10, (name, (a, b), want)
    if name == "a < 0":
        assert a == 0 and b > 0
    if name == "b < 0":
        assert b == 0 and a > 0
    if name == "one usable bin":
        assert (a, b) == (0.0, float(s[7]) ** 2)
    if name == "no usable bin":
        assert (a, b) == (0.0, fallback)
        assert [float(t) for t in cva.nle.nlf_fit_bins(torch.from_numpy(s), torch.from_numpy(c), torch.from_numpy(x))] == [0, 0]


def test_fit_bins_is_batched_and_takes_the_device_dtypes():
    """Every case above in one call, shaped like a clip's bins (N,1,D,bins), float32 sigma and int32 counts as
    nlf_bins returns them, a fallback per image; other min_count and iters."""
    cases = list(_fit_cases().values())
    s = torch.tensor(np.stack([c[0] for c in cases]), dtype=torch.float32).reshape(1, 1, len(cases), 32)
    c = torch.tensor(np.stack([c[1] for c in cases]), dtype=torch.int32).reshape(1, 1, len(cases), 32)
    x = torch.from_numpy(cases[0][2])
    fb = torch.arange(1, len(cases) + 1, dtype=torch.float64).reshape(1, 1, -1) * 1e-4
    for min_count, iters in ((64, 2), (5, 0), (600, 3)):
        a, b = cva.nle.nlf_fit_bins(s, c, x, min_count=min_count, iters=iters, fallback=fb)
        assert a.shape == b.shape == (1, 1, len(cases))
        for i in range(len(cases)):
            want = R.fit(s[0, 0, i].double().numpy(), c[0, 0, i].numpy(), x.numpy(), min_count, iters, float(fb[0, 0, i]))
            assert abs(float(a[0, 0, i]) - want[0]) <= 1e-10 and abs(float(b[0, 0, i]) - want[1]) <= 1e-10, (i, min_count)


def test_restated_map():
    y = np.random.default_rng(0).random((3, 12, 15))
    m = R.image_map(y, 0.5, 0.01, smooth=1, floor=0.0)
    assert np.allclose(m, np.sqrt(0.5 * y.mean(axis=0) + 0.01), rtol=1e-14)
    assert np.allclose(R.image_map(np.full((1, 12, 15), 0.3), 0.5, 0.01, smooth=7), np.sqrt(0.16), rtol=1e-14)
    assert float(R.image_map(y, 0.0, 0.0, floor=2e-3).min()) == 2e-3
    p = torch.nn.functional.pad(torch.from_numpy(y.mean(axis=0))[None, None], (3, 3, 3, 3), mode="reflect")
    box = torch.nn.functional.avg_pool2d(p, 7, stride=1)[0, 0].numpy()
    assert np.allclose(R.image_map(y, 1.0, 0.0, smooth=7, floor=0.0), np.sqrt(box), rtol=1e-13)
    assert R.code_map(y[None], s=2).shape == (1, 1, 6, 8)


# ------------------------------------------------------------------------------------------------ ABI and surface
def test_abi_symbols_and_refusals():
    lib = cva._lib.lib()
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    assert re.search(r"\bint cdl_nle_nlf_bins\(", header) and re.search(r"\bsize_t cdl_nle_nlf_bins_scratch_floats\(", header)
    assert "cdl_nle_nlf_bins" in cva._lib.SIGNATURES and "cdl_nle_nlf_bins_scratch_floats" in cva._lib.SIZE_T_FUNCS
    assert hasattr(ctypes.CDLL(cva._lib.LIB_PATH), "cdl_nle_nlf_bins")
    n = int(lib.cdl_nle_nlf_bins_scratch_floats(2, 3, 64, 40))
    assert n == 2 * 2 * 3 * 28 * 16 == 2 * int(lib.cdl_nle_mad_scratch_floats(2, 3, 64, 40))        # two bands
    assert lib.cdl_nle_nlf_bins_scratch_floats(1, 1, 9, 64) == 0             # smaller than the filter
    bad = cva._lib.CDL_EINVAL
    call = lambda y, s, c, sc, H=64, W=40, bins=32, lo=0.0, hi=1.0, room=n: lib.cdl_nle_nlf_bins(
        y, s, c, sc, room, 2, 3, H, W, bins, lo, hi, None)
    assert call(None, _FAKE, _FAKE, _FAKE) == bad
    assert call(_FAKE, None, _FAKE, _FAKE) == bad
    assert call(_FAKE, _FAKE, None, _FAKE) == bad
    assert call(_FAKE, _FAKE, _FAKE, None) == bad
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, H=9) == bad                      # image smaller than the filter
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, W=9) == bad
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, bins=0) == bad
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, lo=0.5, hi=0.5) == bad            # hi <= lo
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, lo=0.5, hi=0.25) == bad
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, room=n - 1) == bad               # scratch too small: one band is not enough
    assert call(_FAKE, _FAKE, _FAKE, _FAKE, room=n // 2) == bad


def test_launch_statements_of_the_file_are_the_five_there_were():
    spec = importlib.util.spec_from_file_location("launch_coverage", os.path.join(ROOT, "tools", "launch_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ids = [s.id for s in mod.scan_sources() if s.file == "cdl_nle.hip"]
    assert ids == ["cdl_nle.hip:k_hh_abs", "cdl_nle.hip:k_select", "cdl_nle.hip:k_hh_abs#2",
                   "cdl_nle.hip:k_select_cells<true>", "cdl_nle.hip:k_select_cells<false>"]


def test_python_surface_and_refusals():
    for name in ("nlf_bins", "nlf_fit_bins", "nlf_fit", "nlf_map"):
        assert callable(getattr(cva.nle, name))
    y = torch.zeros(1, 1, 16, 16)
    for fn in (cva.nle.nlf_bins, cva.nle.nlf_fit):
        with pytest.raises(ValueError, match="bins"):
            fn(y, bins=0)
        with pytest.raises(ValueError, match="hi"):
            fn(y, lo=0.5, hi=0.5)
        with pytest.raises(RuntimeError, match="cpu"):                       # no CPU compute path
            fn(y)
    for smooth in (0, 4, -3):
        with pytest.raises(ValueError, match="smooth"):
            cva.nle.nlf_map(y, 0.1, 0.1, smooth=smooth)
    with pytest.raises(ValueError, match="together"):
        cva.nle.nlf_map(y, a=0.1)
