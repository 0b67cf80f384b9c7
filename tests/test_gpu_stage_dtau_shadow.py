"""The fused 2-D reverse stage against the record made on the commit before its threshold-gradient partials moved under the
synthesis MFMAs and their per-tile exchange left LDS (tools/make_golden_stage_dtau_shadow_parent_bits.py; DESIGN.md
section 5.6): every value bit for bit -- the change is scheduling and data movement only, so there is no tolerance.

The step-wise cases write the support/sign maps themselves (empty, full, all signs negative, one channel, one pixel column,
and bits that follow the bits of the lane number) so that a wrong exchange between lanes c and c ^ 1, 2, 4, 8, 16 of the
per-tile transposition shows in `dtau_partial`; the K = 3 training steps walk the tiles in both directions, several per
workgroup, on both tile heights.  20 x 70 and 33 x 65 leave a partial tile on both axes.

On the CPU: the order in which LaneTransposeSum<16> (cdl_wave_dev.h) adds, restated in numpy float32 -- a halving
butterfly in which lane c keeps the half of its values that bit n of c selects and receives the same half from lane c ^ n --
against the plain sums in lane order, for the same patterns."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_stage_dtau_shadow_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_stage_dtau_shadow_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _record():
    return np.load(os.path.join(ROOT, "tests", "golden", "t2_stage_dtau_shadow_parent_bits.npz"))


_CASES = _tool().CASES


def _expected_names(mod):
    names = set()
    for case in mod.STEP_CASES:
        for pat in mod.PATTERNS:
            for s in ("bwd", "bwd_nosynth", "bwd_da"):
                names |= {f"{case}/{pat}/{s}/{q}" for q in ("du", "patches", "dtau_partial")}
            names.add(f"{case}/{pat}/bwd_da/dA")
    for case in mod.STEPMAP_CASES:
        for pat in ("full", "lanes"):
            for s in ("bwd", "bwd_da"):
                names |= {f"{case}/{pat}/{s}/{q}" for q in ("du", "patches", "dtau_partial", "dcmap")}
            names.add(f"{case}/{pat}/bwd_da/dA")
    for case in mod.TRAIN_CASES:
        names |= {f"{case}/{q}" for q in ("xhat", "z", "dy", "dsigma", "dt", "dA", "dB")}
    for case in mod.TRAINMAP_CASES:
        names |= {f"{case}/{q}" for q in ("xhat", "z", "dy", "dcmap", "dt", "dA", "dB")}
    return names


def test_the_record_holds_the_cases_and_nothing_else():
    mod, want = _tool(), _record()
    assert (len(mod.STEP_CASES), len(mod.STEPMAP_CASES), len(mod.TRAIN_CASES), len(mod.TRAINMAP_CASES)) == (16, 4, 10, 1)
    assert sorted(want.files) == sorted(_expected_names(mod))
    # the partials of the patterns differ from each other: the record can tell a wrong exchange from a right one
    full, lanes = (want[f"step/M64P7/blocked/split3/{p}/bwd/dtau_partial"] for p in ("full", "lanes"))
    # (33 x 65: the second tile column is the one pixel column x = 64, whose low five bits are clear -- no support there)
    assert not np.array_equal(full, lanes) and np.count_nonzero(lanes) == lanes.size // 2 and np.count_nonzero(full) == full.size
    one = want["step/M64P7/blocked/split3/onechannel/bwd/dtau_partial"]
    assert np.count_nonzero(one[:, 13]) == one.shape[0] and np.count_nonzero(np.delete(one, 13, axis=1)) == 0
    assert np.count_nonzero(want["step/M64P7/blocked/split3/empty/bwd/dtau_partial"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", _CASES)
def test_values_keep_the_parent_commits_bits(case, hip_env):
    want, got = _record(), _tool().compute_case(case, hip_env)
    assert got and all(k.startswith(case + "/") for k in got)
    differ = {}
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64) and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            differ[k] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert not differ, differ


# ---- LaneTransposeSum<16>'s order of additions, on the CPU ---------------------------------------------------------------
def _lane_transpose_sum16(v):
    """v[lane, i], 32 lanes x 16 values (float32) -> r[lane]: what LaneTransposeSum<16>::run leaves on each lane of a half-wave.
    Step n = 8, 4, 2, 1: lane c keeps w[k] = v[k + n] if c & n else v[k] and adds what lane c ^ n sends -- that lane's copy of
    the same index -- as keep + received, in float32."""
    w = np.asarray(v, dtype=np.float32)
    lanes = np.arange(w.shape[0])
    n = w.shape[1] // 2
    while n >= 1:
        up = (lanes & n) != 0
        keep = np.where(up[:, None], w[:, n:2 * n], w[:, :n])
        send = np.where(up[:, None], w[:, :n], w[:, n:2 * n])
        w = (keep + send[lanes ^ n]).astype(np.float32)
        n //= 2
    return w[:, 0]


def _in_lane_order(v, i, c):
    """The same additions read off the tree instead of the register shuffle: after the step at distance d a lane holds, for an
    index it kept, (what it held before) + (what lane ^ d held before), and before the first step (d = 8) its own value."""
    def after(lane, d):
        if d == 16:
            return np.float32(v[lane, i])
        return np.float32(after(lane, 2 * d) + after(lane ^ d, 2 * d))
    return after(c, 1)


def _patterns(rng):
    lanes = np.arange(32)
    base = rng.standard_normal((32, 16)).astype(np.float32)
    yield "empty", np.zeros((32, 16), np.float32)
    yield "full", base
    yield "allneg", -np.abs(base)
    one = np.zeros_like(base)
    one[:, 5] = base[:, 5]
    yield "onechannel", one
    col = np.zeros_like(base)
    col[5] = base[5]
    yield "onecolumn", col
    lane_bits = np.stack([np.where((lanes >> (i % 5)) & 1, base[:, i], np.float32(0)) for i in range(16)], 1)
    yield "lanes", lane_bits.astype(np.float32)
    yield "magnitudes", (base * np.float32(10.0) ** rng.integers(-6, 7, size=(32, 16))).astype(np.float32)


def test_lane_transpose_sum_order_restated():
    rng = np.random.default_rng(5)
    for name, v in _patterns(rng):
        r = _lane_transpose_sum16(v)
        for c in range(32):
            i = c % 16                       # lane c ends with (its half of) total #(c mod 16): lanes c and c ^ 16 hold the two halves
            want = _in_lane_order(v, i, c)
            assert r[c].tobytes() == np.float32(want).tobytes(), (name, c)
            group = (c & 16) + np.arange(16)  # the 16 lanes whose values it holds
            exact = v[group, i].astype(np.float64).sum()
            scale = np.abs(v[group, i]).astype(np.float64).sum()
            assert abs(float(r[c]) - exact) <= 4 * 2.0 ** -24 * scale, (name, c)    # 4 roundings deep: log2(16) float32 additions
        total = r[:16].astype(np.float32) + r[16:].astype(np.float32)              # lane_transpose_sum's last step (c ^ 16)
        exact = v.astype(np.float64).sum(0)
        assert np.all(np.abs(total - exact) <= 5 * 2.0 ** -24 * np.abs(v).astype(np.float64).sum(0)), name
