"""The fused 2-D tier with several tiles per workgroup and partial tiles in both axes, against the record made on the
commit before the stage kernel's per-tile phase changed (tools/make_golden_stage_tile_phase_parent_bits.py; DESIGN.md
section 5.2g): every value bit for bit -- the change is data movement and scheduling only, so there is no tolerance.
CDL_FUSED_GRID=4 gives the workgroups 5, 5, 4 and 4 of the 18 tiles: the next tile's thin inputs are then loaded across
an image boundary and past the last tile; the default grid has one tile per workgroup.  CDL_FUSED_DA=0 is the form in
which the last reverse stage's du_0 must still reach memory (k_wgrad2d reads it)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_stage_tile_phase_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_stage_tile_phase_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _record():
    return np.load(os.path.join(ROOT, "tests", "golden", "t1_stage_tile_phase_parent_bits.npz"))


_CASES = _tool().CASES


def test_the_record_holds_the_cases_and_nothing_else():
    mod, want = _tool(), _record()
    assert len(mod.TRAIN_CASES) == 17 and len(mod.STEP_CASES) == 4
    names = set()
    for case in mod.TRAIN_CASES:
        names |= {f"{case}/{q}" for q in ("xhat", "z", "dy", "dsigma", "dt", "dA", "dB")}
    for case in mod.STEP_CASES:
        names |= {f"{case}/iter/{q}" for q in ("z", "patches", "map")}
        names |= {f"{case}/{s}/{q}" for s in ("bwd", "bwd_da") for q in ("du", "patches", "dtau_partial")}
        names.add(f"{case}/bwd_da/dA")
    assert sorted(want.files) == sorted(names)


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
