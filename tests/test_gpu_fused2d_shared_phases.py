"""The fused 2-D tier after k_stage and k_wgrad2d came to share one copy of their common device phases (DESIGN.md
section 34), against the record made on the commit before (tools/make_golden_fused2d_shared_phases_parent_bits.py): every
value bit for bit -- the change moves text and keeps the order of every floating-point sum, so there is no tolerance.
The record covers what the earlier stage-tile-phase record does not: the split4 and bf16 arithmetic, the bf16 storage
layout (the 64 x 32 stage and the LAY_BLK16 k_wgrad2d), the map forms with dL/dcmap, k_wgrad2d with one operator and
with two, and the tangent sweep; 40 x 150 with CDL_FUSED_GRID=4 has partial tiles in both axes, several tiles per
workgroup, a walk into the next image and past the last tile."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_fused2d_shared_phases_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_fused2d_shared_phases_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _record():
    """One record in several files (the tool's save_parts: no committed file reaches 1 MiB)."""
    return _tool().load_parts(os.path.join(ROOT, "tests", "golden", "f2d_shared_phases_parent_bits.npz"))


_CASES = _tool().CASES


def test_the_record_holds_the_cases_and_nothing_else():
    mod, want = _tool(), _record()
    mp = ("M64P7", "M32P5")
    cells = ("split3/blocked", "split4/blocked", "bf16/blocked", "split3/nchw", "split3/blocked_bf16")
    train = [f"train/{m}/{c}/{g}" for m in mp for c in cells for g in ("g4", "gdef")] + \
            [f"train/{m}/split3/blocked/g4/da0" for m in mp]
    maps = [f"map/{m}/{lay}/{g}" for m in mp for lay in ("blocked", "nchw") for g in ("g4", "gdef")]
    steps = [f"step/{m}/{p}/{lay}" for m in mp for p in ("split3", "split4") for lay in ("nchw", "blocked")]
    jvps = [f"jvp/{m}" for m in mp]
    assert sorted(mod.TRAIN_CASES) == sorted(train) and sorted(mod.MAP_CASES) == sorted(maps)
    assert sorted(mod.STEP_CASES) == sorted(steps) and sorted(mod.JVP_CASES) == sorted(jvps)
    assert mod.CASES == mod.TRAIN_CASES + mod.MAP_CASES + mod.STEP_CASES + mod.JVP_CASES and len(mod.CASES) == 40
    assert (mod.N, mod.C, mod.SP, mod.K_TRAIN, mod.K_JVP, mod.CAPPED) == (2, 1, (40, 150), 3, 2, "4")
    names = {f"{case}/{q}" for case in train + maps for q in ("xhat", "z", "dy", "dsigma", "dt", "dA", "dB")}
    names |= {f"{case}/{q}" for case in jvps for q in ("xhat", "xdot", "dt", "dA", "dB")}
    for case in steps:
        names |= {f"{case}/iter/{q}" for q in ("z", "patches", "map")}
        names |= {f"{case}/{s}/{q}" for s in ("bwd", "bwd_da") for q in ("du", "patches", "dtau_partial")}
        names |= {f"{case}/bwd_da/dA", f"{case}/wgrad1/d0", f"{case}/wgrad2/d0", f"{case}/wgrad2/d1"}
    assert sorted(want) == sorted(names)
    for case in maps:                                        # dL/dcmap: one value per pixel of the map
        assert want[case + "/dsigma"].shape == (2, 1, 40, 150)


@pytest.mark.parametrize("case", _CASES)
def test_values_keep_the_parent_commits_bits(case, hip_env):
    want, got = _record(), _tool().compute_case(case, hip_env)
    assert got and all(k.startswith(case + "/") for k in got)
    assert sorted(got) == sorted(k for k in want if k.startswith(case + "/") and (case + "/da0/") not in k)
    differ = {}
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64) and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            differ[k] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert not differ, differ
