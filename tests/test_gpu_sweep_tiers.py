"""The sweep tiers through the nets' public calls, against the record made on the commit before the tiers got one route,
one table, one fused-sweep wrapper and one host loop (tools/make_golden_sweep_tiers_parent_bits.py; DESIGN.md section
5.3): every value bit for bit -- the change moves host code only, so there is no tolerance -- and, per case, the same
launches in the same order."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = ["generic/train", "generic/tangent", "generic/map", "generic/fp32", "fused/blocked/train", "fused/blocked/tangent",
         "fused/nchw/train", "fused/nchw/tangent", "tile/train", "tile/tangent", "strip/train", "strip/tangent",
         "strip/generator"]


@functools.lru_cache(maxsize=None)
def _record():
    """(what the parent commit recorded, what this commit computes): one run of every case, shared by the tests."""
    spec = importlib.util.spec_from_file_location("make_golden_sweep_tiers_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_sweep_tiers_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return np.load(os.path.join(ROOT, "tests", "golden", "t0_sweep_tiers_parent_bits.npz")), mod.compute()


def _of(case, names):
    return sorted(k for k in names if k.rpartition("/")[0] == case)


def test_the_record_holds_the_cases_and_nothing_else():
    want, got = _record()
    assert sorted(got) == sorted(want.files)
    assert sorted({k.rpartition("/")[0] for k in got}) == sorted(CASES)
    for case in CASES:
        names = {k.rpartition("/")[2] for k in _of(case, got)}
        assert {"xhat", "dt", "dA", "dB", "launches"} <= names, case
        if case.endswith("tangent"):
            assert {"xdot", "z", "zd"} <= names, case
        elif case != "strip/generator":
            assert {"z", "dy", "dsigma"} <= names, case
    assert {"strip/generator/codes"} <= set(got)


@pytest.mark.parametrize("case", CASES)
def test_values_keep_the_parent_commits_bits(case):
    want, got = _record()
    differ = {}
    for k in _of(case, got):
        if k.endswith("/launches"):
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64) and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            differ[k] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert not differ, differ


@pytest.mark.parametrize("case", CASES)
def test_launches_are_the_parent_commits_in_its_order(case):
    want, got = _record()
    a, b = [str(s) for s in got[case + "/launches"]], [str(s) for s in want[case + "/launches"]]
    assert len(b) > 10
    assert a == b, [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:5]
