"""The sparse matrix-core tier after its three files came to share one plane gate, one plane dispatch, the device pieces of
cdl_wave_dev.h and one filter-gradient entry, against the record made on the commit before
(tools/make_golden_mfma_tier_parent_bits.py): every value bit for bit -- the change moves text and keeps the order of
every floating-point sum, so there is no tolerance.  The cases are the cells of test_gpu_generic_cells.py on their own
seeded data, every form of every kernel, plus a K = 2 sweep of a strip shape through the folded filter-gradient entry with
the codes in the "rsc" layout and forced to "nchw"."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_generic_cells as T
from conftest import ROOT

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_mfma_tier_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_mfma_tier_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _record():
    """One record in several files (the tool's save_parts: no committed file reaches 1 MiB)."""
    return _tool().load_parts(os.path.join(ROOT, "tests", "golden", "mfma_tier_parent_bits.npz"))


_CASES = _tool().CASES


def test_the_record_holds_the_cases_and_nothing_else():
    mod, want = _tool(), _record()
    ana = [f"ana/{c.id}" for c in T.ANA_CELLS + T.SIGN_MIXED]
    syn = [f"syn/{c.id}" for c in T.SYN_CELLS]
    wgm = [f"wgm/{c.id}" for c in T.WGM_CELLS]
    assert mod.CASES == ana + syn + wgm + ["strip/rsc", "strip/nchw"] and len(set(mod.CASES)) == len(mod.CASES)
    assert mod.STRIP == dict(K=2, M=100, P=7, s=1, shape=(1, 1, 33, 70))
    full = ["plain", "first", "iter", "gated", "map", "rev/du", "rev/dt", "revmap/du", "revmap/dt"] + \
           [f"{p}/{q}" for p in ("prox", "prox2", "proxmap", "prox2map") for q in ("z", "u")]
    names = {f"ana/{c.id}/{q}" for c in T.ANA_CELLS for q in full}
    names |= {f"ana/{c.id}/{q}" for c in T.SIGN_MIXED for q in ("first", "iter", "map")}
    names |= {f"{case}/{q}" for case in syn for q in ("vector", "scalar", "scalarW37")}
    names |= {f"{case}/{n}{tag}" for case in wgm for tag in ("", "W70") for n in ("single", "gated", "pair0", "pair1")}
    names |= {f"strip/{lay}/{q}" for lay in ("rsc", "nchw") for q in ("xp", "z", "dA", "dB", "dt")}
    assert sorted(want) == sorted(names)
    for c in T.ANA_CELLS:                                    # threshold sums in full
        assert want[f"ana/{c.id}/rev/dt"].shape == want[f"ana/{c.id}/revmap/dt"].shape == (2, c.M)
    for c in T.WGM_CELLS:                                    # filter gradients in full
        G, plane = int(np.prod((c.C,) + c.P[:-2])), c.P[-2:]
        assert all(want[f"wgm/{c.id}/{n}"].shape[0] == c.M and want[f"wgm/{c.id}/{n}"].size == c.M * G * plane[0] * plane[1]
                   for n in mod.WGM_NAMES)
    for lay in ("rsc", "nchw"):
        assert want[f"strip/{lay}/dA"].shape == want[f"strip/{lay}/dB"].shape == (2, 100, 1, 7, 7)


@pytest.mark.parametrize("case", _CASES)
def test_values_keep_the_parent_commits_bits(case, hip_env):
    want, got = _record(), _tool().compute_case(case, hip_env)
    assert got and all(k.startswith(case + "/") for k in got)
    assert sorted(got) == sorted(k for k in want if k.startswith(case + "/"))
    differ = {}
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64) and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            differ[k] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert not differ, differ
