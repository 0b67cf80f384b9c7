"""The generic operators after their tier ladder moved into cdl_operators.hip and the dense tier's host side was folded
(DESIGN.md section 37), against the record made on the commit before (tools/make_golden_operator_ladder_parent_bits.py): the
same launch sites and every value byte for byte -- the change moves host text only, so there is no tolerance.  The cases are
every (tier, key) at which test_gpu_dispatch.py pins a launch site, through the calls it makes there, and the dense tier
(held to its own past output here, to the float64 model cell by cell in test_gpu_dense_cells.py): cdl_dense_conv in both
roles, cdl_dense_wgrad, the ResidualBlock and the perceptual loss (every form of cdl_dense_vgg)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_dispatch as D
from conftest import ROOT

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_operator_ladder_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_operator_ladder_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _record():
    """One record in several files (save_parts of the mfma_tier_parent_bits tool: no committed file reaches 1 MiB)."""
    return _tool().load_parts(os.path.join(ROOT, "tests", "golden", "operator_ladder_parent_bits.npz"))


_CASES = _tool().CASES


def _strings(obj, out):
    if isinstance(obj, str):
        if ".hip:" in obj:
            out.add(obj)
    elif isinstance(obj, dict):
        _strings(list(obj.values()), out)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            _strings(v, out)
    return out


def test_the_record_holds_the_cases_and_nothing_else():
    mod, want = _tool(), _record()
    assert len(set(mod.CASES)) == len(mod.CASES)
    assert sorted(want) == sorted(n for case in mod.CASES for n in mod.array_names(case))
    # the dense tier's cases, as DESIGN.md section 37 lists them
    conv = ["N1C24M40_17x33_P3x3_s1", "N1C24M40_17x33_P5x5_s1", "N1C24M40_2x17x33_P3x3x3_s1"]
    wg = [f"N1C{C}M{M}_2x9x{W}_P3x3x3_s1" for C, M in ((24, 24), (40, 72)) for W in (33, 36)]
    assert all(f"{kind}/mfma/{k}" in mod.CASES for kind in ("ana", "syn") for k in conv)
    assert all(f"wg/mfma/{k}" in mod.CASES for k in wg)
    assert mod.CASES[-2:] == ["residual/4x8x8", "perceptual/3x37x50"]
    den = "cdl_dense_mfma.hip:"
    for k in conv:                                           # on the dense tier, both roles, every call
        for kind in ("ana", "syn"):
            assert all(den + "k_dense<MT>" in mod.sites_of(want[f"{kind}/mfma/{k}/{c}/sites"]) for c in mod.CALLS[kind]), k
    for k in wg:                                             # scalar loads at W = 33, 16-byte loads at W = 36; filter gradients in full
        vec = "true" if k.split("_")[1].endswith("36") else "false"
        assert all(den + f"k_dense_wgrad<{vec}>" in mod.sites_of(want[f"wg/mfma/{k}/{c}/sites"]) for c in ("plain", "gated"))
        C, M = (24, 24) if "C24" in k else (40, 72)
        assert all(want[f"wg/mfma/{k}/{n}"].shape == (M, C, 3, 3, 3) for n in ("plain/dw", "gated/dw", "pair/dw0", "pair/dw1"))
    vgg = set(mod.sites_of(want["perceptual/3x37x50/fwd/sites"])) | set(mod.sites_of(want["perceptual/3x37x50/bwd/sites"]))
    assert {den + "k_dense_vgg<MODE>", den + "k_dense<MT>", den + "k_dense_prep#2"} <= vgg
    # every launch site test_gpu_dispatch.py pins is in some recorded site list: its constants, its parametrize tables, and the
    # sites it names inside test bodies
    pinned = _strings([v for k, v in vars(D).items() if k.isupper()], set())
    for name, fn in vars(D).items():
        if name.startswith("test_"):
            _strings([m.args for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"], pinned)
    pinned |= {D.GEN + k for k in ("k_analysis<false>", "k_synthesis", "k_wgrad", "k_tau_partial<true,false>")}
    pinned |= {D.ANA + "k_ana_tau_final<false>", D.DEN + "k_dense<MT>", D.DEN + "k_dense_wgrad<true>",
               D.DEN + "k_dense_wgrad<false>", D.DEN + "k_dense_wfold"}
    pinned = {s for s in pinned if not s.endswith(":")}     # (the file prefixes themselves)
    seen = {s for k, v in want.items() if k.endswith("/sites") for s in mod.sites_of(v)}
    assert pinned <= seen, sorted(pinned - seen)


@pytest.mark.parametrize("case", _CASES)
def test_route_and_values_keep_the_parent_commits_bits(case, hip_env):
    want, got = _record(), _tool().compute_case(case, hip_env)
    assert got and sorted(got) == sorted(k for k in want if k.startswith(case + "/"))
    differ = {}
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if k.endswith("/sites"):
            assert _tool().sites_of(a) == _tool().sites_of(b), k
            continue
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64) and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            differ[k] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert not differ, differ
