"""What the sweep-tiers record does not reach -- the CSR sweeps, the matrix-core rungs of the generic tier, the residual
block on both of its branches, the VGG backward and the single-bank filter calls -- against the record made on the commit
before the `_ws` pairs and the single-bank forms became one entry point per operator
(tools/make_golden_entry_points_parent_bits.py): every value bit for bit -- the change moves host
code only, so there is no tolerance -- and, per case, the same launches in the same order.  The single-bank calls are the
one place where the launches changed on purpose: they must name the batch kernels."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = ["csr/f1/train", "csr/f2/train", "csr/f2/map", "csr/f2/tangent", "mfma/train", "mfma/tangent", "mfma/csr",
         "residual/dense", "residual/valu", "vgg/step", "gabor/0", "gabor/1", "gabor/2", "project"]
# the launches of the single-bank calls after the fold (the parent ran k_gabor, k_gabor_bwd and k_project)
BATCH_SITES = {"gabor/0": ["cdl_generic.hip:k_gabor_batch", "cdl_generic.hip:k_gabor_bwd_batch"],
               "gabor/1": ["cdl_generic.hip:k_gabor_batch", "cdl_generic.hip:k_gabor_bwd_batch"],
               "gabor/2": ["cdl_generic.hip:k_gabor_batch", "cdl_generic.hip:k_gabor_bwd_batch"],
               "project": ["cdl_generic.hip:k_project_batch"]}
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_SYN = "cdl_synth_mfma.hip:k_synth_m<PH,PW,SW,"
K_WGM = "cdl_wgrad_mfma.hip:k_wgm<PH,PW,SW,NG,CT>"
# case -> (launch-site prefixes, (PROX, REV) pairs of k_ana_m) that must have run; the 3-D geometry has too few
# filter-gradient tiles for k_wgm (tests/test_gpu_dispatch.py)
MFMA_SITES = {"mfma/train": ((K_ANA, K_SYN, K_WGM), {(0, 0), (0, 1)}),
              "mfma/tangent": ((K_ANA, K_SYN), {(0, 1)}),
              "mfma/csr": ((K_ANA, K_SYN, K_WGM), {(1, 0)})}


@functools.lru_cache(maxsize=None)
def _record():
    """(what the parent commit recorded, what this commit computes): one run of every case, shared by the tests."""
    spec = importlib.util.spec_from_file_location("make_golden_entry_points_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_entry_points_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return np.load(os.path.join(ROOT, "tests", "golden", "t1_entry_points_parent_bits.npz")), mod.compute()


def _of(case, names):
    return sorted(k for k in names if k.rpartition("/")[0] == case)


def test_the_record_holds_the_cases_and_nothing_else():
    want, got = _record()
    assert sorted(got) == sorted(want.files)
    assert sorted({k.rpartition("/")[0] for k in got}) == sorted(CASES)
    for case in CASES:
        names = {k.rpartition("/")[2] for k in _of(case, got)}
        assert "launches" in names, case
        if case.startswith("csr/") or case == "mfma/csr":
            assert {"xhat", "z", "dzp", "d.t", "d.A.0.weight", "d.B.0.weight"} <= names, case
            assert {"xdot", "zd", "dzdp", "dzda"} <= names if case.endswith("tangent") else {"dy", "dsigma"} <= names, case
        elif case.startswith("mfma/"):
            assert {"xhat", "z", "dt", "dA", "dB", "ana"} <= names, case
        elif case.startswith("residual/"):
            assert {"xhat", "z", "d.t", "d.residual_blocks.0.conv1.weight", "d.residual_blocks.1.conv2.weight"} <= names
        elif case.startswith("gabor/"):
            assert names == {"w", "dalpha", "da", "dw0", "dpsi", "launches"}
    assert {"vgg/step/value", "vgg/step/doutput", "vgg/step/dtarget", "project/w"} <= set(got)
    assert got["csr/f2/map/dsigma"].shape == (2, 1, 13, 11)


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
    if case in BATCH_SITES:
        assert len(b) == len(BATCH_SITES[case])
        assert a == BATCH_SITES[case]
        return
    assert len(b) > 10
    assert a == b, [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:5]
    if case in MFMA_SITES:
        sites, variants = MFMA_SITES[case]
        missing = [s for s in sites if not any(x.startswith(s) for x in a)]
        missing += sorted(variants - set(map(tuple, got[case + "/ana"].tolist())))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if missing and cus != 256:      # the plans read the compute-unit count (tests/test_gpu_dispatch.py)
            pytest.skip(f"the shapes reach the matrix cores at 256 compute units, this device has {cus}: {missing}")
        assert not missing, missing
