"""The workspace sizes of the generic operators after their tier ladder moved into cdl_operators.hip (DESIGN.md section
37), through the library's host-only size queries -- no GPU.  tests/golden/operator_ladder_parent_sizes.json holds what the
commit before answered (tools/make_golden_operator_ladder_parent_sizes.py): the four *_workspace_floats,
cdl_ista_scratch_floats and cdl_residual_scratch_floats, for the geometries of test_gpu_dispatch.py, the ResidualBlock and
VGG16 geometries of their tests and the edges of the tiled filter gradient's and the dense tier's plan rules, under every
switch setting of test_gpu_dispatch.py's ENV, each also with cdl_set_exact_fp32(1).  Equality, with one named exception:
under CDL_NO_TILED the parent's cdl_wgrad_workspace_floats counts rungs that cannot run, so there -- and nowhere else --
the answer may be the parent's or 0."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT
from test_gpu_dispatch import ENV

RECORD = json.load(open(os.path.join(GOLDEN, "operator_ladder_parent_sizes.json")))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_golden_operator_ladder_parent_sizes",
                                                  os.path.join(ROOT, "tools", "make_golden_operator_ladder_parent_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_record_covers_the_tool_geometries_and_every_setting(tool):
    assert RECORD["funcs"] == tool.FUNCS and RECORD["geoms"] == tool.geometries()
    assert sorted(RECORD["sizes"]) == sorted(ENV)
    n = len(RECORD["geoms"])
    assert all(len(RECORD["sizes"][s][e]) == n for s in ENV for e in ("exact0", "exact1"))
    # the record is not blind: the sizes that can be zero are zero somewhere and not elsewhere (the reverse step has its
    # floor, the filter gradient and the sweep always a kernel with partial banks), and the switches move them
    rows = [r for s in ENV for e in ("exact0", "exact1") for r in RECORD["sizes"][s][e]]
    always = {"cdl_analysis_rev_workspace_floats", "cdl_wgrad_workspace_floats", "cdl_ista_scratch_floats"}
    for i, f in enumerate(tool.FUNCS):
        assert {bool(r[i]) for r in rows} == ({True} if f in always else {False, True}), f
    sizes = RECORD["sizes"]
    assert sizes["mfma"]["exact0"] != sizes["mfma"]["exact1"] and sizes["mfma"]["exact0"] != sizes["tiled"]["exact0"]
    assert sizes["tiled"]["exact0"] != sizes["plain"]["exact0"]


@pytest.mark.parametrize("setting", sorted(ENV))
def test_sizes_equal_the_parent_commits(setting, tool, hip_env):
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the record holds for 256 compute units (also what the library plans for without a device); this "
                    f"device has {torch.cuda.get_device_properties(0).multi_processor_count}")
    got, want = tool.record(setting, hip_env), RECORD["sizes"][setting]
    wgrad = tool.FUNCS.index("cdl_wgrad_workspace_floats")
    bad = []
    for e in ("exact0", "exact1"):
        for g, a, b in zip(RECORD["geoms"], got[e], want[e]):
            for i, f in enumerate(tool.FUNCS):
                ok = a[i] == b[i] or ("CDL_NO_TILED" in ENV[setting] and i == wgrad and a[i] == 0)
                if not ok:
                    bad.append((e, g, f, a[i], b[i]))
    assert not bad, bad[:20]
