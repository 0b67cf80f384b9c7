"""The plans of the fused generic tier (cdl_fusedg_*: tile, strip and grouped strip kernel behind one set of entry points)
through the library's host-only size queries -- no GPU.  tests/golden/fusedg_plans.json holds the answers recorded by
tools/make_golden_fusedg_plans.py from the library before the three plan structs became one: which geometries are
supported, the sizes of every buffer a caller allocates, and the code layout, with CDL_FUSEDG_STRIP=0 and =1."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

ENTRIES = json.load(open(os.path.join(GOLDEN, "fusedg_plans.json")))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_golden_fusedg_plans",
                                                  os.path.join(ROOT, "tools", "make_golden_fusedg_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_tool_geometry_list(tool):
    assert [e["geom"] for e in ENTRIES] == tool.geometries()
    kinds = {(e["strip0"]["supported"], e["strip0"]["code_layout"][0], e["strip1"]["code_layout"][0]) for e in ENTRIES}
    # unsupported; tile kernel only; tile kernel or, when switched on, the grouped strip kernel; strip kernel
    assert kinds == {(0, 0, 0), (1, 0, 0), (1, 0, 3), (1, 3, 3)}


def test_plans_equal_the_recorded_ones(tool, hip_env):
    got = tool.record(hip_env)
    assert len(got) == len(ENTRIES)
    bad = [(e["geom"], key) for e, r in zip(got, ENTRIES) for key in ("strip0", "strip1") if e[key] != r[key]]
    assert not bad, bad


def test_strip_plan_refuses_codes_beyond_the_descriptor_range():
    """A sample's code tensor must stay below 2^31 bytes in BOTH layouts the strip kernel addresses through a buffer
    descriptor.  With M = 96, stride 1 and an image of (4, 1398081) the (N,M,..) layout fits and the padded row-strip
    layout (43691 strips of 32 columns) does not: such a geometry is unsupported -- it runs on the generic tier -- instead
    of failing at its first launch.  One strip fewer is supported."""
    import cdlnet_video_amd as cva
    lib = cva._lib.lib()

    def ask(W, M=96, H=4, P=3, s=1):
        gs = cva._lib.Geom(1, 1, M, 1, H, W, 1, P, P, 0, P // 2, P // 2, 1, s, s)
        ref = ctypes.byref(gs)
        return int(lib.cdl_fusedg_supported(ref)), int(lib.cdl_fusedg_code_floats(ref, 3)), int(lib.cdl_fusedg_code_layout(ref, 0))

    assert ask(1398081) == (0, 0, 0)
    sup, rsc, lay = ask(1398049)
    assert (sup, lay) == (1, 3) and rsc == 96 * 4 * 43690 * 32 and rsc * 4 < 2 ** 31
    seen = set()
    for M, H, P, s, W0 in ((96, 4, 3, 1, 1398049), (169, 2, 7, 2, 6353474), (72, 8, 5, 1, 932065)):
        for W in range(W0 - 2000 * s, W0 + 2000 * s, s):
            sup, rsc, lay = ask(W, M, H, P, s)
            seen.add(sup)
            assert rsc * 4 < 2 ** 31, (M, H, W, rsc)
            assert (sup == 1) == (rsc > 0) and lay == (3 if sup else 0), (M, H, W)
    assert seen == {0, 1}
