"""The launch trace and the launch-coverage manifest, without a GPU.

The trace is host code: a launch that fails for want of a device is recorded all the same, so the library's record
format, the CDL_TRACE_FILE log and the tool's mapping of records onto the `kernel<<<...>>>` sites of the sources are
checked here.  On a machine with a device the same launch is made with real tensors."""
import ctypes
import importlib.util
import json
import os
import re

import pytest
import torch

import cdlnet_video_amd as cva
from conftest import ROOT

MANIFEST = os.path.join(ROOT, "tests", "launch_coverage.json")


def _tool():
    spec = importlib.util.spec_from_file_location("launch_coverage", os.path.join(ROOT, "tools", "launch_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _one_launch():
    """One cdl_thresholds call: k_thresholds of cdl_generic.hip."""
    if torch.cuda.is_available():
        cva.ops.thresholds(torch.zeros(2, 2, 3, 1, 1).cuda(), None, 1)
        return
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = cva._lib.lib().cdl_thresholds(p, None, p, 2, 1, 3, None)
    assert rc < 0 and rc not in (cva._lib.CDL_EINVAL, cva._lib.CDL_EUNSUPPORTED)     # a HIP error: no device


def test_trace_is_off_by_default_scoped_and_cleared_when_switched_on():
    lib = cva._lib.lib()
    assert lib.cdl_trace(0) == 0
    kept = lib.cdl_trace_read(None, 0)
    _one_launch()
    assert lib.cdl_trace_read(None, 0) == kept                   # off: nothing recorded
    with cva.ops.trace() as t:
        _one_launch()
        _one_launch()
        assert len(t.read()) == 2
    assert lib.cdl_trace(0) == 0                                 # the scope restored what it found
    assert [r.file for r in t] == ["cdl_generic.hip"] * 2 and "cdl_thresholds" in t[0].func
    with cva.ops.trace() as t2:                                  # switched on again: the log starts empty
        assert len(t2.read()) == 0
        small = ctypes.create_string_buffer(8)                   # a short buffer gets a cut, terminated copy
        _one_launch()
        assert lib.cdl_trace_read(small, 8) > 8 and len(small.value) == 7
    mod = _tool()
    assert mod.site_of(mod.index(mod.scan_sources()), (t[0].file, t[0].line, t[0].func, t[0].note)) == "cdl_generic.hip:k_thresholds"


def test_trace_records_from_another_thread():
    import threading
    with cva.ops.trace() as t:
        th = threading.Thread(target=_one_launch)
        th.start()
        th.join()
    assert len(t) == 1


def test_trace_file_gets_each_distinct_record_once(tmp_path, hip_env):
    path = tmp_path / "trace.log"
    hip_env("CDL_TRACE_FILE", str(path))
    kept = cva._lib.lib().cdl_trace_read(None, 0)
    for _ in range(3):
        _one_launch()
    assert cva._lib.lib().cdl_trace_read(None, 0) == kept        # the in-process log stays off
    lines = path.read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("cdl_generic.hip:") and lines[0].count("\t") == 2
    assert [r.file for r in cva.ops.parse_trace(path.read_text())] == ["cdl_generic.hip"]


def test_record_parsing():
    text = ("cdl_analysis_mfma.hip:441\tint (anonymous namespace)::launch_mtp(const cdl_geom *) "
            "[PH = 9, PW = 5, SW = 2, MT = 1, PROX = false, REV = true, MAP = false]\tMTW=1 tpw=4 ngy=2 lds_over_96k=1 wgs=96\n"
            "# test tests/test_x.py::test_y\n"
            "cdl_generic_tiled.hip:900\tint cdl_tiled_wgrad(const cdl_geom *)\tk_wgrad_l<7,7,1> tiles=64\n")
    a, b = cva.ops.parse_trace(text)
    assert (a.file, a.line) == ("cdl_analysis_mfma.hip", 441)
    assert a.template() == {"PH": 9, "PW": 5, "SW": 2, "MT": 1, "PROX": False, "REV": True, "MAP": False}
    assert a.values() == {"MTW": 1, "tpw": 4, "ngy": 2, "lds_over_96k": 1, "wgs": 96}
    assert b.template() == {} and b.values() == {"tiles": 64}
    mod = _tool()
    tests = {}
    recs = mod.parse_log(text, tests)
    assert len(recs) == 2 and list(tests.values()) == ["tests/test_x.py::test_y"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="the ladder is walked with launches that must fail: no-device machines only")
def test_first_rung_of_the_analysis_ladder_at_the_workgroup_minimum():
    """Without a device cdl_cu_count() falls back to 256, the value the shapes of tests/test_gpu_dispatch.py were
    chosen for, and the first launch of the chosen tier is recorded before it fails: 96 workgroups take the
    matrix-core analysis, 72 the tiled fp32 kernel -- and so do the 96 without a workspace ("workspace == NULL: VALU")."""
    lib = cva._lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    first = {}
    for N in (4, 3):
        gs = cva.ops.Geometry.make(N, 1, 16, (6, 30, 61), (3, 5, 5), (1, 2, 2), 1).c_struct()
        n = lib.cdl_analysis_workspace_floats(ctypes.byref(gs))
        with cva.ops.trace() as t:
            lib.cdl_analysis(ctypes.byref(gs), p, p, 1.0, None, None, None, p, p, n, None, None, None)
        first[N] = t[0].file
    assert first == {4: "cdl_analysis_mfma.hip", 3: "cdl_generic_tiled.hip"}
    gs = cva.ops.Geometry.make(4, 1, 16, (6, 30, 61), (3, 5, 5), (1, 2, 2), 1).c_struct()
    with cva.ops.trace() as t:
        lib.cdl_analysis(ctypes.byref(gs), p, p, 1.0, None, None, None, p, None, 0, None, None, None)
    assert t[0].file == "cdl_generic_tiled.hip"


# ------------------------------------------------------------------------------------------------- launch sites
def test_every_launch_site_is_followed_by_a_check_and_can_be_told_apart():
    """Each `kernel<<<...>>>` has a CDL_LAUNCH_CHECK behind it (that is where the record is made), and sites that
    share a check line are named by a CDL_TRACE_NOTE, or the tool could not tell which of them ran."""
    mod = _tool()
    sites = mod.scan_sources()
    assert len(sites) > 90
    assert not [s.id for s in sites if not s.checks]
    assert len({s.id for s in sites}) == len(sites)
    for (file, _), group in mod.index(sites).items():
        if len(group) > 1:
            src = open(os.path.join(mod.CSRC, file)).read()
            for s in group:
                assert re.search(r'CDL_TRACE_NOTE\("[^"]*\b' + s.kernel + r'\b', src), f"{s.id}: no note names the kernel"
    for path in sorted(os.listdir(mod.CSRC)):                   # no launch escapes the trace by checking the error itself
        if path.endswith(".hip"):
            assert "hipGetLastError" not in open(os.path.join(mod.CSRC, path)).read(), path


def test_manifest_accounts_for_every_launch_site():
    """tests/launch_coverage.json: launch site -> the test that reaches it, or a waiver with its reason.  A new kernel
    launch arrives with one of the two."""
    mod = _tool()
    man = json.load(open(MANIFEST))
    ids = [s.id for s in mod.scan_sources()]
    assert not [i for i in ids if i not in man], "launch sites missing from tests/launch_coverage.json"
    assert not [k for k in man if k not in ids], "stale entries in tests/launch_coverage.json"
    for site, entry in man.items():
        assert set(entry) in ({"test"}, {"waiver"}), (site, entry)
        if "waiver" in entry:
            assert len(entry["waiver"].strip()) >= 20, f"{site}: a waiver states its reason"
            continue
        path, _, name = entry["test"].partition("::")
        name = name.split("[")[0]
        assert os.path.exists(os.path.join(ROOT, path)), entry
        assert re.search(r"^def " + re.escape(name) + r"\(", open(os.path.join(ROOT, path)).read(), re.M), entry
