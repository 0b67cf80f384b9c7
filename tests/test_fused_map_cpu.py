"""Noise-level maps on the fused 2-D tier, without a GPU: the C ABI and its ctypes mirror, the
keyword-only arguments of `ops`, the opt-in knob, `loop._route` as a table, the kernel names the host registers, and the
launch record of a map stage."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cdlnet_video_amd as cva
from cdlnet_video_amd import _lib, loop, ops
from conftest import ROOT

# entry point -> (arguments before the stream in the parent, what it gained in front of the stream)
GAINED = {
    "cdl_fused2d_iter_fwd": (10, ("cmap", "tslope")),
    "cdl_fused2d_forward": (14, ("cmap", "tslope")),
    "cdl_fused2d_stage_bwd": (14, ("cmap", "tslope", "dcmap", "dcmap_add")),
    "cdl_fused2d_dtau_reduce": (6, ("dtau_partial_w",)),
    "cdl_fused2d_backward": (25, ("cmap", "tslope", "dcmap")),
}
UNCHANGED = {"cdl_fused2d_tangent": 16, "cdl_fusedg_iter_fwd": 11, "cdl_fusedg_stage_bwd": 11, "cdl_fusedg_dtau_reduce": 7,
             "cdl_fusedg_forward": 15, "cdl_fusedg_backward": 27, "cdl_fusedg_tangent": 16}


def _decl(header, name):
    return re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)).split(",")


def test_entry_points_gained_nullable_arguments_in_front_of_the_stream():
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    for name, (before, gained) in GAINED.items():
        sig, decl = _lib.SIGNATURES[name], _decl(header, name)
        assert len(sig) == before + len(gained) + 1 == len(decl), name
        assert sig[-1] is ctypes.c_void_p and re.search(r"\*stream\b", decl[-1]), name
        for arg, ctype, text in zip(gained, sig[before:-1], decl[before:-1]):
            if arg == "dcmap_add":                               # the accumulate flag of dcmap
                assert ctype is ctypes.c_int and re.search(r"\bint dcmap_add\b", text), name
            else:
                assert ctype is ctypes.c_void_p and re.search(rf"\*{arg}\b", text), (name, arg, text)
    for name, argc in UNCHANGED.items():
        assert len(_lib.SIGNATURES[name]) == argc == len(_decl(header, name)), name
    for base in list(GAINED) + list(UNCHANGED):
        for suffix in ("_map", "_cmap", "_smap", "_sigma"):
            sibling = base + suffix
            assert sibling not in _lib.SIGNATURES and sibling not in _lib.SIZE_T_FUNCS, sibling
            assert not re.search(rf"\b{sibling}\b", header), sibling


def test_the_partial_buffer_of_a_map_stage_is_sized_by_the_library():
    """With a map the reverse stage writes a second (tiles, M) array behind the first: the size comes from the library."""
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    assert re.search(r"\bsize_t cdl_fused2d_dtau_partial_floats\(const cdl_geom \*g, int with_map\);", header)
    assert _lib.SIZE_T_FUNCS["cdl_fused2d_dtau_partial_floats"] == [_lib._G, ctypes.c_int]
    lib = _lib.lib()
    g = ops.Geometry.make(3, 1, 64, (33, 130), (7, 7), (3, 3), 1)
    tiles = ops.fused_tiles(g)
    assert tiles == 3 * 3 * 3
    assert lib.cdl_fused2d_dtau_partial_floats(g._c_ref(), 0) == tiles * 64
    assert lib.cdl_fused2d_dtau_partial_floats(g._c_ref(), 1) == 2 * tiles * 64
    assert ops._dtau_partial_floats(ops._FUSED2D, g, True) == 2 * tiles * 64
    bad = ops.Geometry.make(3, 1, 48, (33, 130), (7, 7), (3, 3), 1)                  # not a geometry of the tier
    assert lib.cdl_fused2d_dtau_partial_floats(bad._c_ref(), 1) == 0


def test_ops_gain_keyword_only_arguments_that_default_to_none():
    for fn, kws in ((ops.fused_iter, ("cmap", "tslope")), (ops.fused_forward, ("cmap", "tslope")),
                    (ops.fused_stage_bwd, ("cmap", "tslope", "dcmap")), (ops.fused_backward, ("cmap", "tslope", "dcmap")),
                    (ops.fused_dtau_reduce, ("weighted",))):
        params = inspect.signature(fn).parameters
        for kw in kws:
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None, (fn.__name__, kw)
    for fn in (ops.fusedg_iter, ops.fusedg_forward, ops.fusedg_stage_bwd, ops.fusedg_backward):     # the other tier: untouched
        assert not {"cmap", "tslope", "dcmap"} & set(inspect.signature(fn).parameters), fn.__name__


def test_the_knob_defaults_to_generic_and_its_scope_restores():
    assert loop.MAP_TIER == "generic"
    for bad in ("auto", "fusedg", "", None):
        with pytest.raises(ValueError):
            loop.set_map_tier(bad)
        with pytest.raises(ValueError):
            loop.map_tier_scope(bad)
    assert loop.MAP_TIER == "generic"
    with loop.map_tier_scope("fused"):
        assert loop.MAP_TIER == "fused"
        with loop.map_tier_scope("generic"):
            assert loop.MAP_TIER == "generic"
        assert loop.MAP_TIER == "fused"
    assert loop.MAP_TIER == "generic"
    with pytest.raises(RuntimeError):
        with loop.map_tier_scope("fused"):
            raise RuntimeError("inside")
    assert loop.MAP_TIER == "generic"
    loop.set_map_tier("fused")
    try:
        assert loop.MAP_TIER == "fused"
    finally:
        loop.set_map_tier("generic")


@pytest.fixture
def geometries(monkeypatch):
    """Two stand-in geometries: one the 2-D tier takes, one only the tile / strip kernels take."""
    monkeypatch.setattr(ops, "fused_supported", lambda g: g == "flagship")
    monkeypatch.setattr(ops, "fusedg_supported", lambda g: g in ("flagship", "fusedg-only"))
    saved = (loop.BACKEND, loop.PRECISION, loop.CODE_LAYOUT, loop.MAP_TIER)
    yield "flagship", "fusedg-only"
    loop.BACKEND, loop.PRECISION, loop.CODE_LAYOUT, loop.MAP_TIER = saved


def test_route_table(geometries):
    flag, other = geometries
    plain = lambda: (loop._route(flag, False, False), loop._route(other, False, False), loop._route("neither", False, False))
    today = ("fused", "fusedg", "generic")
    assert loop._route(flag, False, True) == "generic" and plain() == today          # map + default
    loop.set_map_tier("fused")
    assert loop._route(flag, False, True) == "fused" and plain() == today             # map + knob
    for layout in ("nchw", "blocked"):
        loop.set_code_layout(layout)
        assert loop._route(flag, False, True) == "fused"
    assert loop._route(other, False, True) == "generic"                               # a fusedg-only geometry
    assert loop._route("neither", False, True) == "generic"
    assert loop._route(flag, True, True) == "generic"                                 # fp32: `exact`
    assert loop._route(flag, True, False) == "generic"
    loop.set_backend("generic")
    assert loop._route(flag, False, True) == "generic" and plain() == ("generic",) * 3
    loop.set_backend("auto")
    for prec in ("split4", "bf16", "fp32"):
        with loop.precision_scope(prec):
            assert loop._route(flag, prec == "fp32", True) == "generic", prec
            assert plain() == today                                                   # (exact is the caller's flag)
    loop.set_code_layout("blocked_bf16")
    assert loop._route(flag, False, True) == "generic" and plain() == today
    loop.set_code_layout("blocked")
    assert loop._route(flag, False, True) == "fused"


def test_tier_table_passes_the_map_to_the_fused_2d_sweeps_only(monkeypatch):
    seen = {}
    monkeypatch.setattr(loop, "_forward_fused", lambda *a, **k: seen.setdefault("fwd", k))
    monkeypatch.setattr(loop, "_backward_fused", lambda *a, **k: seen.setdefault("bwd", k))
    st = type("St", (), dict(layout="blocked", precision="split3"))()
    loop._TIERS["fused"].forward(st, *range(8), False, cmap="c", tslope="s")
    loop._TIERS["fused"].reverse(st, *range(13), cmap="c", tslope="s", dcmap="d")
    assert seen["fwd"]["cmap"] == "c" and seen["fwd"]["tslope"] == "s"
    assert (seen["bwd"]["cmap"], seen["bwd"]["tslope"], seen["bwd"]["dcmap"]) == ("c", "s", "d")
    with pytest.raises(TypeError):
        loop._TIERS["fusedg"].forward(st, *range(8), False, cmap="c", tslope="s")


def test_stage_kernels_carry_one_name_on_host_and_device():
    """The stage kernel's parameter type depends on its mode, so the mode's constant is part of every mangled name: it must
    be spelled the same by the host pass (which registers the name) and the device pass (which defines it) -- an unnamed
    type in it is numbered per pass, and the launch then finds no kernel."""
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(re.findall(rb"_ZN12_GLOBAL__N_17k_stageI[A-Za-z0-9_$]*", blob))
    assert names and not [n for n in names if b"$" in n]
    modes = {int(m) for m in re.findall(rb"_ZN12_GLOBAL__N_17k_stageILi\dELi0ELi(\d)E", b"\n".join(names))}
    assert modes == {0, 1, 2, 4, 5, 6}                              # split3: the three modes and their map forms
    assert not re.search(rb"17k_stageILi\dELi[12]ELi[456]E", blob)  # no map form in another arithmetic


@pytest.mark.skipif(torch.cuda.is_available(), reason="the launch must fail for want of a device")
def test_a_map_stage_reaches_its_kernel_without_a_device():
    """cdl_fused2d_iter_fwd with and without a map, no device.  The stage launcher raises its kernel's dynamic-LDS limit
    before it launches, and that call is the first to fail without a device: no launch record is made on this path (unlike
    the analysis ladder of test_launch_trace_cpu.py), so what shows here is that a map in split3 gets as far as its
    kernel -- a HIP error, not a refusal -- while every other combination is refused first.  The mode in the launch
    record's template text (MODE = 4 / 5 / 6) is asserted on the device, tests/test_gpu_fused_map.py."""
    lib = cva._lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    gs = ops.Geometry.make(1, 1, 32, (16, 64), (7, 7), (3, 3), 1).c_struct()
    zout = ctypes.c_void_p(p.value + 1024)
    for zin, cmap in ((None, None), (None, p), (p, None), (p, p)):
        for layouts in (0, 1 << 5 | 1 << 7):                       # NCHW, blocked
            rc = lib.cdl_fused2d_iter_fwd(ctypes.byref(gs), p, zin, p, p, 1.0, zout, p, None, layouts, cmap, cmap, None)
            assert rc < 0 and rc not in (_lib.CDL_EINVAL, _lib.CDL_EUNSUPPORTED), (zin, cmap, layouts, rc)
    # a map without its slopes, or in an arithmetic or layout that has no map form: refused before any launch
    with ops.trace() as t:
        assert lib.cdl_fused2d_iter_fwd(ctypes.byref(gs), p, p, p, p, 1.0, zout, p, None, 2 << 5 | 2 << 7, p, p, None) == _lib.CDL_EUNSUPPORTED
        assert lib.cdl_fused2d_iter_fwd(ctypes.byref(gs), p, None, p, p, 1.0, zout, p, None, 1, p, p, None) == _lib.CDL_EUNSUPPORTED
        assert lib.cdl_fused2d_iter_fwd(ctypes.byref(gs), p, None, p, p, 1.0, zout, p, None, 0, p, None, None) == _lib.CDL_EINVAL
        assert lib.cdl_fused2d_iter_fwd(ctypes.byref(gs), p, None, p, p, 1.0, zout, p, None, 2, p, p, None) == _lib.CDL_EUNSUPPORTED
        assert lib.cdl_fused2d_dtau_reduce(ctypes.byref(gs), p, p, p, p, None, p, None) == _lib.CDL_EINVAL
    assert len(t) == 0
