"""Per-frame noise levels on the fused generic tier, the parts that need no device: the knob and the
route table, the classification of sigma, what the shared sweep wrapper hands to the tiers, the C surface (a flag bit, no
changed signature), awgn3d(per_frame=True), the window crop, and -- on the oracle -- that the levels of the device tests are
told apart: a kernel reading another row of the threshold table would move xhat by far more than the tolerance."""
import ctypes
import os
import re
import types

import pytest
import torch

import cdlnet_video_amd as cva
from cdlnet_video_amd import _lib, loop, net as netmod, ops
from conftest import ROOT, rel_err
from frame_levels_util import CASES, build, levels, misread
from oracle import cdl_oracle as O

XTOL = 1e-5          # tests/test_gpu_sigmamap.py


@pytest.fixture
def knobs():
    saved = (loop.BACKEND, loop.PRECISION, loop.CODE_LAYOUT, loop.MAP_TIER, loop.FRAME_TIER)
    yield
    loop.BACKEND, loop.PRECISION, loop.CODE_LAYOUT, loop.MAP_TIER, loop.FRAME_TIER = saved


# ------------------------------------------------------------------------------------------ the knob
def test_knob_and_scope(knobs):
    assert loop.FRAME_TIER == "generic"
    with pytest.raises(ValueError):
        loop.set_frame_tier("fusedg")
    with pytest.raises(ValueError):
        loop.frame_tier_scope("strip")
    with loop.frame_tier_scope("fused"):
        assert loop.FRAME_TIER == "fused" and loop.MAP_TIER == "generic"          # a knob of its own
        with loop.frame_tier_scope("generic"):
            assert loop.FRAME_TIER == "generic"
        assert loop.FRAME_TIER == "fused"
    assert loop.FRAME_TIER == "generic"
    with pytest.raises(RuntimeError):
        with loop.frame_tier_scope("fused"):
            raise RuntimeError("inside")
    assert loop.FRAME_TIER == "generic"
    loop.set_frame_tier("fused")
    assert loop.FRAME_TIER == "fused"
    loop.set_map_tier("fused")
    assert loop.FRAME_TIER == "fused" and loop.MAP_TIER == "fused"
    loop.set_frame_tier("generic")
    assert loop.MAP_TIER == "fused"


# ------------------------------------------------------------------------------------------ the route
def _geoms(monkeypatch):
    """Stand-in geometries: a clip the tile kernel takes, a clip no fused plan takes, a 2-D flagship frame, and a one-frame
    geometry of the fused generic tier (D == 1: the strip kernel's ground, and JDD's)."""
    g = lambda name, D: types.SimpleNamespace(name=name, dims=(D, 32, 64))
    clip, odd, flag, flat = g("clip", 4), g("odd", 4), g("flagship", 1), g("flat", 1)
    monkeypatch.setattr(ops, "fused_supported", lambda q: q is flag)
    monkeypatch.setattr(ops, "fusedg_supported", lambda q: q in (clip, flag, flat))
    return clip, odd, flag, flat


def test_route_table(monkeypatch, knobs):
    clip, odd, flag, flat = _geoms(monkeypatch)
    every = (clip, odd, flag, flat)
    plain = lambda: tuple(loop._route(q, False, False) for q in every)
    as_map = lambda: tuple(loop._route(q, False, True) for q in every)
    frames = lambda exact=False: tuple(loop._route(q, exact, True, frames=True) for q in every)
    today_plain = ("fusedg", "generic", "fused", "fusedg")
    generic = ("generic",) * 4
    # without the knob: today's table, whatever the new keyword says
    assert plain() == today_plain and as_map() == generic and frames() == generic
    loop.set_map_tier("fused")                                   # the rows tests/test_fused_map_cpu.py pins
    assert as_map() == ("generic", "generic", "fused", "generic") and plain() == today_plain
    assert frames() == ("generic", "generic", "fused", "generic")        # frame levels are a map to that knob
    loop.set_map_tier("generic")
    # with the knob: a clip the tile / grouped strip kernels take, and nothing else
    loop.set_frame_tier("fused")
    assert frames() == ("fusedg", "generic", "generic", "generic")
    assert plain() == today_plain and as_map() == generic                # three-argument calls answer as before
    assert frames(exact=True) == generic                                 # the fp32 arithmetic
    assert loop._route(clip, False, False, frames=True) == "fusedg"      # (not a map: the keyword is not read)
    loop.set_backend("generic")
    assert frames() == generic and plain() == generic
    loop.set_backend("auto")
    for prec in ("split4", "bf16"):                                      # `exact` is the caller's flag; the tier has one arithmetic
        with loop.precision_scope(prec):
            assert frames() == ("fusedg", "generic", "generic", "generic")
    loop.set_map_tier("fused")                                           # both knobs: each keeps its own ground
    assert frames() == ("fusedg", "generic", "fused", "generic")
    assert as_map() == ("generic", "generic", "fused", "generic")


# ------------------------------------------------------------------------------------------ the frame form of sigma
N, D, H, W = 3, 5, 12, 20
GRID = (D, H, W)


def _scale(sigma, n=N, grid=GRID):
    return netmod._noise_scale(sigma, True, n, torch.device("cpu"), grid)


FRAME_FORMS = [(N, 1, D, 1, 1), (1, 1, D, 1, 1), (D, 1, 1)]


@pytest.mark.parametrize("shape", FRAME_FORMS)
def test_frame_forms_are_classified(shape, knobs):
    sigma = 255.0 * (0.05 + torch.rand(shape))
    dense = _scale(sigma)                                        # the knob off: the dense expansion, as today
    assert tuple(dense.shape) == (N, 1) + GRID and dense.is_contiguous()
    want = (sigma / 255.0).reshape((1,) * (5 - len(shape)) + shape).expand(N, 1, D, H, W)
    assert torch.equal(dense, want)
    loop.set_frame_tier("fused")
    c = _scale(sigma)
    assert tuple(c.shape) == (N, 1, D, 1, 1) and c.is_contiguous()
    assert torch.equal(c.expand(N, 1, D, H, W), dense)           # the same levels, bit for bit
    g = types.SimpleNamespace(N=N, ndim=3, code_spatial=GRID)
    assert loop._frame_levels(g, c) and not loop._frame_levels(g, dense)
    assert torch.equal(loop._dense_levels(g, c), dense)


def test_everything_else_is_classified_as_before(knobs):
    forms = [25.0, torch.tensor(25.0), torch.rand(N), torch.rand(N, 1, 1, 1, 1), torch.rand(N, 1, D, H, W),
             torch.rand(1, 1, D, H, 1), torch.rand(N, 1, 1, H, W), torch.rand(1, 1, 1, 1, W)]
    before = [_scale(s) for s in forms]
    before_2d = [_scale(s, grid=(H, W)) for s in (torch.rand(N, 1, H, 1), torch.rand(1, 1, 1, W))]
    torch.manual_seed(0)
    amb = torch.rand(1, 1, N, 1, 1)                              # D == N: the per-sample rule wins, knob or not
    amb_before = _scale(amb, grid=(N, H, W))
    loop.set_frame_tier("fused")
    for s, ref in zip(forms, before):
        got = _scale(s)
        assert got.shape == ref.shape and torch.equal(got, ref)
    assert all(b.shape == (N, 1, H, W) for b in before_2d)       # a 2-D net has no frames: rows / columns stay dense maps
    assert tuple(amb_before.shape) == (N,) and torch.equal(_scale(amb, grid=(N, H, W)), amb_before)
    assert _scale(torch.rand(N, 1, D, 1, 1), grid=(D, 1, 1)).shape == (N, 1, D, 1, 1)      # a 1 x 1 plane: dense IS that shape
    assert not loop._frame_levels(types.SimpleNamespace(N=N, ndim=3, code_spatial=(D, 1, 1)), torch.rand(N, 1, D, 1, 1))
    assert _scale(None) is None and netmod._noise_scale(torch.rand(N, 1, D, 1, 1), False, N, torch.device("cpu"), GRID) is None


def test_gradient_of_sigma_keeps_its_shape(knobs):
    loop.set_frame_tier("fused")
    for shape in FRAME_FORMS:
        sigma = torch.rand(shape, requires_grad=True)
        _scale(sigma).sum().backward()
        assert sigma.grad.shape == sigma.shape


# ------------------------------------------------------------------------------------------ the shared sweep wrapper
K, M = 2, 8


@pytest.fixture
def sweep_spies(monkeypatch):
    calls = []

    def spy(name, result):
        def run(*args, **kw):
            calls.append((name, args, kw))
            return result
        return run

    z = torch.zeros(1)
    monkeypatch.setattr(ops, "thresholds", lambda t, c, n: calls.append(("thresholds", (t, c, n), {})) or torch.zeros(K, n, M))
    for name in ("_forward_generic", "_forward_fused", "_forward_fusedg"):
        monkeypatch.setattr(loop, name, spy(name, (z, z, [z], [], ["maps"])))
    for name in ("_backward_generic", "_backward_fused", "_backward_fusedg"):
        monkeypatch.setattr(loop, name, spy(name, ([z] * K, [z] * K)))
    return calls


@pytest.mark.parametrize("takes", [True, False])
def test_forward_and_reverse_sweep_carry_frame_levels(monkeypatch, sweep_spies, knobs, takes):
    g = ops.Geometry.make(N, 1, M, GRID, (3, 3, 3), (1, 1, 1), 1)
    monkeypatch.setattr(ops, "fused_supported", lambda q: False)
    monkeypatch.setattr(ops, "fusedg_supported", lambda q: takes)
    monkeypatch.setattr(ops, "fusedg_code_layout", lambda q, training=True: "nchw")
    loop.set_frame_tier("fused")
    t = torch.rand(K, 2, M, 1, 1, 1)
    c = torch.rand(N, 1, D, 1, 1)
    w = [torch.zeros(g.filter_shape())] * K
    st = types.SimpleNamespace(exact=False, K=K, geom=g)
    loop._forward_sweep(st, g, torch.zeros(g.image_shape()), None, c, t, w, w, True, False)
    (_, (_, c_thr, n_thr), _), (name, args, kw) = sweep_spies
    sv = types.SimpleNamespace(yp=torch.zeros(g.image_shape()), mask_p=None, c=c, t=t, A=w, B=w, codes=[], resid=[], maps=[])
    del sweep_spies[:]
    dt = torch.zeros(K, 2, M)
    out = loop._reverse_sweep(st, sv, torch.zeros(g.image_shape()), None, dt, want_c=True)
    (bname, bargs, bkw), = sweep_spies
    if takes:
        assert (st.tier, st.frames, st.is_map) == ("fusedg", True, False)
        assert name == "_forward_fusedg" and kw["planes"] is True and "cmap" not in kw
        assert n_thr == N * D and torch.equal(c_thr, c.reshape(-1))              # cdl_thresholds with N * D levels
        assert bname == "_backward_fusedg" and bkw["planes"] is True
        assert torch.equal(bargs[4], c.reshape(-1)) and tuple(bkw["dtau"].shape) == (K, N * D, M)
        assert out[4] is None and out[3] is bkw["dtau"]
    else:                                                                        # the dense map, exactly as without the knob
        assert (st.tier, st.frames, st.is_map) == ("generic", False, True)
        assert name == "_forward_generic" and torch.equal(kw["cmap"], c.expand(N, 1, D, H, W)) and kw["cmap"].is_contiguous()
        assert c_thr is None and n_thr == N
        assert bname == "_backward_generic" and torch.equal(bkw["cmap"], kw["cmap"]) and bkw["dtau"] is None
        assert tuple(bkw["dcmap"].shape) == (N, 1, D, H, W)
        assert tuple(out[4].shape) == tuple(c.shape)                             # dL/dc in the shape c came in


def test_per_sample_and_dense_sweeps_get_todays_arguments(monkeypatch, sweep_spies, knobs):
    g = ops.Geometry.make(N, 1, M, GRID, (3, 3, 3), (1, 1, 1), 1)
    monkeypatch.setattr(ops, "fused_supported", lambda q: False)
    monkeypatch.setattr(ops, "fusedg_supported", lambda q: True)
    monkeypatch.setattr(ops, "fusedg_code_layout", lambda q, training=True: "nchw")
    t = torch.rand(K, 2, M, 1, 1, 1)
    w = [torch.zeros(g.filter_shape())] * K
    for knob in ("generic", "fused"):
        loop.set_frame_tier(knob)
        for c, tier in ((torch.rand(N), "fusedg"), (torch.rand(N, 1, D, H, W), "generic")):
            del sweep_spies[:]
            st = types.SimpleNamespace(exact=False)
            loop._forward_sweep(st, g, torch.zeros(g.image_shape()), None, c, t, w, w, False, False)
            (_, (_, c_thr, n_thr), _), (name, args, kw) = sweep_spies
            assert st.tier == tier and not st.frames and name == "_forward_" + tier and "planes" not in kw
            assert n_thr == N and (c_thr is c if c.dim() == 1 else c_thr is None)


def test_fusedg_tier_still_takes_no_map():
    st = types.SimpleNamespace(layout="nchw", frames=True)
    with pytest.raises(TypeError):
        loop._TIERS["fusedg"].forward(st, *range(8), False, cmap="c", tslope="s")
    with pytest.raises(TypeError):
        loop._TIERS["fusedg"].reverse(st, *range(13), cmap="c", tslope="s", dcmap="d")


# ------------------------------------------------------------------------------------------ the C surface
PARENT_SIGNATURES = {           # the cdl_fusedg_* rows of _lib.SIGNATURES before the flag: none may change
    "cdl_fusedg_tangent": "GI" + "P" * 12 + "IP",
    "cdl_fusedg_prep": "GPPPP",
    "cdl_fusedg_iter_fwd": "GPPPPFPPPIP",
    "cdl_fusedg_stage_bwd": "GPPPPPPPIIP",
    "cdl_fusedg_assemble": "GPPPFPPIP",
    "cdl_fusedg_dtau_reduce": "GPPPPPP",
    "cdl_fusedg_forward": "GI" + "P" * 11 + "IP",
    "cdl_fusedg_backward": "GI" + "P" * 20 + "ZIPPP",
}


def test_header_and_ctypes_table_carry_the_flag_and_no_changed_signature():
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    m = re.search(r"#define\s+CDL_TAU_PER_PLANE\s+(\d+)", header)
    assert m and int(m.group(1)) == ops.TAU_PER_PLANE == 512
    taken = ops.TILES_REVERSED | 15 | (3 << 5) | (3 << 7)        # arithmetic, tile order, CDL_LAYOUT_IN, CDL_LAYOUT_OUT
    assert ops.TAU_PER_PLANE & taken == 0
    letter = {_lib._G: "G", _lib._I: "I", _lib._P: "P", _lib._F: "F", ctypes.c_size_t: "Z"}
    for name, sig in PARENT_SIGNATURES.items():
        assert "".join(letter[a] for a in _lib.SIGNATURES[name]) == sig, name
    assert _lib.SIGNATURES["cdl_fusedg_dtau_reduce_planes"] == _lib.SIGNATURES["cdl_fusedg_dtau_reduce"]
    # the header declares the parent's parameter lists, and the sibling with the same one
    decl = lambda name: re.sub(r"/\*.*?\*/|\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1))
    assert decl("cdl_fusedg_iter_fwd").count(",") == 10 and decl("cdl_fusedg_forward").count(",") == 14
    assert decl("cdl_fusedg_backward").count(",") == 26 and decl("cdl_fusedg_dtau_reduce").count(",") == 6
    assert decl("cdl_fusedg_dtau_reduce_planes").count(",") == 6
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.cdl_fusedg_dtau_reduce_planes and lib.cdl_fusedg_dtau_reduce


# ------------------------------------------------------------------------------------------ awgn3d
def test_awgn3d_per_frame():
    x = torch.rand(3, 2, 4, 6, 5)
    gen = lambda: torch.Generator().manual_seed(9)
    y0, s0 = cva.utils.awgn3d(x, (10, 40), gen())
    y1, s1 = cva.utils.awgn3d(x, (10, 40), gen(), per_frame=False)
    assert tuple(s0.shape) == (3, 1, 1, 1, 1) and torch.equal(s0, s1) and torch.equal(y0, y1)
    g = gen()                                                    # the default's draws: rand (N,1,1,1,1), then randn
    sref = 10 + 30 * torch.rand((3, 1, 1, 1, 1), generator=g)
    assert torch.equal(s0, sref) and torch.equal(y0, x + torch.randn(x.shape, generator=g) * (sref / 255))
    yf, sf = cva.utils.awgn3d(x, (10, 40), gen(), per_frame=True)
    assert tuple(sf.shape) == (3, 1, 4, 1, 1) and float(sf.min()) >= 10 and float(sf.max()) <= 40
    assert sf.unique().numel() == 12
    g = gen()
    sref = 10 + 30 * torch.rand((3, 1, 4, 1, 1), generator=g)
    assert torch.equal(sf, sref) and torch.equal(yf, x + torch.randn(x.shape, generator=g) * (sref / 255))
    yc, sc = cva.utils.awgn3d(x, 25, gen(), per_frame=True)      # a fixed level is used as it is
    assert sc == 25
    with pytest.raises(ValueError):
        cva.utils.awgn3d(x[:, :, 0], (10, 40), gen(), per_frame=True)


# ------------------------------------------------------------------------------------------ windows
def test_window_crop_keeps_extent_one_axes():
    plan = cva.windowed.plan_windows((8, 12, 20), 1, (4, 12, 20), (1, 0, 0))
    assert len(plan.windows) == 2
    c = torch.arange(2 * 8, dtype=torch.float32).reshape(2, 1, 8, 1, 1)
    dense = c.expand(2, 1, 8, 12, 20).contiguous()
    pairs = [(w, n) for w in range(2) for n in range(2)]
    got, ref = plan.gather(c, pairs), plan.gather(dense, pairs)
    assert tuple(got.shape) == (4, 1, plan.shape[0], 1, 1) and tuple(ref.shape) == (4, 1) + tuple(plan.shape)
    assert torch.equal(got.expand_as(ref), ref)                  # cropped along depth with its window, nowhere else


# ------------------------------------------------------------------------------------------ the levels of the device tests
@pytest.mark.parametrize("label", sorted(CASES))
def test_levels_are_distinct_and_a_misread_row_shows(label):
    """On the oracle: applying the levels of row n, row zd or row d * N + n of the (N*D, M) table instead of row
    n * D + zd moves xhat by more than 100 x XTOL, so the device tests cannot pass with a wrong row index."""
    net, sd, x, y, mask, w, lev = build(label)
    cfg = CASES[label]
    Nn, Dd = cfg["shape"][0], cfg["shape"][2]
    assert lev.unique().numel() == Nn * Dd and torch.equal(lev, levels(Nn, Dd, 74))
    run = lambda sigma: O.ista(sd, y, K=cfg["K"], P=tuple(cfg["P"]), s=1, sigma=sigma, adaptive=True, mask=mask, ndim=3)[0]
    with torch.no_grad():
        right = run(lev)
        assert torch.equal(run(lev.expand((Nn, 1) + tuple(cfg["shape"][2:])).contiguous()), right)
        for which, wrong in misread(lev).items():
            if torch.equal(wrong, lev):
                assert Nn == 1 and which != "row n", (label, which)       # N = 1: rows zd and d * N + n ARE the right rows
                continue
            err = rel_err(run(wrong), right)
            assert err > 100 * XTOL, (label, which, err)
