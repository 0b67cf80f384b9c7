"""cva.functional without a GPU: the surface, the argument checks that come before any device work,
and the argument checks of the new C entry points (the library loads without a device; an ill-formed call returns
CDL_EINVAL before any launch)."""
import ctypes

import pytest
import torch

import cdlnet_video_amd as cva
from cdlnet_video_amd import _lib, ops

F = cva.functional
NAMES = ["analysis", "synthesis", "shrink", "ST", "prox_csr", "prox_csr_f2", "analysis_shrink", "pre_process",
         "post_process"]


def test_surface():
    assert "functional" in cva.__all__
    for name in NAMES:
        assert callable(getattr(F, name)), name
    assert sorted(F.__all__) == sorted(NAMES)
    assert F.ST is F.shrink


def _code(*shape):
    return torch.randn(*shape)


@pytest.mark.parametrize("call", [
    lambda: F.analysis(torch.randn(2, 1, 8, 8), torch.randn(4, 1, 3, 3)),
    lambda: F.synthesis(_code(2, 4, 8, 8), torch.randn(4, 1, 3, 3)),
    lambda: F.shrink(_code(2, 4, 8, 8), 0.1),
    lambda: F.shrink(_code(2, 4, 8, 8), torch.rand(2, 1, 8, 8)),
    lambda: F.prox_csr(_code(2, 4, 8, 8), _code(2, 4, 8, 8), 0.1, torch.rand(4, 1, 1)),
    lambda: F.prox_csr_f2(_code(2, 4, 8, 8), _code(2, 4, 8, 8), _code(2, 4, 8, 8), 0.1, 0.5, 0.5),
    lambda: F.analysis_shrink(torch.randn(2, 1, 8, 8), torch.randn(4, 1, 3, 3), torch.rand(1, 4, 1, 1)),
    lambda: F.pre_process(torch.randn(2, 1, 7, 9), 2),
    lambda: F.post_process(torch.randn(2, 1, 8, 10), [torch.zeros(2, 1, 1, 1), (0, 1, 0, 1)]),
    lambda: cva.ST(_code(2, 4, 8, 8), 0.1),
    lambda: cva.prox_CSR(_code(2, 4, 8, 8), _code(2, 4, 8, 8), 0.1, 0.5),
])
def test_cpu_tensors_are_refused(call):
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        call()


@pytest.mark.parametrize("t", [torch.rand(3), torch.rand(2, 4, 8, 7), torch.rand(3, 1, 1, 1), torch.rand(1, 2, 4, 8, 8)])
def test_threshold_that_does_not_broadcast(t):
    u = _code(2, 4, 8, 8)
    with pytest.raises(ValueError, match="does not broadcast"):
        F.shrink(u, t)
    with pytest.raises(ValueError, match="does not broadcast"):
        F.prox_csr(u, u, t, 0.5)
    with pytest.raises(ValueError, match="does not broadcast"):
        F.prox_csr_f2(u, u, u, 0.1, 0.5, t)


def test_thresholds_on_another_device_or_in_a_list_are_converted_like_before():
    """torch.as_tensor(t, device=x.device), as ST / prox_CSR always did: only the code's device decides."""
    u = _code(2, 4, 8, 8)
    with pytest.raises(RuntimeError, match="`x` is on cpu"):
        cva.ST(u, [[[0.1]], [[0.2]], [[0.3]], [[0.4]]])
    with pytest.raises(ValueError, match="does not broadcast"):
        cva.prox_CSR(u, u, [0.1, 0.2, 0.3], 0.5)


def test_analysis_shrink_takes_row_thresholds_only():
    with pytest.raises(ValueError, match="spatial"):
        F.analysis_shrink(torch.randn(2, 1, 8, 8), torch.randn(4, 1, 3, 3), torch.rand(2, 1, 8, 8))


def test_mask_gradient_is_refused_before_any_device_work():
    mask = torch.ones(2, 1, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="mask"):
        F.synthesis(_code(2, 4, 8, 8), torch.randn(4, 1, 3, 3), mask=mask)
    with pytest.raises(NotImplementedError, match="mask"):
        F.pre_process(torch.randn(2, 1, 8, 8), 1, mask=mask)


def test_broadcast_strides():
    code = (3, 5, 4, 6)
    st = lambda shape: (lambda b: (b.n, b.m, b.p))(ops.bcast_strides(shape, code))
    assert st((3, 5, 1, 1)) == (5, 1, 0)          # the row form
    assert st((1, 5, 1, 1)) == (0, 1, 0)
    assert st((3, 1, 1, 1)) == (1, 0, 0)
    assert st((1, 1, 1, 1)) == (0, 0, 0)
    assert st((3, 1, 4, 6)) == (24, 0, 1)
    assert st((1, 1, 4, 6)) == (0, 0, 1)
    assert st((1, 5, 4, 6)) == (0, 24, 1)
    assert st((3, 5, 4, 6)) == (120, 24, 1)
    for bad in ((3, 5, 4, 1), (2, 5, 1, 1), (3, 5, 1), (3, 4, 1, 1)):
        with pytest.raises(ValueError):
            ops.bcast_strides(bad, code)


# ------------------------------------------------------------------------------------------ the C entry points
N, M, H, W = 2, 3, 4, 5
PER_M = H * W
GEOM = ops.Geometry.make(N, 1, M, (H, W), (1, 1), (0, 0), 1)
PTR = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before a launch
# ... and must never reach a launch: where a device is present a regressed argument check would start a kernel on PTR, so
# these run only where there is none (the library loads without a device)
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="argument checks on fake pointers: only without a device")
ROW = (M, 1, 0)
DENSE = (M * PER_M, PER_M, 1)
BAD_STRIDES = [(M, 1, 2), (M, 2, 0), (M + 1, 1, 0), (PER_M, PER_M, 1), (1, 1, 0), (M * PER_M, 1, 1), (-M, 1, 0)]


def _b(s):
    return ctypes.byref(_lib.Bcast(*s)) if s is not None else None


def _prox_b(u=PTR, zp=PTR, za=None, lam=PTR, sl=ROW, g1=PTR, s1=ROW, g2=None, s2=ROW, out=PTR, geom=GEOM):
    g = ctypes.byref(geom.c_struct()) if geom is not None else None
    return _lib.lib().cdl_prox_csr_b(g, u, zp, za, lam, _b(sl), g1, _b(s1), g2, _b(s2), out, None)


def _prox_b_bwd(gz=PTR, u=PTR, zp=PTR, za=None, lam=PTR, sl=ROW, g1=PTR, s1=ROW, g2=None, s2=ROW, gu=PTR, gzp=None, gza=None,
                dl=PTR, d1=PTR, d2=None, scratch=PTR, n=None, geom=GEOM):
    gs = geom.c_struct()
    if n is None:
        n = int(_lib.lib().cdl_prox_csr_scratch_floats(ctypes.byref(gs)))
    return _lib.lib().cdl_prox_csr_b_bwd(ctypes.byref(gs), gz, u, zp, za, lam, _b(sl), g1, _b(s1), g2, _b(s2), gu, gzp, gza,
                                         dl, d1, d2, scratch, n, None)


def _shrink_b(x=PTR, tau=PTR, st=ROW, out=PTR, n=N, m=M, per_m=PER_M):
    return _lib.lib().cdl_shrink_b(x, tau, _b(st), out, n, m, per_m, None)


def _shrink_b_bwd(gup=PTR, x=PTR, tau=PTR, st=ROW, gx=PTR, el=None, n=N, m=M, per_m=PER_M):
    return _lib.lib().cdl_shrink_b_bwd(gup, x, tau, _b(st), gx, el, n, m, per_m, None)


@no_device
def test_new_entry_points_refuse_null_pointers():
    E = _lib.CDL_EINVAL
    for name in ("u", "zp", "lam", "g1", "out", "sl", "s1", "geom"):
        assert _prox_b(**{name: None}) == E, name
    for name in ("gz", "u", "zp", "lam", "g1", "gu", "scratch", "sl", "s1"):
        assert _prox_b_bwd(**{name: None}) == E, name
    for name in ("x", "tau", "out", "st"):
        assert _shrink_b(**{name: None}) == E, name
    for name in ("gup", "x", "tau", "gx", "st"):
        assert _shrink_b_bwd(**{name: None}) == E, name
    assert _shrink_b(n=0) == E and _shrink_b(m=0) == E and _shrink_b(per_m=0) == E
    assert _prox_b_bwd(n=0) == E                                            # scratch too small


@no_device
def test_new_entry_points_refuse_f2_without_gamma2():
    E = _lib.CDL_EINVAL
    assert _prox_b(za=PTR, g2=None) == E
    assert _prox_b(za=PTR, g2=PTR, s2=None) == E
    assert _prox_b_bwd(za=PTR, g2=None) == E
    assert _prox_b_bwd(za=PTR, g2=PTR, s2=None) == E
    assert _prox_b_bwd(gza=PTR) == E and _prox_b_bwd(d2=PTR) == E       # a second neighbour's outputs without it


@no_device
@pytest.mark.parametrize("bad", BAD_STRIDES)
def test_new_entry_points_refuse_strides_that_are_neither_zero_nor_dense(bad):
    E = _lib.CDL_EINVAL
    assert _prox_b(sl=bad) == E and _prox_b(s1=bad) == E
    assert _prox_b(za=PTR, g2=PTR, s2=bad) == E
    assert _prox_b_bwd(sl=bad) == E and _prox_b_bwd(s1=bad) == E
    assert _prox_b_bwd(za=PTR, g2=PTR, d2=PTR, s2=bad) == E
    assert _shrink_b(st=bad) == E and _shrink_b_bwd(st=bad) == E


@no_device
def test_row_form_callers_keep_their_argument_checks():
    E = _lib.CDL_EINVAL
    gs = ctypes.byref(GEOM.c_struct())
    lib = _lib.lib()
    assert lib.cdl_prox_csr(gs, None, PTR, None, PTR, PTR, None, PTR, None) == E
    assert lib.cdl_prox_csr(gs, PTR, PTR, PTR, PTR, PTR, None, PTR, None) == E
    assert lib.cdl_prox_csr(None, PTR, PTR, None, PTR, PTR, None, PTR, None) == E
    assert lib.cdl_shrink(None, PTR, PTR, 6, PER_M, None) == E
