"""Tensor-level wrappers over the C ABI (include/cdlnet_hip.h).

PyTorch supplies device memory and the stream; every operation here is a call into
libcdlnet_hip.so.  Inputs must be CUDA (ROCm) fp32 tensors -- there is no CPU path.
"""
import collections
import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib


def _stream():
    """Stream of the CURRENT device: every public function of this module runs under `_on_tensor_device`,
    which makes the tensors' device current first, so this is the tensors' stream."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _first_cuda_tensor(args, kwargs=None):
    """First CUDA tensor among the arguments, searching nested lists / tuples to any depth (gabor_filter_banks takes
    a list of 4-tuples of tensors)."""
    for a in list(args) + (list(kwargs.values()) if kwargs else []):
        if torch.is_tensor(a):
            if a.is_cuda:
                return a
        elif isinstance(a, (list, tuple)):
            t = _first_cuda_tensor(a)
            if t is not None:
                return t
    return None


def _on_tensor_device(fn):
    """Run `fn` with its first CUDA tensor argument's device current (net.to('cuda:1') without a
    torch.cuda.set_device(1) must not hand cuda:1 pointers to a stream of cuda:0).  `_dev` then rejects
    any further tensor that lives elsewhere."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = _first_cuda_tensor(args, kwargs)
        if t is None or t.device.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return wrapper


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: cdlnet-video_amd computes only through its HIP kernels "
            "(libcdlnet_hip.so) on a ROCm device; move the module and inputs to 'cuda'.")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"{name} is on {t.device} but this call runs on cuda:{torch.cuda.current_device()}: "
                           "all tensors of one call must live on one device")
    return t.contiguous()


def _opt(t, name):
    return None if t is None else _dev(t, name)


def _buf(t, name, shape=None, dtype=torch.float32):
    """The non-copying sibling of `_dev` for outputs and work buffers the caller provides (None stays None): a kernel
    writes through this very tensor, so a non-contiguous one is an error, never a `.contiguous()` copy."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: a buffer the HIP kernels write must live on the ROCm device")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor (strides {t.stride()})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


_KINDS = {}
_PTR, _GEOM, _BCAST, _INT, _FLOAT, _ASIS = range(6)


def _kinds(name):
    """How `_call` converts each argument of an entry point, from its declared types (the stream, last, left out):
    worked out once per entry point."""
    kind = {_lib._P: _PTR, _lib._G: _GEOM, _lib._B: _BCAST, _lib._I: _INT, ctypes.c_size_t: _INT, _lib._F: _FLOAT}
    sig = _lib.SIGNATURES[name]
    assert sig and sig[-1] is _lib._P, f"{name} takes no stream"
    _KINDS[name] = tuple(kind.get(t, _ASIS) for t in sig[:-1])
    return _KINDS[name]


def _check_pointer(t, cur, name, i):
    """A tensor that is about to become a pointer in a kernel must be contiguous and on the current ROCm device (`cur`;
    below -1: not asked for yet -- get_device() is -1 off the device, so a CPU tensor is refused without touching one).
    Returns the current device."""
    dev = t.get_device()
    if dev < 0:
        raise RuntimeError(f"{name}: argument {i} is on {t.device}, not on the ROCm device")
    if dev != cur:
        cur = torch.cuda.current_device()
        if dev != cur:
            raise RuntimeError(f"{name}: argument {i} is on {t.device} but this call runs on cuda:{cur}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: argument {i} is not contiguous")
    return cur


def _call(name, *args):
    """The one way into a stream-taking entry point: `args` are the C arguments before the stream, converted by their
    declared type in _lib.SIGNATURES -- Geometry / _lib.Bcast by reference, a tensor as its data pointer, None as NULL, a
    list or tuple of tensors as a pointer table (an empty one: NULL; a None entry: NULL), Python numbers as int / float;
    anything else (an int or float array) passes as it is.  Every tensor that becomes a pointer must be a contiguous CUDA
    tensor of the current device: RuntimeError / ValueError here, before the library is entered, instead of a host or
    foreign pointer in a kernel.  Appends the current stream and raises on the return code."""
    kinds = _KINDS.get(name) or _kinds(name)
    if len(args) != len(kinds):
        raise TypeError(f"{name}: takes {len(kinds)} arguments before the stream, got {len(args)}")
    cur = -2                                        # the current device: not asked for yet
    cargs = list(args)                              # also what keeps the pointer tables alive for the call
    for i, kind in enumerate(kinds):
        a = cargs[i]
        if kind == _PTR:
            if a is None:
                continue
            if isinstance(a, torch.Tensor):
                if a.get_device() != cur or not a.is_contiguous():      # the first tensor of a call, or a bad one
                    cur = _check_pointer(a, cur, name, i)
                cargs[i] = a.data_ptr()
            elif isinstance(a, (list, tuple)):
                for t in a:
                    if t is not None:
                        cur = _check_pointer(t, cur, name, i)
                cargs[i] = (ctypes.c_void_p * len(a))(*[None if t is None else t.data_ptr() for t in a]) if a else None
        elif kind == _GEOM:
            cargs[i] = a._c_ref()
        elif kind == _INT:
            cargs[i] = int(a)
        elif kind == _FLOAT:
            cargs[i] = float(a)
        elif kind == _BCAST:
            cargs[i] = ctypes.byref(a)
    _lib.check(getattr(_lib.lib(), name)(*cargs, _stream()), name)


def _size(name, g):
    """A size query of the library for geometry `g` (_lib.SIZE_T_FUNCS: host only, no stream)."""
    return int(getattr(_lib.lib(), name)(g._c_ref()))


def _three(v, fill):
    v = [int(x) for x in v]
    return [fill] * (3 - len(v)) + v


@dataclass(frozen=True)
class Geometry:
    """Operator geometry in the 3-D convention of `cdl_geom` (2-D: leading axis is 1)."""
    N: int
    C: int
    M: int
    dims: Tuple[int, int, int]        # padded image extents D,H,W
    P: Tuple[int, int, int]
    pad: Tuple[int, int, int]
    stride: Tuple[int, int, int]
    ndim: int                         # 2 or 3: how tensors are shaped on the Python side

    @staticmethod
    def make(N, C, M, spatial, P, pad, stride):
        nd = len(spatial)
        stride = [stride] * nd if isinstance(stride, int) else list(stride)
        g = Geometry(int(N), int(C), int(M), tuple(_three(spatial, 1)), tuple(_three(P, 1)),
                     tuple(_three(pad, 0)), tuple(_three(stride, 1)), nd)
        for d, s in zip(g.dims, g.stride):
            if d % s:
                raise ValueError(f"image extent {d} is not a multiple of stride {s}")
        for p, q in zip(g.P, g.pad):
            if p % 2 == 0 or q != p // 2:
                raise ValueError("filters must have odd extent with padding P//2 "
                                 "(the reference's conv/conv-transpose pair only closes for odd P)")
        return g

    @property
    def code_spatial(self):
        return tuple(d // s for d, s in zip(self.dims, self.stride))[3 - self.ndim:]

    @property
    def image_spatial(self):
        return self.dims[3 - self.ndim:]

    def c_struct(self):
        return _lib.Geom(self.N, self.C, self.M, *self.dims, *self.P, *self.pad, *self.stride)

    def _c_ref(self):
        """`const cdl_geom *` for a call: one struct per Geometry, made at first use (no entry point writes to it)."""
        gs = self.__dict__.get("_gs")
        if gs is None:
            gs = self.c_struct()
            object.__setattr__(self, "_gs", gs)
        return ctypes.byref(gs)

    def code_shape(self):
        return (self.N, self.M) + self.code_spatial

    def image_shape(self):
        return (self.N, self.C) + self.image_spatial

    def filter_shape(self):
        return (self.M, self.C) + self.P[3 - self.ndim:]


def _pads6(pads, ndim):
    """F.pad-ordered (last dim first) pads -> {d_lo,d_hi,h_lo,h_hi,w_lo,w_hi} int array."""
    per_axis = [(pads[2 * i], pads[2 * i + 1]) for i in range(ndim)][::-1]   # first spatial dim first
    flat = [0, 0] * (3 - ndim) + [v for lo_hi in per_axis for v in lo_hi]
    return (ctypes.c_int * 6)(*flat)


def split_pad(length, s):
    """(before, after) making `length` a multiple of s, floor/ceil split (model/utils.py:35-44)."""
    rem = length % s
    if rem == 0:
        return (0, 0)
    extra = s - rem
    return (extra // 2, extra - extra // 2)


def stride_pads(spatial, s):
    """F.pad-ordered tuple (model/utils.py:46-51, 103-111)."""
    out = []
    for length in reversed(tuple(spatial)):
        out.extend(split_pad(int(length), s))
    return tuple(out)


# ------------------------------------------------------------------------------------------
def preprocess(y, s, mask=None):
    """model/utils.py:5-22 / 70-87 on the device: returns (yp, mean(N,), pads, mask_p)."""
    y = _dev(y, "y")
    mask = _opt(mask, "mask")
    if mask is not None and mask.shape != y.shape:
        raise ValueError("mask must have the shape of y")
    nd = y.dim() - 2
    if nd not in (2, 3):
        raise ValueError("expected (N,C,H,W) or (N,C,D,H,W)")
    N, C = y.shape[:2]
    sp = _three(y.shape[2:], 1)
    pads = stride_pads(y.shape[2:], s)
    p6 = _pads6(pads, nd)
    padded = tuple(int(d) + p6[2 * i] + p6[2 * i + 1] for i, d in enumerate(sp))[3 - nd:]
    yp = torch.empty((N, C) + padded, device=y.device, dtype=torch.float32)
    mask_p = torch.empty_like(yp) if mask is not None else None
    mean = torch.empty(N, device=y.device, dtype=torch.float32)
    _call("cdl_preprocess", y, mask, yp, mask_p, mean, N, C, *sp, p6)
    return yp, mean, pads, mask_p


def postprocess(xp, mean, pads):
    """model/utils.py:24-33 / 89-101: crop the stride padding and add the mean back."""
    xp = _dev(xp, "xp")
    nd = xp.dim() - 2
    N, C = xp.shape[:2]
    p6 = _pads6(pads, nd)
    spp = _three(xp.shape[2:], 1)
    sp = [spp[i] - p6[2 * i] - p6[2 * i + 1] for i in range(3)]
    out = torch.empty((N, C) + tuple(sp[3 - nd:]), device=xp.device, dtype=torch.float32)
    _call("cdl_postprocess", xp, mean, out, N, C, *sp, p6)
    return out


def postprocess_bwd(gxhat, pads):
    gxhat = _dev(gxhat, "grad_xhat")
    nd = gxhat.dim() - 2
    N, C = gxhat.shape[:2]
    p6 = _pads6(pads, nd)
    sp = _three(gxhat.shape[2:], 1)
    spp = [sp[i] + p6[2 * i] + p6[2 * i + 1] for i in range(3)]
    out = torch.empty((N, C) + tuple(spp[3 - nd:]), device=gxhat.device, dtype=torch.float32)
    _call("cdl_postprocess_bwd", gxhat, out, N, C, *sp, p6)
    return out


def preprocess_bwd(dyp, pads, g_xhat=None, mask=None):
    """dL/dy from dL/dyp (the reflect pad's adjoint, the mean's) and, through the mean postprocess adds back, from
    dL/dxhat (cdl_preprocess_bwd).  `mask`: the unpadded mask preprocess was given."""
    dyp = _dev(dyp, "dyp")
    g_xhat, mask = _opt(g_xhat, "g_xhat"), _opt(mask, "mask")
    nd = dyp.dim() - 2
    N, C = dyp.shape[:2]
    p6 = _pads6(pads, nd)
    spp = _three(dyp.shape[2:], 1)
    sp = [spp[i] - p6[2 * i] - p6[2 * i + 1] for i in range(3)]
    dy = torch.empty((N, C) + tuple(sp[3 - nd:]), device=dyp.device, dtype=torch.float32)
    for t in (g_xhat, mask):
        assert t is None or tuple(t.shape) == tuple(dy.shape)
    _call("cdl_preprocess_bwd", dyp, g_xhat, mask, dy, N, C, *sp, p6)
    return dy


def thresholds(t, c, N):
    """tau (K,N,M) = t[k,0] + c[n]*t[k,1]; t is the (K,2,M,1,1[,1]) parameter."""
    t = _dev(t, "t")
    K, two, M = t.shape[:3]
    c = _opt(c, "c")
    tau = torch.empty((K, N, M), device=t.device, dtype=torch.float32)
    _call("cdl_thresholds", t, c, tau, K, N, M)
    return tau


def shrink(x, tau):
    """ST(x, tau) with tau (N,M) broadcast over the spatial axes (net.py:11-14)."""
    x, tau = _dev(x, "x"), _dev(tau, "tau")
    rows = x.shape[0] * x.shape[1]
    assert tau.numel() == rows
    out = torch.empty_like(x)
    _call("cdl_shrink", x, tau, out, rows, x.numel() // rows)
    return out


def bcast_strides(shape, code_shape):
    """cdl_bcast of a contiguous threshold of `shape` against `code_shape` = (N, M, *spatial): each of its first two axes
    is 1 or full, and its spatial axes are all 1 (the row form) or all full.  Raises ValueError otherwise."""
    shape, code_shape = tuple(int(v) for v in shape), tuple(int(v) for v in code_shape)
    sp = code_shape[2:]
    per_m = 1
    for d in sp:
        per_m *= d
    ok = len(shape) == len(code_shape) and shape[0] in (1, code_shape[0]) and shape[1] in (1, code_shape[1])
    spatial = ok and shape[2:] == sp and per_m > 1
    if not ok or not (spatial or all(d == 1 for d in shape[2:])):
        raise ValueError(f"threshold of shape {shape} is not a broadcast form of the code shape {code_shape}")
    p = 1 if spatial else 0
    dm = per_m if spatial else 1
    m = dm if shape[1] > 1 else 0
    n = (dm * shape[1] if shape[0] > 1 else 0)
    return _lib.Bcast(n, m, p)


def _thr(t, name, g_shape):
    t = _dev(t, name)
    return t, bcast_strides(t.shape, g_shape)


def shrink_b(x, tau):
    """ST(x, tau), tau a broadcast form of x's shape (bcast_strides) (cdl_shrink_b)."""
    x = _dev(x, "x")
    tau, st = _thr(tau, "tau", x.shape)
    N, M = x.shape[:2]
    out = torch.empty_like(x)
    _call("cdl_shrink_b", x, tau, st, out, N, M, x.numel() // (N * M))
    return out


def shrink_b_bwd(gup, x, tau, dtau_el=None):
    """Reverse of shrink_b: returns gx = gup at the support; dtau_el (shaped like x, optional) receives the threshold
    gradient per code element (cdl_shrink_b_bwd)."""
    gup, x = _dev(gup, "gup"), _dev(x, "x")
    tau, st = _thr(tau, "tau", x.shape)
    dtau_el = _buf(dtau_el, "dtau_el", x.shape)
    assert gup.shape == x.shape
    N, M = x.shape[:2]
    gx = torch.empty_like(x)
    _call("cdl_shrink_b_bwd", gup, x, tau, st, gx, dtau_el, N, M, x.numel() // (N * M))
    return gx


def prox_csr_b(g: Geometry, u, z_prev, lam, gam1, z_after=None, gam2=None):
    """prox_csr with thresholds of any broadcast form of the code shape (cdl_prox_csr_b)."""
    u, z_prev, z_after = _dev(u, "u"), _dev(z_prev, "z_prev"), _opt(z_after, "z_after")
    _check_codes(g, u=u, z_prev=z_prev, z_after=z_after)
    (lam, sl), (gam1, s1) = _thr(lam, "lam", g.code_shape()), _thr(gam1, "gam1", g.code_shape())
    gam2, s2 = _thr(gam2, "gam2", g.code_shape()) if z_after is not None else (None, _lib.Bcast(0, 0, 0))
    out = torch.empty_like(u)
    _call("cdl_prox_csr_b", g, u, z_prev, z_after, lam, sl, gam1, s1, gam2, s2, out)
    return out


def prox_csr_b_bwd(g: Geometry, gz, u, z_prev, lam, gam1, z_after=None, gam2=None, want=(True, True, True),
                   gz_prev=None, gz_after=None):
    """Reverse of prox_csr_b: returns (gu, dlam, dgam1, dgam2); gz_prev / gz_after (code-shaped, optional) are accumulated
    into.  Each threshold gradient asked for in `want` comes before the reduction over the threshold's broadcast axes:
    (N, M, 1..) row sums for a threshold without spatial extent, the code shape for one with."""
    gz, u, z_prev, z_after = _dev(gz, "gz"), _dev(u, "u"), _dev(z_prev, "z_prev"), _opt(z_after, "z_after")
    gz_prev, gz_after = _buf(gz_prev, "gz_prev", g.code_shape()), _buf(gz_after, "gz_after", g.code_shape())
    _check_codes(g, gz=gz, u=u, z_prev=z_prev, z_after=z_after)
    (lam, sl), (gam1, s1) = _thr(lam, "lam", g.code_shape()), _thr(gam1, "gam1", g.code_shape())
    gam2, s2 = _thr(gam2, "gam2", g.code_shape()) if z_after is not None else (None, _lib.Bcast(0, 0, 0))
    rows = (g.N, g.M) + (1,) * g.ndim

    def buf(wanted, st):
        return torch.empty(g.code_shape() if st.p else rows, device=gz.device, dtype=torch.float32) if wanted else None

    dl, d1 = buf(want[0], sl), buf(want[1], s1)
    d2 = buf(want[2], s2) if z_after is not None else None
    gu = torch.empty_like(gz)
    n = _size("cdl_prox_csr_scratch_floats", g)
    scratch = torch.empty(n, device=gz.device, dtype=torch.float32)
    _call("cdl_prox_csr_b_bwd", g, gz, u, z_prev, z_after, lam, sl, gam1, s1, gam2, s2, gu, gz_prev, gz_after, dl, d1, d2,
          scratch, n)
    return gu, dl, d1, d2


def _check_map(g: Geometry, cmap, tslope=None, rows=1):
    """A noise-level map is a dense (N, 1, *code_spatial) tensor; its slope row(s) hold `rows` * M values."""
    if cmap is not None and tuple(cmap.shape) != (g.N, 1) + g.code_spatial:
        raise ValueError(f"cmap: shape {tuple(cmap.shape)} is not the code grid {(g.N, 1) + g.code_spatial}")
    if tslope is not None and tslope.numel() != rows * g.M:
        raise ValueError(f"tslope: expected {rows * g.M} values, got {tslope.numel()}")


def _check_map_pair(g: Geometry, cmap, tslope, rows=1):
    """A noise-level map and its slope row(s) go together: both through `_opt` and `_check_map`, or both None."""
    cmap, tslope = _opt(cmap, "cmap"), _opt(tslope, "tslope")
    if (cmap is None) != (tslope is None):
        raise ValueError("cmap and tslope go together")
    _check_map(g, cmap, tslope, rows)
    return cmap, tslope


def _check_rows(g: Geometry, **thresholds):
    """Thresholds of the (N, M) row form: one value per (sample, channel)."""
    for name, t in thresholds.items():
        if t is not None and t.numel() != g.N * g.M:
            raise ValueError(f"{name}: expected {g.N * g.M} per-(sample, channel) thresholds")


def _check_codes(g: Geometry, **tensors):
    for name, t in tensors.items():
        if t is not None and (tuple(t.shape) != g.code_shape() or not t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous tensor of the code shape {g.code_shape()}")


def analysis(g: Geometry, x, w, alpha=1.0, zin=None, gate=None, tau=None, out=None, *, cmap=None, tslope=None):
    """cdl_analysis.  cmap (N,1,*code_spatial) with tslope (M): the threshold of element (n, m, pix) is
    tau[n,m] + cmap[n,pix] * tslope[m] (tau then holds t[k,0,m])."""
    x, w = _dev(x, "x"), _dev(w, "w")
    zin, gate, tau = _opt(zin, "zin"), _opt(gate, "gate"), _opt(tau, "tau")
    cmap, tslope = _check_map_pair(g, cmap, tslope)
    assert tuple(x.shape) == g.image_shape(), (x.shape, g.image_shape())
    assert tuple(w.shape) == g.filter_shape(), (w.shape, g.filter_shape())
    out = _new(g.code_shape(), x.device) if out is None else _buf(out, "out")
    ws, n = _analysis_workspace(g, x.device)
    _call("cdl_analysis", g, x, w, alpha, zin, gate, tau, out, ws, n, cmap, tslope)
    return out


def synthesis(g: Geometry, z, w, alpha=1.0, gate=None, mask=None, sub=None, out=None):
    z, w = _dev(z, "z"), _dev(w, "w")
    gate, mask, sub = _opt(gate, "gate"), _opt(mask, "mask"), _opt(sub, "sub")
    assert tuple(z.shape) == g.code_shape(), (z.shape, g.code_shape())
    assert tuple(w.shape) == g.filter_shape(), (w.shape, g.filter_shape())
    out = _new(g.image_shape(), z.device) if out is None else _buf(out, "out")
    n = _size("cdl_synthesis_workspace_floats", g)
    _call("cdl_synthesis", g, z, gate, w, alpha, mask, sub, out, _scratch(z.device, n) if n else None, n)
    return out


_WGRAD_WS = {}
_SCRATCH = {}


def _scratch(device, n):
    """One grow-only scratch buffer per (device, STREAM) for kernels that need transient partial sums: launches on one
    stream are ordered, so they may share it; two streams each get their own (a single per-device buffer would be a
    silent race between concurrent streams)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < n:
        buf = _SCRATCH[key] = torch.empty(n, device=device, dtype=torch.float32)
    return buf


def _analysis_workspace(g: Geometry, device):
    """(scratch or None, floats) for the analysis entry points that take a workspace."""
    n = _size("cdl_analysis_workspace_floats", g)
    return (_scratch(device, n) if n else None), n


def _wgrad_workspace(g: Geometry, device):
    """(buffer, floats): the filter-gradient workspace, one per (device, stream, size), reused."""
    n = _size("cdl_wgrad_workspace_floats", g)
    key = (device, torch.cuda.current_stream(device).cuda_stream, n)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = _WGRAD_WS[key] = torch.empty(max(n, 1), device=device, dtype=torch.float32)
    return ws, n


def _filter_grads(g: Geometry, K, device):
    """(dA list, dB list) of a reverse sweep: one allocation, 2K views (at cfg1's size the allocator calls cost more
    than the kernels)."""
    dAB = torch.empty((2 * K,) + g.filter_shape(), device=device, dtype=torch.float32)
    return list(dAB[:K].unbind(0)), list(dAB[K:].unbind(0))


def wgrad(g: Geometry, z, x, alpha=1.0, gate=None):
    z, x, gate = _dev(z, "z"), _dev(x, "x"), _opt(gate, "gate")
    dw = torch.empty(g.filter_shape(), device=z.device, dtype=torch.float32)
    ws, n = _wgrad_workspace(g, z.device)
    _call("cdl_wgrad", g, z, gate, x, alpha, dw, ws, n)
    return dw


def wgrad_pair(g: Geometry, z0, x0, alpha0, z1, x1, alpha1):
    """(alpha0 * z0 (x) x0, alpha1 * z1 (x) x1): the two ungated filter gradients of one reverse iteration, one
    launch where the matrix-core kernel covers the shape (cdl_wgrad_pair)."""
    z0, x0, z1, x1 = _dev(z0, "z0"), _dev(x0, "x0"), _dev(z1, "z1"), _dev(x1, "x1")
    dw0 = torch.empty(g.filter_shape(), device=z0.device, dtype=torch.float32)
    dw1 = torch.empty_like(dw0)
    ws, n = _wgrad_workspace(g, z0.device)
    _call("cdl_wgrad_pair", g, z0, x0, alpha0, dw0, z1, x1, alpha1, dw1, ws, n)
    return dw0, dw1


def _dt_halves(g: Geometry, dt_k, name="dt_k"):
    """The (2, M) threshold-gradient slice of one iteration as its two rows (views: the kernels take them separately)."""
    halves = _buf(dt_k, name).reshape(2, -1)
    if halves.shape[1] != g.M:
        raise ValueError(f"{name}: expected 2 x {g.M} values, got {dt_k.numel()}")
    return halves[0], halves[1]


def _dtau_rows(g: Geometry, dtau_n):
    """The optional per-sample (N, M) threshold gradient of one iteration."""
    if _buf(dtau_n, "dtau_n") is not None and dtau_n.numel() != g.N * g.M:
        raise ValueError(f"dtau_n: expected {g.N * g.M} values, got {dtau_n.numel()}")
    return dtau_n


def tau_grad(g: Geometry, gup, zout, c, dt_k, dtau_n=None, *, cmap=None, gate=False):
    """Writes the (2,M) slice `dt_k` of the threshold gradient for one iteration [and the per-sample (N,M) `dtau_n`].
    cmap (in place of c): dt_k[1] is weighted by the noise-level map.  gate: `gup` is also gated in place by the support
    of `zout` (cdl_tau_grad_gate)."""
    gup, zout, c, cmap = _dev(gup, "g"), _dev(zout, "zout"), _opt(c, "c"), _opt(cmap, "cmap")
    _check_map(g, cmap)
    dt0, dt1 = _dt_halves(g, dt_k)
    dtau_n = _dtau_rows(g, dtau_n)
    # CDL_TAU_SPLITS * N * M (twice with a map)
    scratch = torch.empty((32 if cmap is not None else 16) * g.N * g.M, device=gup.device, dtype=torch.float32)
    _call("cdl_tau_grad_gate" if gate else "cdl_tau_grad", g, gup, zout, c, dt0, dt1, dtau_n, scratch, cmap)


def sigma_grad(g: Geometry, du, z, tslope, dcmap, acc_add):
    """dcmap (N,1,*code_spatial) (+)= -sum_m tslope[m] sign(z) du: the noise-level map's gradient of one iteration
    (cdl_sigma_grad); du is the gated dL/du_k, z = z_{k+1}."""
    du, z, tslope = _dev(du, "du"), _dev(z, "z"), _dev(tslope, "tslope")
    _check_map(g, _buf(dcmap, "dcmap"), tslope)
    assert tuple(du.shape) == g.code_shape() == tuple(z.shape)
    _call("cdl_sigma_grad", g, du, z, tslope, dcmap, bool(acc_add))


def dyp_split(g: Geometry, q, mask, dyp, acc_add, make_q=True):
    """Generic reverse sweep: q holds S = A_k^T du_k (unmasked); dyp (+)= S, then q = -mask * S in place (cdl_dyp_split)."""
    q, dyp = _buf(q, "q", g.image_shape()), _buf(dyp, "dyp", g.image_shape())
    _call("cdl_dyp_split", g, q, _opt(mask, "mask"), dyp, bool(acc_add), bool(make_q))


def analysis_rev(g: Geometry, x, w, alpha, zin, zsup, c, dt_k, out=None, *, cmap=None):
    """One reverse-sweep step (cdl_analysis_rev): out = [zsup != 0] (zin + alpha A x), and the (2, M) threshold
    gradient slice `dt_k` of `out` with respect to the code `zsup` -- cdl_analysis followed by cdl_tau_grad_gate, as one
    fat launch where the matrix-core analysis covers the geometry."""
    x, w, zin, zsup, c = _dev(x, "x"), _dev(w, "w"), _opt(zin, "zin"), _dev(zsup, "zsup"), _opt(c, "c")
    cmap = _opt(cmap, "cmap")                                  # the noise-level map in place of c (dt_k[1] weighted by it)
    _check_map(g, cmap)
    dt0, dt1 = _dt_halves(g, dt_k)
    out = _new(g.code_shape(), x.device) if out is None else _buf(out, "out")
    n = _size("cdl_analysis_rev_workspace_floats", g)
    _call("cdl_analysis_rev", g, x, w, alpha, zin, zsup, c, dt0, dt1, None, out, _scratch(x.device, n), n, cmap)
    return out


def prox_csr(g: Geometry, u, z_prev, lam, gam1, z_after=None, gam2=None, out=None):
    """prox_CSR (z_after None) / prox_CSR_f2 of net.py:229-262; lam, gam* are (N,M) like tau."""
    u, z_prev, lam, gam1 = _dev(u, "u"), _dev(z_prev, "z_prev"), _dev(lam, "lam"), _dev(gam1, "gam1")
    z_after, gam2 = _opt(z_after, "z_after"), _opt(gam2, "gam2")
    _check_codes(g, u=u, z_prev=z_prev, z_after=z_after)
    _check_rows(g, lam=lam, gam1=gam1, gam2=gam2)
    out = torch.empty_like(u) if out is None else _buf(out, "out", g.code_shape())
    _call("cdl_prox_csr", g, u, z_prev, z_after, lam, gam1, gam2, out)
    return out


def analysis_prox(g: Geometry, x, w, alpha, zin, z_prev, lam, gam1, z_after=None, gam2=None, u_out=None, out=None, *,
                  cmap=None, tslope=None):
    """cdl_analysis with the CSR map as epilogue: returns z = prox(zin + alpha*corr(x; w)); `u_out`
    (a code-shaped tensor) receives the pre-shrinkage value when given.  cmap (N,1,*code_spatial) with tslope (3,M): the
    thresholds of element (n, m, pix) are lam[n,m] + cmap[n,pix] * tslope[0,m], and the same for gam1, gam2."""
    x, w = _dev(x, "x"), _dev(w, "w")
    cmap, tslope = _check_map_pair(g, cmap, tslope, 3)          # the slopes of lam, gam1, gam2
    zin, z_prev, z_after = _opt(zin, "zin"), _dev(z_prev, "z_prev"), _opt(z_after, "z_after")
    assert tuple(x.shape) == g.image_shape(), (x.shape, g.image_shape())
    assert tuple(w.shape) == g.filter_shape(), (w.shape, g.filter_shape())
    _check_codes(g, zin=zin, z_prev=z_prev, z_after=z_after)
    u_out = _buf(u_out, "u_out", g.code_shape())
    out = _new(g.code_shape(), x.device) if out is None else _buf(out, "out")
    ws, n = _analysis_workspace(g, x.device)
    _call("cdl_analysis_prox", g, x, w, alpha, zin, z_prev, z_after, _dev(lam, "lam"), _dev(gam1, "gam1"),
          _opt(gam2, "gam2"), u_out, out, ws, n, cmap, tslope)
    return out


def prox_csr_tangent(g: Geometry, ud, u, z_prev, lam, gam1, z_after=None, gam2=None, zd_prev=None, zd_after=None,
                     out=None, *, cmap=None, tslope=None):
    """Tangent of prox_csr at the primal (u, z_prev[, z_after]) along (ud, zd_prev, zd_after) (cdl_prox_csr_tangent): a nest
    of gates read off the primal's intermediates; a None neighbour tangent is a zero one.  out may be ud.
    cmap / tslope as analysis_prox's (lam, gam* then hold the constant parts): the gates are read at the primal's thresholds."""
    cmap, tslope = _check_map_pair(g, cmap, tslope, 3)
    ud, u, z_prev, lam, gam1 = _dev(ud, "ud"), _dev(u, "u"), _dev(z_prev, "z_prev"), _dev(lam, "lam"), _dev(gam1, "gam1")
    z_after, gam2 = _opt(z_after, "z_after"), _opt(gam2, "gam2")
    zd_prev, zd_after = _opt(zd_prev, "zd_prev"), _opt(zd_after, "zd_after")
    _check_codes(g, ud=ud, u=u, z_prev=z_prev, z_after=z_after, zd_prev=zd_prev, zd_after=zd_after)
    _check_rows(g, lam=lam, gam1=gam1, gam2=gam2)
    out = torch.empty_like(ud) if out is None else _buf(out, "out", g.code_shape())
    _call("cdl_prox_csr_tangent", g, ud, u, z_prev, z_after, lam, gam1, gam2, zd_prev, zd_after, out, cmap, tslope)
    return out


def analysis_prox_tangent(g: Geometry, x, w, alpha, zin, u, z_prev, lam, gam1, z_after=None, gam2=None, zd_prev=None,
                          zd_after=None, out=None, *, cmap=None, tslope=None):
    """cdl_analysis followed by the tangent of the CSR map in place (cdl_analysis_prox_tangent): with ud = zin +
    alpha*corr(x; w), returns Jprox(u; z_prev[, z_after]) (ud, zd_prev, zd_after) -- the bits of analysis, then prox_csr_tangent.
    cmap / tslope: as prox_csr_tangent's."""
    x, w = _dev(x, "x"), _dev(w, "w")
    cmap, tslope = _check_map_pair(g, cmap, tslope, 3)
    zin, u, z_prev, z_after = _opt(zin, "zin"), _dev(u, "u"), _dev(z_prev, "z_prev"), _opt(z_after, "z_after")
    zd_prev, zd_after = _opt(zd_prev, "zd_prev"), _opt(zd_after, "zd_after")
    assert tuple(x.shape) == g.image_shape(), (x.shape, g.image_shape())
    assert tuple(w.shape) == g.filter_shape(), (w.shape, g.filter_shape())
    _check_codes(g, zin=zin, u=u, z_prev=z_prev, z_after=z_after, zd_prev=zd_prev, zd_after=zd_after)
    out = _new(g.code_shape(), x.device) if out is None else _buf(out, "out", g.code_shape())
    ws, n = _analysis_workspace(g, x.device)
    _call("cdl_analysis_prox_tangent", g, x, w, alpha, zin, u, z_prev, z_after, _dev(lam, "lam"), _dev(gam1, "gam1"),
          _opt(gam2, "gam2"), zd_prev, zd_after, out, ws, n, cmap, tslope)
    return out


def prox_csr_bwd(g: Geometry, gz, u, z_prev, lam, gam1, c, dlam, dgam1, z_after=None, gam2=None, dgam2=None,
                 gz_prev=None, gz_after=None, out=None, *, cmap=None, tslope=None, dcmap=None, dsum_n=None):
    """Reverse of prox_csr: returns gu; accumulates into gz_prev / gz_after; writes the (2,M) slices
    dlam, dgam1[, dgam2] of the threshold gradients of this iteration.  dsum_n (3,N,M): the threshold sums per sample.
    cmap / tslope as analysis_prox's (c is then None): the slices receive [sum s, sum cmap*s], and dcmap
    (N,1,*code_spatial) is accumulated into."""
    gz, u, z_prev = _dev(gz, "gz"), _dev(u, "u"), _dev(z_prev, "z_prev")
    z_after, gam2, c = _opt(z_after, "z_after"), _opt(gam2, "gam2"), _opt(c, "c")
    cmap, tslope = _check_map_pair(g, cmap, tslope, 3)
    if _buf(dcmap, "dcmap") is not None:
        if cmap is None:
            raise ValueError("dcmap: there is no cmap to take the gradient of")
        _check_map(g, dcmap)
    dsum_n = _buf(dsum_n, "dsum_n", (3, g.N, g.M))
    for name, t in (("dlam", dlam), ("dgam1", dgam1), ("dgam2", dgam2)):
        if _buf(t, name) is not None and t.numel() != 2 * g.M:
            raise ValueError(f"{name}: expected 2 x {g.M} values, got {t.numel()}")
    gz_prev, gz_after = _buf(gz_prev, "gz_prev", g.code_shape()), _buf(gz_after, "gz_after", g.code_shape())
    out = torch.empty_like(gz) if out is None else _buf(out, "out", g.code_shape())
    n = _size("cdl_prox_csr_scratch_floats", g)
    scratch = torch.empty(n, device=gz.device, dtype=torch.float32)
    _call("cdl_prox_csr_bwd", g, gz, u, z_prev, z_after, _dev(lam, "lam"), _dev(gam1, "gam1"), gam2, c, out, gz_prev,
          gz_after, dlam, dgam1, dgam2, scratch, n, cmap, tslope, dcmap, dsum_n)
    return out


def residual_geometry(x, w):
    """Geometry of a ResidualBlock conv (net.py:105-120): C == M channels, unit stride, padding P//2."""
    M = int(w.shape[0])
    if tuple(w.shape[:2]) != (M, M) or x.shape[1] != M:
        raise ValueError(f"ResidualBlock expects (M,M,...) filters and M-channel input, got {tuple(w.shape)} / {tuple(x.shape)}")
    P = tuple(w.shape[2:])
    return Geometry.make(x.shape[0], M, M, x.shape[2:], P, tuple(p // 2 for p in P), 1)


def residual_forward(g: Geometry, x, w1, w2):
    """(h, out) = (relu(conv1 x), relu(conv2 h + x)); h is what the reverse pass keeps."""
    x, w1, w2 = _dev(x, "x"), _dev(w1, "w1"), _dev(w2, "w2")
    assert tuple(x.shape) == g.code_shape() and tuple(w1.shape) == g.filter_shape() == tuple(w2.shape)
    h, out = torch.empty_like(x), torch.empty_like(x)
    n = _size("cdl_residual_scratch_floats", g)
    _call("cdl_residual_forward", g, x, w1, w2, h, out, _scratch(x.device, n) if n else None, n)
    return h, out


def residual_backward(g: Geometry, x, h, out, w1, w2, g_out):
    """(dx, dw1, dw2) for g_out = dL/dout."""
    x, h, out = _dev(x, "x"), _dev(h, "h"), _dev(out, "out")
    w1, w2, g_out = _dev(w1, "w1"), _dev(w2, "w2"), _dev(g_out, "g_out")
    new = lambda t: torch.empty(t.shape, device=t.device, dtype=torch.float32)      # contiguous, whatever t's strides
    dx, dh = new(x), new(x)
    dw1, dw2 = new(w1), new(w2)
    n = _size("cdl_residual_scratch_floats", g)
    _call("cdl_residual_backward", g, x, h, out, w1, w2, g_out, dx, dw1, dw2, dh, _scratch(x.device, n) if n else None, n)
    return dx, dw1, dw2


def project_filters_(w):
    """In-place unit-ball projection of every (m,c) filter of w (M,C,*P): project_filter_banks_ of one bank."""
    project_filter_banks_([w])
    return w


def project_filter_banks_(banks):
    """In-place unit-ball projection of every filter of every bank (same-shaped (M,C,*P) tensors): one launch."""
    banks = list(banks)
    if not banks:
        return
    w0 = banks[0]
    for w in banks:
        if not w.is_cuda:
            raise RuntimeError("project(): parameters must live on the ROCm device (no CPU path)")
        assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == w0.shape
    nf = w0.shape[0] * w0.shape[1]
    _call("cdl_project_filter_banks", banks, len(banks), nf, w0.numel() // nf)


def gabor_filters(alpha, a, w0, psi, P, transpose):
    """The (M,C,P,P) filters of one bank: gabor_filter_banks of one bank."""
    return gabor_filter_banks([(alpha, a, w0, psi)], P, [transpose])[0]


def gabor_filters_bwd(alpha, a, w0, psi, dw, P, transpose):
    """[dalpha, da, dw0, dpsi] of one bank for the upstream dw: gabor_filter_banks_bwd of one bank."""
    return list(gabor_filter_banks_bwd([(alpha, a, w0, psi)], [dw], P, [transpose])[0])


def gabor_filter_banks(params, P, transposes):
    """All banks of a net in one launch.  params: [(alpha, a, w0, psi)] per bank; returns the list of (M,C,P,P)
    filters (views of one allocation)."""
    nb = len(params)
    params = [tuple(_dev(v, n) for v, n in zip(pr, ("alpha", "a", "w0", "psi"))) for pr in params]
    order, M, C = params[0][3].shape
    out = torch.empty((nb, M, C, P, P), device=params[0][3].device, dtype=torch.float32)
    ws = list(out.unbind(0))
    flags = (ctypes.c_int * nb)(*[int(bool(t)) for t in transposes])
    _call("cdl_gabor_filter_banks", nb, *zip(*params), flags, ws, order, M, C, P)
    return ws


def gabor_filter_banks_bwd(params, dws, P, transposes):
    """Adjoint of gabor_filter_banks in one launch: per bank (dalpha, da, dw0, dpsi) for upstream dws[k] (None: zeros)."""
    nb = len(params)
    params = [tuple(_dev(v, n) for v, n in zip(pr, ("alpha", "a", "w0", "psi"))) for pr in params]
    dws = [None if d is None else _dev(d, "dw") for d in dws]
    order, M, C = params[0][3].shape
    nq = order * M * C
    dev = params[0][3].device
    blocks = torch.empty((nb, 6 * nq), device=dev, dtype=torch.float32)
    flags = (ctypes.c_int * nb)(*[int(bool(t)) for t in transposes])
    _call("cdl_gabor_filter_banks_bwd", nb, *zip(*params), flags, dws, blocks.unbind(0), order, M, C, P)
    outs = []
    for k, pr in enumerate(params):
        b = blocks[k]
        outs.append((b[:nq].view_as(pr[0]), b[nq:3 * nq].view_as(pr[1]), b[3 * nq:5 * nq].view_as(pr[2]),
                     b[5 * nq:].view_as(pr[3])))
    return outs


# ------------------------------------------------------------------------------------------ fused MFMA path
PRECISION = {"split3": 0, "bf16": 1, "split4": 2}


class exact_fp32:
    """`with exact_fp32(): ...` -- the shape-generic entry points called from this thread inside the block stay on the fp32
    VALU kernels (cdl_set_exact_fp32, include/cdlnet_hip.h); `exact_fp32(False)` is a no-op block."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        if self.on:
            self.prev = _lib.lib().cdl_set_exact_fp32(1)
        return self

    def __exit__(self, *exc):
        if self.on:
            _lib.lib().cdl_set_exact_fp32(self.prev)
        return False


# ------------------------------------------------------------------------------------------ launch trace
@dataclass(frozen=True)
class LaunchRecord:
    """One kernel launch as the library's trace recorded it (cdl_trace, include/cdlnet_hip.h)."""
    file: str          # source file of the launch site, e.g. "cdl_analysis_mfma.hip"
    line: int          # line of the site's CDL_LAUNCH_CHECK
    func: str          # the launcher with the values of its template arguments
    note: str          # run-time variant values of the plan ("MTW=2 tpw=4 ..."), the kernel's name where it is needed

    def template(self):
        """The launcher's template arguments as the compiler printed them: {"PH": 7, "REV": True, ...}."""
        out = {}
        if self.func.endswith("]") and "[" in self.func:
            for tok in self.func[self.func.rindex("[") + 1:-1].split(","):
                if "=" in tok:
                    k, v = (t.strip() for t in tok.split("=", 1))
                    out[k] = {"true": True, "false": False}.get(v, int(v) if v.lstrip("-").isdigit() else v)
        return out

    def values(self):
        """The note's `name=value` pairs, integers where they parse."""
        out = {}
        for tok in self.note.split():
            if "=" in tok:
                k, v = tok.split("=", 1)
                out[k] = int(v) if v.lstrip("-").isdigit() else v
        return out


def parse_trace(text):
    """Records of a trace log (cdl_trace_read or a CDL_TRACE_FILE), in order."""
    out = []
    for ln in text.splitlines():
        parts = ln.split("\t")
        if len(parts) != 3 or ":" not in parts[0]:
            continue
        f, _, n = parts[0].rpartition(":")
        out.append(LaunchRecord(f, int(n), parts[1], parts[2]))
    return out


class Trace(list):
    """The records of a `with trace() as t:` block (filled when the block ends, or by `t.read()` inside it)."""

    def read(self):
        lib = _lib.lib()
        n = lib.cdl_trace_read(None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        lib.cdl_trace_read(buf, n + 1)
        self[:] = parse_trace(buf.value.decode())
        return self

    def files(self):
        return {r.file for r in self}

    def find(self, file=None, func=None, note=None):
        """Records from `file` whose launcher contains `func` and whose note contains `note`."""
        return [r for r in self if (file is None or r.file == file) and (func is None or func in r.func)
                and (note is None or note in r.note)]


class trace:
    """`with trace() as t: ...` -- the kernel launches the library made inside the block, from every thread (the log is
    process-wide: autograd runs the backward on another thread).  Synchronise before leaving the block if launches
    of other threads are expected."""

    def __enter__(self):
        self.prev = _lib.lib().cdl_trace(1)
        self.t = Trace()
        return self.t

    def __exit__(self, *exc):
        self.t.read()
        _lib.lib().cdl_trace(self.prev)
        return False


# layouts of the fat tensors that stay inside a fused sweep (include/cdlnet_hip.h, CDL_LAY_*): "nchw" is the
# reference's layout, "blocked" the pixel-blocked fp32 layout (same values, 16-byte accesses, the default),
# "blocked_bf16" opt-in bf16 STORAGE of the codes (half the bytes; outside the 1e-5 parity gate)
LAYOUT = {"nchw": 0, "blocked": 1, "blocked_bf16": 2, "rsc": 3}
_FUSED_LAYOUTS = ("nchw", "blocked", "blocked_bf16")     # of the fused 2-D kernels; "rsc": the strip kernels' (fusedg_*)
TILES_REVERSED = 16
TAU_PER_PLANE = 512                # cdl_fusedg_* only: one threshold row per (sample, depth) plane (CDL_TAU_PER_PLANE)


def _lay_in(layout):
    return LAYOUT[layout] << 5


def _lay_out(layout):
    return LAYOUT[layout] << 7


def fused_code_buffer(g: "Geometry", layout, device, count=1):
    """`count` code tensors in `layout`: NCHW tensors for "nchw", flat byte-sized fp32 / bf16 buffers otherwise."""
    if layout == "nchw":
        return torch.empty((count,) + g.code_shape(), device=device, dtype=torch.float32)
    nbytes = int(_lib.lib().cdl_fused2d_code_bytes(ctypes.byref(g.c_struct()), LAYOUT[layout]))
    assert nbytes > 0
    if layout == "blocked":
        return torch.empty((count, nbytes // 4), device=device, dtype=torch.float32)
    return torch.empty((count, nbytes // 2), device=device, dtype=torch.bfloat16)


def fused_to_nchw(g: "Geometry", t, layout):
    """A blocked code tensor as (N, M, H, W) fp32 (host-side plumbing for tests and tools: a torch permute)."""
    if layout == "nchw":
        return t
    H, W = g.dims[1], g.dims[2]
    XB = (W + 31) // 32
    v = t.reshape(g.N, H, XB, g.M // 4, 32, 4).to(torch.float32)
    return v.permute(0, 3, 5, 1, 2, 4).reshape(g.N, g.M, H, XB * 32)[..., :W].contiguous()


def fused_from_nchw(g: "Geometry", z, layout):
    """Inverse of fused_to_nchw (padding pixels are zero)."""
    if layout == "nchw":
        return z
    H, W = g.dims[1], g.dims[2]
    XB = (W + 31) // 32
    zp = torch.nn.functional.pad(z, (0, XB * 32 - W))
    v = zp.reshape(g.N, g.M // 4, 4, H, XB, 32).permute(0, 3, 4, 1, 5, 2).contiguous().reshape(1, -1)
    return v[0].to(torch.bfloat16 if layout == "blocked_bf16" else torch.float32)


def fused_supported(g: Geometry) -> bool:
    return bool(_size("cdl_fused2d_supported", g))


def fused_prep(wA, wB):
    """bf16 hi/lo MFMA fragments for one launch: analysis bank wA with the synthesis bank wB that
    consumes its output (B_{k+1}, or D after the last iteration)."""
    wA, wB = _dev(wA, "wA"), _dev(wB, "wB")
    M, P = wA.shape[0], wA.shape[-1]
    nbytes = _lib.lib().cdl_fused2d_frag_bytes(M)
    frags = torch.empty(nbytes, device=wA.device, dtype=torch.uint8)
    _call("cdl_fused2d_prep", wA, wB, frags, M, P)
    return frags


def fused_patches(g: Geometry, device):
    return torch.empty(_size("cdl_fused2d_patch_floats", g), device=device, dtype=torch.float32)


def fused_map(g: Geometry, device):
    """Empty support/sign bit map of one code tensor: (N, 4, H, W) int32 words (cdl_fused2d_map_words)."""
    assert _size("cdl_fused2d_map_words", g) == g.N * 4 * g.dims[1] * g.dims[2]
    return torch.empty((g.N, 4, g.dims[1], g.dims[2]), device=device, dtype=torch.int32)


def fused_support_map(g: Geometry, z, out=None):
    """The bit map the reverse stage reads instead of the fat z (built from a tensor; the training forward
    gets it for free from cdl_fused2d_iter_fwd)."""
    z = _dev(z, "z")
    assert tuple(z.shape) == g.code_shape()
    out = fused_map(g, z.device) if out is None else _buf(out, "out", dtype=torch.int32)
    _call("cdl_fused2d_support_map", g, z, out)
    return out


def _assemble(symbol, g, patches, mask, sub, alpha, out, acc, acc_add, write_out):
    patches, acc = _buf(patches, "patches"), _buf(acc, "acc", g.image_shape())
    mask, sub = _opt(mask, "mask"), _opt(sub, "sub")
    out = (_new(g.image_shape(), patches.device) if out is None else _buf(out, "out")) if write_out else None
    _call(symbol, g, patches, mask, sub, alpha, out, acc, bool(acc_add))
    return out


def fused_assemble(g: Geometry, patches, mask=None, sub=None, alpha=1.0, out=None, acc=None, acc_add=False,
                   write_out=True):
    """out = mask * alpha * (overlap-sum of the patches) - sub [and acc = S or acc += S with S the unmasked, unscaled
    overlap-sum]; write_out=False: acc only.  Returns out (None without write_out)."""
    return _assemble("cdl_fused2d_assemble", g, patches, mask, sub, alpha, out, acc, acc_add, write_out)


def fused_tiles(g: Geometry) -> int:
    return _size("cdl_fused2d_tiles", g)


def _dtau_reduce(symbol, g, dtau_partial, c, dt_k, dtau_n, *more):
    dt0, dt1 = _dt_halves(g, dt_k)
    _call(symbol, g, _buf(dtau_partial, "dtau_partial"), _opt(c, "c"), dt0, dt1, _dtau_rows(g, dtau_n), *more)


def fused_dtau_reduce(g: Geometry, dtau_partial, c, dt_k, dtau_n=None, *, weighted=None):
    """(2,M) `dt_k` [and the per-image (N,M) `dtau_n`].  weighted (in place of c): the map-weighted partials of a reverse
    stage that ran with a noise-level map -- rows fused_tiles(g).. of its dtau_partial; dt_k[1] is their sum."""
    if weighted is not None and c is not None:
        raise ValueError("the weighted partials replace the per-sample level c")
    if _buf(weighted, "weighted") is not None and weighted.numel() < fused_tiles(g) * g.M:
        raise ValueError(f"weighted: expected {fused_tiles(g)} x {g.M} values, got {weighted.numel()}")
    _dtau_reduce("cdl_fused2d_dtau_reduce", g, dtau_partial, c, dt_k, dtau_n, weighted)


def fused_wgrad_workspace(g: Geometry, device):
    return torch.empty(_size("cdl_fused2d_wgrad_workspace_floats", g), device=device, dtype=torch.float32)


def fused_wgrad(g: Geometry, workspace, X0=None, T0=None, alpha0=1.0, X1=None, T1=None, alpha1=1.0,
                precision="split3", layout="nchw", tiles_reversed=False):
    """Up to two filter gradients in one launch: dw_a = alpha_a * sum X_a (x) im2col(T_a); `layout` of X0, X1.
    tiles_reversed: walk the tiles from the last to the first (what every other launch of a sweep does)."""
    outs = []
    args = []
    for X, T, al in ((X0, T0, alpha0), (X1, T1, alpha1)):
        if X is None:
            outs.append(None)
            args += [None, None, 0.0, None]
        else:
            X, T = (_dev(X, "X") if layout == "nchw" else X), _dev(T, "T")
            outs.append(torch.empty(g.filter_shape(), device=X.device, dtype=torch.float32))
            args += [X, T, al, outs[-1]]
    _call("cdl_fused2d_wgrad", g, *args, _buf(workspace, "workspace"),
          PRECISION[precision] | _lay_in(layout) | (TILES_REVERSED if tiles_reversed else 0))
    return outs


def _check_data_grads(g: Geometry, K, dyp, dtau, families=1, rows=None):
    """The optional outputs of the *_backward sweeps: dyp (thin, as yp), dtau (K,N,M) -- (K,3,N,M) for the three threshold
    families of the CSR sweep, (K,rows,M) with per-plane thresholds; contiguous fp32."""
    _buf(dyp, "dyp", g.image_shape())
    rows = g.N if rows is None else rows
    _buf(dtau, "dtau", (K, rows, g.M) if families == 1 else (K, families, rows, g.M))


def _dt_sweep(g: Geometry, K, dt, name="dt"):
    """The (K, 2, M) threshold gradient a reverse sweep fills (None stays None)."""
    if _buf(dt, name) is not None and dt.numel() != K * 2 * g.M:
        raise ValueError(f"{name}: expected {K} x 2 x {g.M} values, got {dt.numel()}")
    return dt


def _thin(g: Geometry, device, count):
    """`count` image-shaped (thin) tensors in one allocation."""
    return torch.empty((count,) + g.image_shape(), device=device, dtype=torch.float32)


def _ptr_table(tensors):
    """Host array of device pointers (kept alive by the caller for the duration of the call)."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sweep_tables(K, keep, alloc_z, alloc_r, z_K=None):
    """The code and residual tables of a K-iteration forward or tangent sweep: (z, r), with z[k] the buffer iteration k
    writes and r[k - 1] the residual it reads.  keep: every entry gets a buffer of its own (training); otherwise two
    ping-pong buffers each, so consecutive entries never alias (the C side refuses zout == zin).  z_K: the last code's own
    tensor where the sweep keeps it apart from the internal codes (the fused tiers: other layout).  alloc_z / alloc_r(count):
    `count` code / thin buffers (one allocation, indexable); at least one is asked for even where none is used (K == 1)."""
    inner = K if z_K is None else K - 1
    nz = inner if keep else min(inner, 2)
    nr = (K - 1) if keep else min(K - 1, 2)
    zbuf, rbuf = alloc_z(max(nz, 1)), alloc_r(max(nr, 1))
    z = [zbuf[k % nz] for k in range(inner)] + ([] if z_K is None else [z_K])
    return z, [rbuf[k % nr] for k in range(K - 1)]


# ------------------------------------------------------------------------------------------ fused generic path
# cdl_fusedg.hip: the fused iteration for any C, 2-D / 3-D, unit stride, P in {3,5,7}, M <= 64 (BASELINE configs[2]
# and [3]), and -- behind the same entry points -- cdl_strip.hip: one image channel, stride 1 or 2, up to 192 subbands
# (the shipped CDLNet-s2030 architecture); same call structure as the 2-D flagship path above, codes in the
# reference's (N,M,[D,]H,W) layout.
def fusedg_supported(g: Geometry) -> bool:
    return bool(_size("cdl_fusedg_supported", g))


def _fusedg_sizes(g: Geometry):
    """(fragment bytes, patch floats, tiles, map words)."""
    return tuple(_size("cdl_fusedg_" + q, g) for q in ("frag_bytes", "patch_floats", "tiles", "map_words"))


def _fusedg_map_shape(g: Geometry):
    """(N, planes) + code dims.  The tile kernel (unit stride, M <= 64): 4 planes; the strip kernel (cdl_strip.hip): 4
    planes per PAIR of 32-channel tiles, on the code grid."""
    mw = _fusedg_sizes(g)[3]
    sp = tuple(d // st for d, st in zip(g.dims, g.stride))          # (Dz, Hz, Wz), leading 1 for 2-D
    per = 1
    for d in sp:
        per *= d
    return (g.N, mw // (g.N * per)) + sp


def fusedg_map(g: Geometry, device):
    return torch.empty(_fusedg_map_shape(g), device=device, dtype=torch.int32)


def fusedg_prep(g: Geometry, wA, wB):
    wA, wB = _dev(wA, "wA"), _dev(wB, "wB")
    frags = torch.empty(_fusedg_sizes(g)[0], device=wA.device, dtype=torch.uint8)
    _call("cdl_fusedg_prep", g, wA, wB, frags)
    return frags


def fusedg_patches(g: Geometry, device):
    return torch.empty(_fusedg_sizes(g)[1], device=device, dtype=torch.float32)


def _rsc_dims(g: Geometry):
    """(N, M, rows, Wz, strips): rows = code depth x code height (the layout blocks every code row of every depth)."""
    cs = g.code_shape()
    rows = 1
    for d in cs[2:-1]:
        rows *= d
    return cs[0], cs[1], rows, cs[-1], (cs[-1] + 31) // 32


def fusedg_rsc_buffer(g: Geometry, device, count=1):
    """Flat fp32 buffer(s) for code tensors in the strip kernels' row-strip channel-major layout ("rsc":
    [n][code depth][code row][ceil(Wz/32)][M][32 columns]; include/cdlnet_hip.h CDL_LAY_RSC)."""
    N, M, rows, wz, nsx = _rsc_dims(g)
    return torch.empty((count, N * M * rows * nsx * 32), device=device, dtype=torch.float32)


def fusedg_to_rsc(g: Geometry, z):
    """(N,M,[Dz,]Hz,Wz) -> flat rsc buffer (host-side plumbing for tests)."""
    N, M, rows, wz, nsx = _rsc_dims(g)
    zp = torch.zeros((N, M, rows, nsx * 32), device=z.device, dtype=torch.float32)
    zp[..., :wz] = z.reshape(N, M, rows, wz)
    return zp.reshape(N, M, rows, nsx, 32).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def fusedg_from_rsc(g: Geometry, buf):
    N, M, rows, wz, nsx = _rsc_dims(g)
    z = buf.reshape(N, rows, nsx, M, 32).permute(0, 3, 1, 2, 4).reshape(N, M, rows, nsx * 32)
    return z[..., :wz].contiguous().reshape(g.code_shape())


def fusedg_assemble(g: Geometry, patches, mask=None, sub=None, alpha=1.0, out=None, acc=None, acc_add=False,
                    write_out=True):
    """As fused_assemble (the optional unmasked sum into `acc` included)."""
    return _assemble("cdl_fusedg_assemble", g, patches, mask, sub, alpha, out, acc, acc_add, write_out)


def fusedg_support_map(g: Geometry, z):
    """Bit map of a code tensor in the layout the fused stages use: (N, 4 * pairs, code dims) words; channel
    32R + 8q + 4h + e is bit 16(R&1) + 4q + e of plane 4(R>>1) + 2h (support, [z != 0]) and of plane 4(R>>1) + 2h + 1
    (sign bit, set only where there is support) -- one plane quadruple per pair of 32-channel tiles (M <= 64: the 4 planes of the tile kernel).
    Host-side plumbing for tests."""
    z = _dev(z, "z")
    N, M = z.shape[:2]
    shape = _fusedg_map_shape(g)
    sp = shape[2:]
    zz = z.reshape((N, M) + sp)
    out = torch.zeros(shape, device=z.device, dtype=torch.int64)
    for ch in range(M):
        R, rem = divmod(ch, 32)
        q, rem = divmod(rem, 8)
        h, e = divmod(rem, 4)
        bit = 16 * (R & 1) + 4 * q + e
        pl = 4 * (R >> 1) + 2 * h
        nz = zz[:, ch] != 0
        out[:, pl] |= nz.to(torch.int64) << bit
        out[:, pl + 1] |= (torch.signbit(zz[:, ch]) & nz).to(torch.int64) << bit
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out)
    return out.to(torch.int32).contiguous()


def _plane_rows(g: Geometry, planes):
    """Threshold rows of one iteration on the fused generic tier: one per sample, or (planes) one per (sample, depth) plane."""
    return g.N * g.dims[0] if planes else g.N


def _plane_levels(g: Geometry, c, planes):
    """The levels c that weight dt[:,1]: (N), or (N*D) with per-plane thresholds (None stays None)."""
    if c is not None and c.numel() != _plane_rows(g, planes):
        raise ValueError(f"c: expected {_plane_rows(g, planes)} noise levels, got {c.numel()}")
    return c


def fusedg_dtau_reduce(g: Geometry, dtau_partial, c, dt_k, dtau_n=None, planes=False):
    """planes: the (sample, depth) plane is the "sample" -- c (N*D), dtau_n (N*D, M); dt_k[0] does not change."""
    if not planes:
        return _dtau_reduce("cdl_fusedg_dtau_reduce", g, dtau_partial, c, dt_k, dtau_n)
    dt0, dt1 = _dt_halves(g, dt_k)
    _call("cdl_fusedg_dtau_reduce_planes", g, _buf(dtau_partial, "dtau_partial"), _plane_levels(g, _opt(c, "c"), True), dt0, dt1,
          _buf(dtau_n, "dtau_n", (_plane_rows(g, True), g.M)))


def fusedg_code_layout(g: Geometry, training=True) -> str:
    """Layout the fused generic sweeps keep their internal codes in: "rsc" for the strip kernels' shapes (with
    `training`: when the matrix-core filter-gradient kernel takes the geometry, since its VALU fallbacks read the
    reference layout only), else "nchw" (cdl_fusedg_code_layout)."""
    code = _lib.lib().cdl_fusedg_code_layout(ctypes.byref(g.c_struct()), int(bool(training)))
    return "rsc" if int(code) == LAYOUT["rsc"] else "nchw"


def _fusedg_code_buffers(g: Geometry, layout, device, count):
    """`count` code tensors of a sweep: (N,M,..) tensors for "nchw", flat buffers for "rsc"."""
    if layout == "nchw":
        return list(torch.empty((max(count, 1),) + g.code_shape(), device=device, dtype=torch.float32).unbind(0))
    return list(fusedg_rsc_buffer(g, device, max(count, 1)).unbind(0))


# ------------------------------------------------------------------------------------------ sweeps of the two fused tiers
# What the wrappers of the two fused tiers differ in (the rest is one implementation per role, _fused_* below): the prefix of
# the entry points; code_buffers(g, layout, device, count) -> `count` indexable code buffers; to_nchw(g, t, layout) and
# support_map(g, z), which rebuild a bit map from a stored code; map_shape(g) of one bit map; frag_bytes(g) of one prepared
# pair, patch_floats(g), tiles(g) (rows of the stages' threshold partials); reverse_ws(g, device) -> the trailing workspace
# arguments of the reverse sweep (cdl_fusedg_backward's filter gradients are the shape-generic cdl_wgrad's).
# takes_map: the tier's entry points end in the noise-level map arguments (the 2-D tier's do: DESIGN.md section 31).
_FusedTier = collections.namedtuple(
    "_FusedTier", "prefix code_buffers to_nchw support_map map_shape frag_bytes patch_floats tiles reverse_ws takes_map")


def _fusedg_wgrad_workspace(g: Geometry, device):
    nws = _size("cdl_wgrad_workspace_floats", g)
    return _new((max(nws, 1),), device), nws


_FUSED2D = _FusedTier(
    prefix="cdl_fused2d", code_buffers=fused_code_buffer, to_nchw=fused_to_nchw, support_map=fused_support_map,
    map_shape=lambda g: (g.N, 4, g.dims[1], g.dims[2]), frag_bytes=lambda g: _lib.lib().cdl_fused2d_frag_bytes(g.M),
    patch_floats=lambda g: _size("cdl_fused2d_patch_floats", g), tiles=fused_tiles,
    reverse_ws=lambda g, device: (fused_wgrad_workspace(g, device),), takes_map=True)
_FUSEDG = _FusedTier(
    prefix="cdl_fusedg", code_buffers=_fusedg_code_buffers,
    to_nchw=lambda g, t, layout: t if layout == "nchw" else fusedg_from_rsc(g, t), support_map=fusedg_support_map,
    map_shape=_fusedg_map_shape, frag_bytes=lambda g: _size("cdl_fusedg_frag_bytes", g),
    patch_floats=lambda g: _size("cdl_fusedg_patch_floats", g), tiles=lambda g: _size("cdl_fusedg_tiles", g),
    reverse_ws=_fusedg_wgrad_workspace, takes_map=False)


def _tier_map(tier, g, cmap, tslope, rows=1, more=()):
    """The noise-level map arguments an entry point of `tier` ends in: (cmap, tslope) + more for the 2-D tier -- checked
    as on the generic tier, `rows` slope rows -- and none for the tile / strip kernels, which take no map."""
    cmap, tslope = _check_map_pair(g, cmap, tslope, rows)
    if tier.takes_map:
        return (cmap, tslope) + tuple(more)
    if cmap is not None or any(torch.is_tensor(m) for m in more):
        raise ValueError(f"{tier.prefix}: this tier takes no noise-level map (the generic sweeps do)")
    return ()


def _code(t, name, layout):
    """A code tensor stored in `layout` that a kernel reads (None stays None): checked like any input, except the flat
    pixel-blocked buffers of the fused 2-D sweeps (fp32 or bf16; K - 1 of them per reverse sweep), which `_call` checks."""
    return t if t is None or layout.startswith("blocked") else _dev(t, name)


def _fused_iter(tier, g, r, zin, tau, frags, sgn, patches, precision, out, map_out, lay_in, lay_out, cmap=None, tslope=None,
                planes=False):
    r, zin, tau = _dev(r, "r"), _code(zin, "zin", lay_in), _dev(tau, "tau")
    assert tuple(r.shape) == g.image_shape()
    if planes and tau.numel() != _plane_rows(g, True) * g.M:
        raise ValueError(f"tau: expected {_plane_rows(g, True)} x {g.M} per-plane thresholds, got {tau.numel()}")
    frags, patches = _buf(frags, "frags", dtype=torch.uint8), _buf(patches, "patches")
    mp = _tier_map(tier, g, cmap, tslope)
    if out is None:
        out = tier.code_buffers(g, lay_out, r.device, 1)[0]
    _call(tier.prefix + "_iter_fwd", g, r, zin, tau, frags, sgn, _buf(out, "out", dtype=out.dtype), patches,
          _buf(map_out, "map_out", dtype=torch.int32),
          PRECISION[precision] | _lay_in(lay_in) | _lay_out(lay_out) | (TAU_PER_PLANE if planes else 0), *mp)
    return out


def _dtau_partial_floats(tier, g, with_map):
    """Floats of a reverse stage's threshold partials: the library's own figure where the tier takes a map."""
    if tier.takes_map:
        return int(_lib.lib().cdl_fused2d_dtau_partial_floats(g._c_ref(), int(bool(with_map))))
    return tier.tiles(g) * g.M


def _map_partials(tier, g, dtau_partial, with_map):
    """A reverse stage's threshold partials: (tiles, M) floats, and with a noise-level map the weighted ones behind them."""
    n = _dtau_partial_floats(tier, g, with_map)
    if _buf(dtau_partial, "dtau_partial").numel() < n:
        raise ValueError(f"dtau_partial: {dtau_partial.numel()} floats, this stage writes {n}")
    return dtau_partial


def _fused_stage_bwd(tier, g, thin, base, gate_map, frags, patches, dtau_partial, do_synth, precision, out, lay_in, lay_out, rider=(),
                     cmap=None, tslope=None, dcmap=None, dcmap_add=False):
    """`rider`: the arguments an entry point takes between do_synth and the flags (cdl_fused2d_stage_bwd's dA_k)."""
    thin, base = _dev(thin, "thin"), _code(base, "base", lay_in)
    gate_map = _buf(gate_map, "gate_map", dtype=torch.int32)
    frags, patches = _buf(frags, "frags", dtype=torch.uint8), _buf(patches, "patches")
    _check_map(g, _buf(dcmap, "dcmap"))
    mp = _tier_map(tier, g, cmap, tslope, more=(dcmap, bool(dcmap_add)))
    if out is None:
        out = tier.code_buffers(g, lay_out, thin.device, 1)[0]
    _call(tier.prefix + "_stage_bwd", g, thin, base, gate_map, frags, _buf(out, "out", dtype=out.dtype), patches,
          _map_partials(tier, g, dtau_partial, cmap is not None), bool(do_synth), *rider,
          PRECISION[precision] | _lay_in(lay_in) | _lay_out(lay_out), *mp)
    return out


def _fused_forward(tier, g, yp, mask_p, tau, A, B, keep, precision, layout, keep_maps, cmap=None, tslope=None, planes=False):
    K = len(A)
    mp = _tier_map(tier, g, cmap, tslope, rows=K)
    yp, tau, mask_p = _dev(yp, "yp"), _dev(tau, "tau"), _opt(mask_p, "mask")
    if planes and tau.numel() != K * _plane_rows(g, True) * g.M:
        raise ValueError(f"tau: expected {K} x {_plane_rows(g, True)} x {g.M} per-plane thresholds, got {tau.numel()}")
    A, B = [_dev(w, "A") for w in A], [_dev(w, "B") for w in B]
    dev = yp.device
    # one allocation per family (views into it): at cfg1's size the allocator calls cost more than the kernels
    z, r = _sweep_tables(K, keep, lambda n: tier.code_buffers(g, layout, dev, n), lambda n: _thin(g, dev, n),
                         z_K=_new(g.code_shape(), dev))
    maps = list(torch.empty((K,) + tuple(tier.map_shape(g)), device=dev, dtype=torch.int32).unbind(0)) \
        if (keep or keep_maps) else []
    xp = _new(g.image_shape(), dev)
    frags = torch.empty(K * tier.frag_bytes(g), device=dev, dtype=torch.uint8)
    _call(tier.prefix + "_forward", g, K, yp, mask_p, tau, A, B, z, r, maps, xp, frags, _new((tier.patch_floats(g),), dev),
          PRECISION[precision] | _lay_in(layout) | (TAU_PER_PLANE if planes else 0), *mp)
    return xp, z[K - 1], (z if keep else [z[K - 1]]), (r if keep else []), maps


def _fused_tangent(tier, g, vp, mask_p, A, B, maps, keep, precision, layout, last):
    K = len(A)
    vp, mask_p = _dev(vp, "vp"), _opt(mask_p, "mask")
    A, B = [_dev(w, "A") for w in A], [_dev(w, "B") for w in B]
    assert len(maps) == K
    dev = vp.device
    nvp = torch.neg(vp)                                      # thin: the assemble subtracts it
    zd, nrd = _sweep_tables(K, keep, lambda n: tier.code_buffers(g, layout, dev, n), lambda n: _thin(g, dev, n),
                            z_K=_new(g.code_shape(), dev))
    xdp = _new(g.image_shape(), dev)
    frags = torch.empty(K * tier.frag_bytes(g), device=dev, dtype=torch.uint8)
    _call(tier.prefix + "_tangent", g, K, vp, nvp, mask_p, A, B, list(maps), zd, nrd, xdp, frags,
          _new((tier.patch_floats(g),), dev), _new((tier.tiles(g), g.M), dev), PRECISION[precision] | _lay_in(layout))
    return xdp, (zd if keep else ([zd[K - 1]] if last else [])), (nrd if keep else [])


def _fused_backward(tier, g, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, precision, maps, layout, dyp, dtau,
                    cmap=None, tslope=None, dcmap=None, planes=False):
    K = len(A)
    dev = yp.device
    _check_map(g, _buf(dcmap, "dcmap"))
    mp = _tier_map(tier, g, cmap, tslope, rows=K, more=(dcmap,))
    if cmap is not None and (c is not None or dtau is not None):
        raise ValueError("a noise-level map replaces the per-sample level c; its gradient is dcmap, not dtau")
    lay = lambda k: layout if k < K - 1 else "nchw"          # codes[-1] = z_K is always (N,M,..)
    if not maps:
        maps = [tier.support_map(g, tier.to_nchw(g, t, lay(k))) for k, t in enumerate(codes)]
    A, B = [_dev(w, "A") for w in A], [_dev(w, "B") for w in B]
    codes = [_code(t, "z", lay(k)) for k, t in enumerate(codes)]
    resid = [_dev(t, "r") for t in resid]
    if g_xp is None:
        g_xp = torch.zeros(g.image_shape(), device=dev, dtype=torch.float32)
    g_xp, g_z, c, mask_p = _dev(g_xp, "g_xp"), _opt(g_z, "g_z"), _opt(c, "c"), _opt(mask_p, "mask")
    if planes:
        _plane_levels(g, c, True)
    dt = _dt_sweep(g, K, dt)
    _check_data_grads(g, K, dyp, dtau, rows=_plane_rows(g, planes))
    dA, dB = _filter_grads(g, K, dev)
    du = tier.code_buffers(g, layout, dev, 2 if K > 1 else 1)
    frags = torch.empty(K * tier.frag_bytes(g), device=dev, dtype=torch.uint8)
    _call(tier.prefix + "_backward", g, K, yp, mask_p, c, A, B, codes, resid, list(maps), g_xp, g_z, dA, dB, dt, du[0],
          du[1 if K > 1 else 0], _new(g.image_shape(), dev), frags, _new((tier.patch_floats(g),), dev),
          _new((_dtau_partial_floats(tier, g, cmap is not None),), dev), *tier.reverse_ws(g, dev),
          PRECISION[precision] | _lay_in(layout) | (TAU_PER_PLANE if planes else 0), dyp, dtau, *mp)
    return dA, dB


def fused_iter(g: Geometry, r, zin, tau, frags, sgn, patches, precision="split3", out=None, map_out=None,
               lay_in="nchw", lay_out="nchw", *, cmap=None, tslope=None):
    """One fused iteration.  lay_in / lay_out: layouts of zin / the result (a flat buffer unless "nchw").
    cmap (N,1,H,W) with tslope (M): a noise-level map -- the threshold of element (n, m, pix) is
    tau[n,m] + cmap[n,pix] * tslope[m], as `analysis` forms it (split3, "nchw" / "blocked" only)."""
    return _fused_iter(_FUSED2D, g, r, zin, tau, frags, sgn, patches, precision, out, map_out, lay_in, lay_out, cmap, tslope)


def fusedg_iter(g: Geometry, r, zin, tau, frags, sgn, patches, out=None, map_out=None, lay_in="nchw", lay_out="nchw",
                precision="split3", planes=False):
    """precision: "split4" asks the tile kernel for its four-product instances; the strip kernels take "split3" only
    (CDL_EUNSUPPORTED otherwise).  planes: tau is (N*D, M), a threshold row per (sample, depth) plane (CDL_TAU_PER_PLANE)."""
    return _fused_iter(_FUSEDG, g, r, zin, tau, frags, sgn, patches, precision, out, map_out, lay_in, lay_out, planes=planes)


def fused_stage_bwd(g: Geometry, thin, base, gate, frags, patches, dtau_partial, do_synth,
                    precision="split3", out=None, lay_in="nchw", lay_out="nchw", r2=None, alpha=1.0, workspace=None, *,
                    cmap=None, tslope=None, dcmap=None, dcmap_add=False):
    """One reverse-sweep stage: du = [z' != 0] * (base + corr(thin; W1)); patches = W2^T du.  `gate` is the
    bit map of z' (int32, from the forward or fused_support_map) or z' itself (the map is built first).
    With `r2` (thin) and `workspace` (fused_wgrad_workspace) the launch also accumulates dA = alpha * du (x) im2col(r2)
    and (du, dA) is returned.
    cmap / tslope: the forward's noise-level map -- `dtau_partial` is then (2 * fused_tiles(g), M), the map-weighted
    partials behind the plain ones (fused_dtau_reduce's `weighted`); dcmap (N,1,H,W): this iteration's dL/dcmap, written
    or (dcmap_add) added."""
    if gate.dtype != torch.int32:
        gate = fused_support_map(g, gate)
    assert gate.numel() == g.N * 4 * g.dims[1] * g.dims[2]
    r2 = _opt(r2, "r2")
    dA = None if r2 is None else torch.empty(g.filter_shape(), device=thin.device, dtype=torch.float32)
    out = _fused_stage_bwd(_FUSED2D, g, thin, base, gate, frags, patches, dtau_partial, do_synth, precision, out, lay_in,
                           lay_out, rider=(r2, alpha, dA, _buf(workspace, "workspace")), cmap=cmap, tslope=tslope,
                           dcmap=dcmap, dcmap_add=dcmap_add)
    return out if dA is None else (out, dA)


def fusedg_stage_bwd(g: Geometry, thin, base, gate_map, frags, patches, dtau_partial, do_synth, out=None,
                     lay_in="nchw", lay_out="nchw", precision="split3"):
    return _fused_stage_bwd(_FUSEDG, g, thin, base, gate_map, frags, patches, dtau_partial, do_synth, precision, out, lay_in, lay_out)


def fused_forward(g: Geometry, yp, mask_p, tau, A, B, keep, precision="split3", layout="blocked", keep_maps=False, *,
                  cmap=None, tslope=None):
    """Whole forward sweep in one C call.  keep=True: every z_k and r_k gets its own buffer (training) and
    each launch also writes the support/sign bit map of its z_{k+1}; keep=False: two ping-pong buffers
    each, no maps.  `layout`: how z_1..z_{K-1} are stored (they never leave the sweeps; z_K is always NCHW).
    keep_maps (with keep=False): the K bit maps are written although every code and residual ping-pongs (what a tangent
    sweep under no_grad needs of the primal).
    cmap (N,1,H,W) with tslope (K,M): a noise-level map, tau then holding t[k,0,m] for every sample (as ista_forward's).
    Returns (xp, z_K, codes, resid, maps); codes[:-1] are flat buffers in `layout` unless it is "nchw"."""
    return _fused_forward(_FUSED2D, g, yp, mask_p, tau, A, B, keep, precision, layout, keep_maps, cmap, tslope)


def fusedg_forward(g: Geometry, yp, mask_p, tau, A, B, keep, layout="nchw", keep_maps=False, planes=False):
    """Whole forward sweep in one C call (cdl_fusedg_forward); same contract as fused_forward: codes[:-1] come back
    in `layout` ("nchw", or "rsc" where fusedg_code_layout allows it), codes[-1] = z_K as (N,M,..).  planes: tau is
    (K, N*D, M), a threshold row per (sample, depth) plane (CDL_TAU_PER_PLANE: one noise level per frame)."""
    return _fused_forward(_FUSEDG, g, yp, mask_p, tau, A, B, keep, "split3", layout, keep_maps, planes=planes)


def fused_backward(g: Geometry, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, precision="split3", maps=None,
                   layout="blocked", dyp=None, dtau=None, *, cmap=None, tslope=None, dcmap=None):
    """Whole reverse sweep in one C call; returns (dA list, dB list); dt (K,2,M) is written in place.
    cmap / tslope (K,M): the forward's noise-level map in place of c (then None, as dtau); dcmap (N,1,H,W, nullable)
    receives dL/dcmap.
    maps: the forward's bit maps of z_1..z_K (built here from the codes when not given).  `layout`: that of
    codes[:-1] (as fused_forward returned them) and of the du work buffers; codes[-1] = z_K, g_z: NCHW.
    g_xp None (a loss on the code only) is a zero image gradient.  dyp (thin, as yp) / dtau (K,N,M): filled with
    dL/dyp and the per-image threshold gradients when given (cdl_fused2d_backward; None: the plain sweep)."""
    return _fused_backward(_FUSED2D, g, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, precision, maps, layout, dyp, dtau,
                           cmap, tslope, dcmap)


def fusedg_backward(g: Geometry, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, layout="nchw",
                    dyp=None, dtau=None, planes=False):
    """Whole reverse sweep in one C call (cdl_fusedg_backward); returns (dA list, dB list), fills dt (K,2,M) [and
    dyp, dtau: see fused_backward].  `layout`: that of codes[:-1] (and of the du buffers allocated here).  planes: the
    forward ran with per-plane thresholds -- c is (N*D) and dtau (K, N*D, M)."""
    return _fused_backward(_FUSEDG, g, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, "split3", maps, layout, dyp, dtau,
                           planes=planes)


def fused_tangent(g: Geometry, vp, mask_p, A, B, maps, keep, precision="split3", layout="blocked", last=False):
    """Tangent sweep on the fused 2-D kernels in one C call (cdl_fused2d_tangent).  maps: the primal's
    K bit maps.  Returns (xdp, zd, nrd): with keep the tangent codes (zd[:-1] in `layout`, zd[-1] NCHW) and the NEGATED
    tangent residuals -rd_1..-rd_{K-1} (what the stages read), else [] (with `last`, zd = [zd_K] when nothing is kept)."""
    return _fused_tangent(_FUSED2D, g, vp, mask_p, A, B, maps, keep, precision, layout, last)


def fusedg_tangent(g: Geometry, vp, mask_p, A, B, maps, keep, last=False):
    """cdl_fusedg_tangent: as fused_tangent for the tile / strip kernels' shapes; codes in the reference's layout."""
    return _fused_tangent(_FUSEDG, g, vp, mask_p, A, B, maps, keep, "split3", "nchw", last)


# ------------------------------------------------------------------------------------------
# whole sweeps of the shape-generic loop (cdl_sweep.hip)
def _new(shape, device):
    return torch.empty(shape, device=device, dtype=torch.float32)


def ista_scratch(g: Geometry, device):
    n = _size("cdl_ista_scratch_floats", g)
    return _scratch(device, max(n, 1)), n


def _generic_tables(g: Geometry, K, keep, device):
    """_sweep_tables of the generic tier: all K codes in the reference's layout, one allocation per family."""
    return _sweep_tables(K, keep, lambda n: _new((n,) + g.code_shape(), device), lambda n: _thin(g, device, n))


def ista_forward(g: Geometry, yp, mask_p, tau, A, B, keep, z_prev=None, z_after=None, gam1=None, gam2=None, *,
                 cmap=None, tslope=None):
    """Generic forward sweep in one C call.  Plain ST loop (z_prev None) or the CSR maps.  keep=True:
    every z_k, r_k (and u_k for CSR) gets its own buffer.  Returns (xp, z_K, codes, resid, us).
    cmap (N,1,*code_spatial) with tslope (K,M) = t[:,1]: noise-level map, see analysis; with z_prev tslope is (K,3,M),
    the slopes of lam, gam1, gam2, and tau / gam1 / gam2 hold the constant parts (analysis_prox)."""
    K = len(A)
    cmap, tslope = _check_map_pair(g, cmap, tslope, K if z_prev is None else 3 * K)
    yp, tau, mask_p = _dev(yp, "yp"), _dev(tau, "tau"), _opt(mask_p, "mask")
    A = [_dev(w, "A") for w in A]
    B = [_dev(w, "B") for w in B]
    z_prev, z_after = _opt(z_prev, "z_prev"), _opt(z_after, "z_after")
    gam1, gam2 = _opt(gam1, "gam1"), _opt(gam2, "gam2")
    dev = yp.device
    z, r = _generic_tables(g, K, keep, dev)
    u = list(_new((K,) + g.code_shape(), dev).unbind(0)) if (keep and z_prev is not None) else []
    xp = _new(g.image_shape(), dev)
    ws, n = ista_scratch(g, dev)
    _call("cdl_ista_forward", g, K, yp, mask_p, tau, z_prev, z_after, gam1, gam2, A, B, z, r, u, xp, ws, n, cmap, tslope)
    return xp, z[K - 1], (z if keep else [z[K - 1]]), (r if keep else []), u


def ista_backward(g: Geometry, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, us=None, z_prev=None,
                  z_after=None, lam=None, gam1=None, gam2=None, dg1=None, dg2=None, gz_prev=None, gz_after=None,
                  dyp=None, dtau=None, *, cmap=None, tslope=None, dcmap=None):
    """Generic reverse sweep in one C call (cdl_ista_backward); returns (dA, dB) and fills dt [, dg1, dg2, gz_prev,
    gz_after] [, dyp, dtau: see fused_backward; with z_prev dtau is (K,3,N,M), the per-sample sums of lam, gam1, gam2].
    cmap / tslope as ista_forward's (c is then None); dcmap (N,1,*code_spatial; nullable) receives dL/dcmap where dtau
    would be returned."""
    K = len(A)
    dt, dg1, dg2 = _dt_sweep(g, K, dt), _dt_sweep(g, K, dg1, "dg1"), _dt_sweep(g, K, dg2, "dg2")
    gz_prev, gz_after = _buf(gz_prev, "gz_prev", g.code_shape()), _buf(gz_after, "gz_after", g.code_shape())
    _check_data_grads(g, K, dyp, dtau, 1 if z_prev is None else 3)
    cmap, tslope = _opt(cmap, "cmap"), _opt(tslope, "tslope")
    _check_map(g, cmap, tslope, K if z_prev is None else 3 * K)
    if _buf(dcmap, "dcmap") is not None:
        if cmap is None or tslope is None:
            raise ValueError("dcmap: there is no cmap / tslope to take the gradient of")
        _check_map(g, dcmap)
    dev = yp.device
    A = [_dev(w, "A") for w in A]
    B = [_dev(w, "B") for w in B]
    dA, dB = _filter_grads(g, K, dev)
    g0, g1, q = _new(g.code_shape(), dev), _new(g.code_shape(), dev), _new(g.image_shape(), dev)
    ws, n = ista_scratch(g, dev)
    _call("cdl_ista_backward", g, K, _dev(yp, "yp"), _opt(mask_p, "mask"), _opt(c, "c"), _opt(z_prev, "z_prev"),
          _opt(z_after, "z_after"), _opt(lam, "lam"), _opt(gam1, "gam1"), _opt(gam2, "gam2"), A, B,
          [_dev(t, "z") for t in codes], [_dev(t, "r") for t in resid], [_dev(t, "u") for t in us or ()],
          _opt(g_xp, "g_xp"), _opt(g_z, "g_z"), dA, dB, dt, dg1, dg2, gz_prev, gz_after, g0, g1, q, ws, n, dyp, dtau,
          cmap, tslope, dcmap)
    return dA, dB


# ------------------------------------------------------------------------------------------
# forward-mode tangent sweeps at the primal's supports
def tangent_forward(g: Geometry, vp, mask_p, A, B, gates, keep, last=False):
    """Generic tangent sweep in one C call (cdl_tangent_forward): gates = the primal's z_1..z_K (N,M,..); vp the
    pre-processed direction.  Returns (xdp, zd, rd): with keep the K tangent codes and K-1 tangent residuals, else [] (with
    `last`, zd = [zd_K] when nothing is kept: the last code of the ping-pong table)."""
    K = len(A)
    vp, mask_p = _dev(vp, "vp"), _opt(mask_p, "mask")
    A = [_dev(w, "A") for w in A]
    B = [_dev(w, "B") for w in B]
    gates = [_dev(t, "gate") for t in gates]
    assert len(gates) == K and all(tuple(t.shape) == g.code_shape() for t in gates)
    dev = vp.device
    zd, rd = _generic_tables(g, K, keep, dev)
    xdp = _new(g.image_shape(), dev)
    ws, n = ista_scratch(g, dev)
    _call("cdl_tangent_forward", g, K, vp, mask_p, A, B, gates, zd, rd, xdp, _new((2 * g.M,), dev), ws, n)
    return xdp, (zd if keep else ([zd[K - 1]] if last else [])), (rd if keep else [])


def tangent_backward(g: Geometry, vp, mask_p, A, B, gates, zd, rd, g_xp, g_zd=None):
    """Reverse sweep of the generic tangent sweep in one C call (cdl_tangent_backward): (dA list, dB list) for
    dL/dxdp = g_xp [and dL/dzd_K = g_zd]; gates = the primal's codes, zd / rd = what tangent_forward kept."""
    K = len(A)
    dev = vp.device
    A = [_dev(w, "A") for w in A]
    B = [_dev(w, "B") for w in B]
    gates = [_dev(t, "gate") for t in gates]
    zd = [_dev(t, "zd") for t in zd]
    rd = [_dev(t, "rd") for t in rd]
    assert len(gates) == K == len(zd) and len(rd) == K - 1
    dA, dB = _filter_grads(g, K, dev)
    g0, g1, q = _new(g.code_shape(), dev), _new(g.code_shape(), dev), _new(g.image_shape(), dev)
    ws, n = ista_scratch(g, dev)
    _call("cdl_tangent_backward", g, K, _dev(vp, "vp"), _opt(mask_p, "mask"), A, B, gates, zd, rd, _dev(g_xp, "g_xp"),
          _opt(g_zd, "g_zd"), dA, dB, g0, g1, q, _new((2 * g.M,), dev), ws, n)
    return dA, dB


def csr_tangent_forward(g: Geometry, vp, mask_p, lam, gam1, gam2, z_prev, z_after, zd_prev, zd_after, A, B, us, keep, *,
                        cmap=None, tslope=None):
    """Tangent sweep of the CSR loop in one C call (cdl_csr_tangent_forward): us = the primal's u_0..u_{K-1} (its gates, with
    z_prev / z_after and the primal's lam / gam* (K,N,M)); zd_prev / zd_after (nullable) the neighbours' tangents.  Returns
    (xdp, zd_K, zd, rd): with keep the K tangent codes and K-1 tangent residuals, else [].
    cmap (N,1,*code_spatial) with tslope (K,3,M): the primal's noise-level map (ista_forward), lam / gam* the constant parts."""
    K = len(A)
    cmap, tslope = _check_map_pair(g, cmap, tslope, 3 * K)
    vp, mask_p = _dev(vp, "vp"), _opt(mask_p, "mask")
    A = [_dev(w, "A") for w in A]
    B = [_dev(w, "B") for w in B]
    us = [_dev(t, "u") for t in us]
    z_prev, z_after = _dev(z_prev, "z_prev"), _opt(z_after, "z_after")
    zd_prev, zd_after = _opt(zd_prev, "zd_prev"), _opt(zd_after, "zd_after")
    assert len(us) == K
    _check_codes(g, z_prev=z_prev, z_after=z_after, zd_prev=zd_prev, zd_after=zd_after, **{f"u[{k}]": t for k, t in enumerate(us)})
    dev = vp.device
    zd, rd = _generic_tables(g, K, keep, dev)
    xdp = _new(g.image_shape(), dev)
    ws, n = ista_scratch(g, dev)
    _call("cdl_csr_tangent_forward", g, K, vp, mask_p, z_prev, z_after, _dev(lam, "lam"), _dev(gam1, "gam1"),
          _opt(gam2, "gam2"), zd_prev, zd_after, A, B, us, zd, rd, xdp, ws, n, cmap, tslope)
    return xdp, zd[K - 1], (zd if keep else []), (rd if keep else [])


def fused_timing(enable: bool):
    """Start / stop the HIP-event timing of the fused sweeps' fat kernels (cdl_fused2d_timing)."""
    _lib.check(_lib.lib().cdl_fused2d_timing(1 if enable else 0), "cdl_fused2d_timing")


def fused_timing_read():
    """{class: (average ms, launches)} for the forward stage, reverse stage and filter-gradient launches
    recorded since fused_timing(True)."""
    ms = (ctypes.c_double * 4)()
    cnt = (ctypes.c_int * 4)()
    _lib.check(_lib.lib().cdl_fused2d_timing_read(ms, cnt), "cdl_fused2d_timing_read")
    names = ("stage_fwd", "stage_bwd", "wgrad", "stage_first")
    return {n: ((ms[i] / cnt[i]) if cnt[i] else 0.0, int(cnt[i])) for i, n in enumerate(names)}


# every public wrapper runs with its tensors' device current (see _on_tensor_device)
for _name, _obj in list(globals().items()):
    if callable(_obj) and not _name.startswith("_") and getattr(_obj, "__module__", None) == __name__ \
            and not isinstance(_obj, type):
        globals()[_name] = _on_tensor_device(_obj)
del _name, _obj
