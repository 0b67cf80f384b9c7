"""Windowed inference: frames and clips larger than one fused sweep.

Every fused tier addresses one sample's code tensor through a buffer descriptor and refuses a geometry whose codes reach
2^31 bytes per sample; past it `net(y)` runs the three-launch tier.  `denoise(net, y, ...)` pre-processes the whole frame
once (its mean, its reflect padding), cuts the pre-processed frame into overlapping windows, runs them -- stacked along
the batch axis -- through the sweep of the tier their geometry takes (loop.run_windows) and puts the results together.

The fact it rests on: the unrolled loop is a fixed-depth stack of zero-padded convolutions, so xhat at image pixel i
depends on yp only within R = 2 K (P // 2) pixels along each axis, whatever the stride.  A window that carries a halo of R
(rounded up to the stride) around its core, or ends at the frame border, reproduces the untiled result on its core up to
the summation order of the kernels.

The planner (plan_axis, plan_windows) is pure host code and deterministic:
  * one axis of padded length L, core c, halo h (all multiples of the stride): cores [0,c), [c,2c), .. partition the
    axis (the last one may be shorter); every window has extent min(c + 2h, L) and starts at its core's start minus h,
    shifted inward at the two ends -- so all windows of a plan share one shape, and every core keeps at least h of halo
    on each side that is not a frame border;
  * window=None: one window if a fused tier takes the whole padded sample.  Otherwise the axes are tried in the order
    depth, height, width (auto_cores):
      1. one axis alone, the others whole: its largest core whose window (core + 2 halo) a fused tier accepts for one
         sample (largest_core).  The first axis whose largest core is at least twice its halo is cut -- it then sweeps
         at most twice its pixels -- and the search ends;
      2. failing that, the first axis that has an accepted core at all;
      3. failing that, several axes, in the same order: an axis that does not settle it is left at a core of twice
         its halo and the next axis is cut as well;
      4. failing that, the largest core common to every axis that has room.
    The cores of the axis cut last (1 to 3) are equalised: the same number of windows, core = ceil(L / count) rounded up to the
    stride -- on the last axis to 32 code pixels where the largest core allows.  An axis whose halo leaves no room
    (c + 2h >= L for every c) stays whole.  A net no fused tier takes at any size gets one window: the route of net(y).

The gather and the assembly move thin tensors (1/M of a sweep's traffic) with torch slicing.
"""
import itertools
from dataclasses import dataclass
from typing import Tuple

import torch

from . import loop, ops
from .net import CDLNet_CSR, CDLNet_CSRf2, _code_grid, _ISTANet, _mask_tensor, _noise_scale

__all__ = ["AxisWindow", "Plan", "plan_axis", "plan_windows", "exact_halo", "fused_accepts", "largest_core", "auto_cores",
           "denoise"]

BATCH_CODE_BYTES = 1 << 31      # default max_batch: the stacked windows' code tensor stays below this many bytes


@dataclass(frozen=True)
class AxisWindow:
    """One window along one axis: it reads [w0, w1) of the padded frame and owns the core [c0, c1)."""
    w0: int
    w1: int
    c0: int
    c1: int


def plan_axis(length, core, halo, s=1):
    """The windows of one axis of padded extent `length`: cores of `core` pixels (None: the whole axis) with `halo` pixels
    on each side; all three multiples of the stride `s`.  See the module docstring for the rule."""
    L, h = int(length), int(halo)
    c = L if core is None else int(core)
    if L <= 0 or L % s:
        raise ValueError(f"axis extent {L} is not a positive multiple of the stride {s}")
    if c <= 0 or c % s:
        raise ValueError(f"window core {c} is not a positive multiple of the stride {s}")
    if h < 0 or h % s:
        raise ValueError(f"halo {h} is not a non-negative multiple of the stride {s}")
    W = min(c + 2 * h, L)
    if W == L:                                         # every window would be the whole axis
        return (AxisWindow(0, L, 0, L),)
    out = []
    for c0 in range(0, L, c):
        w0 = min(max(c0 - h, 0), L - W)
        out.append(AxisWindow(w0, w0 + W, c0, min(c0 + c, L)))
    return tuple(out)


def _fade_zones(axis):
    """[a, b) between neighbouring windows i and i + 1 of one axis: their overlap, clipped to the span between the centres of
    the two cores (so that the zones of an axis never meet); empty overlap: the core boundary."""
    mid = [(w.c0 + w.c1) // 2 for w in axis]
    zones = []
    for i in range(len(axis) - 1):
        a, b = max(axis[i + 1].w0, mid[i]), min(axis[i].w1, mid[i + 1])
        if a >= b:
            a = b = axis[i].c1
        zones.append((a, b))
    return zones


def _join(pieces, axis, dim, blend):
    """The windows of one axis (piece i spans [w0_i, w1_i) along `dim`) as one tensor spanning the axis.  "crop": each
    core from its window.  "ramp": window i alone between the fade zones, and across zone i the linear cross-fade
    out + u (piece_{i+1} - out), u = (j + 1) / (len + 1) at the zone's j-th pixel: weights 1 - u and u, which sum to
    one, and equal inputs come through bit for bit."""
    if len(axis) == 1:
        return pieces[0]
    shape = list(pieces[0].shape)
    shape[dim] = axis[-1].w1
    out = pieces[0].new_empty(shape)
    if blend == "crop":
        for w, p in zip(axis, pieces):
            out.narrow(dim, w.c0, w.c1 - w.c0).copy_(p.narrow(dim, w.c0 - w.w0, w.c1 - w.c0))
        return out
    zones = _fade_zones(axis)
    ends = [b for _, b in zones] + [axis[-1].w1]
    out.narrow(dim, 0, ends[0]).copy_(pieces[0].narrow(dim, 0, ends[0]))
    for i in range(1, len(axis)):
        w, p = axis[i], pieces[i]
        a, b = zones[i - 1]
        if b > a:
            view = [1] * len(shape)
            view[dim] = b - a
            u = (torch.arange(1, b - a + 1, device=out.device, dtype=out.dtype) / (b - a + 1)).reshape(view)
            old = out.narrow(dim, a, b - a)
            old.add_(u * (p.narrow(dim, a - w.w0, b - a) - old))
        out.narrow(dim, b, ends[i] - b).copy_(p.narrow(dim, b - w.w0, ends[i] - b))
    return out


@dataclass(frozen=True)
class Plan:
    """The windows of a padded frame: per axis its AxisWindows; `windows` lists their index tuples, first axis slowest."""
    dims: Tuple[int, ...]
    s: int
    axes: Tuple[Tuple[AxisWindow, ...], ...]
    halo: Tuple[int, ...]

    @property
    def windows(self):
        return list(itertools.product(*(range(len(a)) for a in self.axes)))

    @property
    def shape(self):
        """Extent of every window."""
        return tuple(a[0].w1 - a[0].w0 for a in self.axes)

    @property
    def counts(self):
        return tuple(len(a) for a in self.axes)

    @property
    def cores(self):
        return tuple(a[0].c1 - a[0].c0 for a in self.axes)

    @property
    def overhead(self):
        """Pixels swept over pixels of the frame: prod((core + 2 halo) / core) away from the borders."""
        swept = frame = 1
        for a, d in zip(self.axes, self.dims):
            swept *= len(a) * (a[0].w1 - a[0].w0)
            frame *= d
        return swept / frame

    def describe(self):
        return {"dims": list(self.dims), "stride": self.s, "window": list(self.shape), "cores": list(self.cores),
                "halo": list(self.halo), "counts": list(self.counts), "overhead": round(self.overhead, 4)}

    def slices(self, w, scale=1):
        idx = self.windows[w] if isinstance(w, int) else w
        return tuple(slice(a[i].w0 // scale, a[i].w1 // scale) for a, i in zip(self.axes, idx))

    def gather(self, x, pairs, scale=1):
        """The (window, sample) `pairs` of x (N, C, *dims / scale) stacked along the batch axis.  An axis on which x has
        extent 1 is kept whole: per-frame noise levels (N,1,D,1,1) are cropped along depth only."""
        wins = self.windows

        def cut(w):
            return tuple(slice(None) if e == 1 else sl for e, sl in zip(x.shape[2:], self.slices(wins[w], scale)))
        return torch.cat([x[(slice(n, n + 1), slice(None)) + cut(w)] for w, n in pairs], 0).contiguous()

    def assemble(self, outs, blend="crop"):
        """outs[w] (N, C, *window shape), in the order of `windows`, put together as (N, C, *dims): one axis after the
        other, the last one first (_join), so the weights of a pixel are the product of its per-axis weights."""
        if blend not in ("crop", "ramp"):
            raise ValueError(f"blend must be 'crop' or 'ramp', not {blend!r}")
        cur = dict(zip(self.windows, outs))
        for a in reversed(range(len(self.axes))):
            cur = {key: _join([cur[key + (i,)] for i in range(len(self.axes[a]))], self.axes[a], 2 + a, blend)
                   for key in {k[:a] for k in cur}}
        return cur[()]


def plan_windows(dims, s, cores, halo):
    """The plan of a padded frame of extents `dims` for the given per-axis cores (None: whole axis) and halos."""
    dims = tuple(int(d) for d in dims)
    return Plan(dims, int(s), tuple(plan_axis(d, c, h, s) for d, c, h in zip(dims, cores, halo)),
                tuple(int(h) for h in halo))


def _round_up(v, m):
    return -(-int(v) // m) * m


def exact_halo(K, P, s):
    """R = 2 K (P // 2) per axis, rounded up to a multiple of the stride."""
    return tuple(_round_up(2 * int(K) * (int(p) // 2), s) for p in P)


def fused_accepts(C, M, P, s):
    """accepts(extents): does a fused tier take ONE sample of these padded extents?  (Host functions of the library.)"""
    pad = tuple(p // 2 for p in P)

    def accepts(ext):
        g = ops.Geometry.make(1, C, M, tuple(ext), P, pad, [s] * len(P))
        return ops.fused_supported(g) or ops.fusedg_supported(g)
    return accepts


def largest_core(dims, s, halo, accepts, axis, cores):
    """The largest core of `axis` whose window -- the other axes as `cores` says (None: whole) -- a fused tier accepts,
    equalised over its windows; None when the halo leaves no room to cut the axis or even a core of one stride is
    refused.  (Acceptance is monotone in the extent: a bisection.)"""
    nd, L, h = len(dims), dims[axis], halo[axis]
    if s + 2 * h >= L:
        return None

    def window(c):
        ext = [dims[b] if cores[b] is None else min(dims[b], cores[b] + 2 * halo[b]) for b in range(nd)]
        ext[axis] = c + 2 * h
        return tuple(ext)

    lo, hi = 1, (L - 2 * h - 1) // s                   # cores k * s with k * s + 2h < L
    if not accepts(window(s)):
        return None
    while lo < hi:
        k = (lo + hi + 1) // 2
        lo, hi = (k, hi) if accepts(window(k * s)) else (lo, k - 1)
    cmax = lo * s
    count = -(-L // cmax)
    even = _round_up(-(-L // count), s)
    if axis == nd - 1 and _round_up(even, 32 * s) <= cmax:
        even = _round_up(even, 32 * s)
    return even


def auto_cores(dims, s, halo, accepts):
    """The automatic plan's cores (module docstring): a tuple with None for an axis left whole."""
    dims = tuple(int(d) for d in dims)
    nd = len(dims)
    whole = (None,) * nd
    if accepts(dims):
        return whole
    if not accepts(tuple(min(d, s + 2 * h) for d, h in zip(dims, halo))):      # no fused tier takes this net at any size
        return whole
    alone = [largest_core(dims, s, halo, accepts, a, whole) for a in range(nd)]
    for ok in (lambda a: alone[a] is not None and alone[a] >= 2 * halo[a], lambda a: alone[a] is not None):
        for a in range(nd):
            if ok(a):
                return whole[:a] + (alone[a],) + whole[a + 1:]
    cores = [None] * nd
    for a in range(nd):
        c = largest_core(dims, s, halo, accepts, a, cores)
        if c is not None:
            cores[a] = c
            return tuple(cores)
        floor = max(s, _round_up(2 * halo[a], s))
        if floor + 2 * halo[a] < dims[a]:
            cores[a] = floor
    common = lambda k: tuple(k * s if k * s + 2 * h < d else None for d, h in zip(dims, halo))
    window = lambda k: tuple(d if c is None else c + 2 * h for d, h, c in zip(dims, halo, common(k)))
    lo, hi = 1, max(dims) // s                         # k = 1 is the smallest window, which is accepted
    while lo < hi:
        k = (lo + hi + 1) // 2
        lo, hi = (k, hi) if accepts(window(k)) else (lo, k - 1)
    return common(lo)


def _per_axis(value, nd, name, allow_none):
    if isinstance(value, (tuple, list)):
        vals = tuple(value)
        if len(vals) != nd:
            raise ValueError(f"{name} has {len(vals)} entries; this net has {nd} spatial axes")
    else:
        vals = (value,) * nd
    for v in vals:
        if v is None and allow_none:
            continue
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name}: {v!r} is not an int" + (" or None" if allow_none else ""))
    return vals


def _refusal(net):
    if isinstance(net, (CDLNet_CSR, CDLNet_CSRf2)):
        return (f"{type(net).__name__}: the codes of a CSR net travel from frame to frame, and a window's codes are not the "
                "frame's")
    if getattr(net, "residual", False):
        return "residual=True: the ResidualBlocks run outside the sweeps of loop.run"
    if not isinstance(net, _ISTANet):
        return f"{type(net).__name__} is not a net of this package"
    return None


def denoise(net, y, sigma=None, mask=1, *, window=None, halo="exact", blend="crop", max_batch=None):
    """xhat of `net(y, sigma, mask)` computed window by window, for frames and clips whose codes no fused sweep can hold.

    net       CDLNet (JDD: C = 3 with a mask), GDLNet or CDLNetVideo(residual=False).
    sigma     every form net(y, sigma) takes; a map is classified on the whole code grid and cropped per window (those
              windows take the tier a map takes in net(y): the generic one, or under loop.set_map_tier("fused") the map
              forms of the fused 2-D kernels where the window's geometry has them).
    mask      1 or a tensor shaped like y; pre-processed with the frame, cropped per window.
    window    core extent per spatial axis: an int or a tuple (None in a slot: the whole axis), multiples of the stride.
              None plans automatically (module docstring); a frame a fused tier takes whole is one window, and the
              result is then bit for bit net(y)[0].
    halo      "exact": R = 2 K (P // 2) per axis, rounded up to the stride -- the result is the untiled one up to the
              kernels' summation order.  An int or a tuple (multiples of the stride): an approximate run, e.g. the
              temporal axis of a clip, whose exact halo exceeds any clip.
    blend     "crop" keeps each window's core; "ramp" cross-fades linearly across the overlap of neighbouring windows
              (for approximate halos).
    max_batch cap on the (sample, window) pairs stacked into one sweep; None: as many as keep the stacked code tensor
              below 2 GiB and the windows on their tier.

    Returns xhat only.  Inference only: refused in grad mode when an input or a parameter requires grad."""
    name = "cdlnet_video_amd: denoise_windowed"
    why = _refusal(net)
    if why is not None:
        raise NotImplementedError(f"{name}: {why}")
    if not torch.is_tensor(y) or y.dim() not in (4, 5):
        raise ValueError(f"{name}: y must be (N,C,H,W) or (N,C,D,H,W)")
    nd, s, N = y.dim() - 2, int(net.s), y.shape[0]
    P = (int(net.P),) * nd if isinstance(net.P, int) else tuple(int(p) for p in net.P)
    if len(P) != nd:
        raise ValueError(f"{name}: y has {nd} spatial axes, the net's filters {len(P)}")
    if blend not in ("crop", "ramp"):
        raise ValueError(f"{name}: blend must be 'crop' or 'ramp', not {blend!r}")
    if max_batch is not None and (isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1):
        raise ValueError(f"{name}: max_batch must be a positive int or None")
    dims = tuple(int(d) + sum(ops.split_pad(int(d), s)) for d in y.shape[2:])
    if isinstance(halo, str) and halo != "exact":
        raise ValueError(f"{name}: halo must be 'exact', an int or a tuple, not {halo!r}")
    halos = exact_halo(net.K, P, s) if isinstance(halo, str) else _per_axis(halo, nd, "halo", False)
    accepts = fused_accepts(y.shape[1], int(net.M), P, s)
    cores = auto_cores(dims, s, halos, accepts) if window is None else _per_axis(window, nd, "window", True)
    plan = plan_windows(dims, s, cores, halos)          # refuses cores / halos that are not multiples of the stride
    if torch.is_grad_enabled():
        for label, v in (("y", y), ("sigma", sigma), ("mask", mask)):
            if torch.is_tensor(v) and v.requires_grad:
                raise NotImplementedError(f"{name}: `{label}` requires grad; windowed inference builds no graph "
                                          "(detach() it, or call net(y))")
        if any(p.requires_grad for p in net.parameters()):
            raise NotImplementedError(f"{name}: the net's parameters require grad; windowed inference builds no graph -- "
                                      "call it under torch.no_grad()")
    if not y.is_cuda:
        raise RuntimeError(
            f"{type(net).__name__}.forward: input is on {y.device}. This package has no CPU "
            "compute path; the iterations run in HIP kernels on a ROCm device.")
    with torch.no_grad():
        y = y.to(torch.float32)
        A, B = net._filters()
        c = _noise_scale(sigma, net.adaptive, N, y.device, _code_grid(y.shape[2:], s))
        if max_batch is None:
            max_batch = _default_batch(plan, y.shape[1], int(net.M), P, s, N)
        yp, mean, pads, mask_p = ops.preprocess(y, s, _mask_tensor(mask, y))
        xp = loop.run_windows(yp, mask_p, c, net.t, A, B, s, plan, blend=blend, max_batch=max_batch)
        return ops.postprocess(xp, mean, pads)


def _default_batch(plan, C, M, P, s, N):
    """The largest stack of windows whose code tensor stays below BATCH_CODE_BYTES and that a fused tier still takes
    where it takes one window (their plans bound the batch size too); at least 1."""
    code = 4 * M
    for d in plan.shape:
        code *= d // s
    b = max(1, min(BATCH_CODE_BYTES // code, N * len(plan.windows)))
    pad = tuple(p // 2 for p in P)

    def tiers(n):
        g = ops.Geometry.make(n, C, M, plan.shape, P, pad, [s] * len(P))
        return ops.fused_supported(g), ops.fusedg_supported(g)
    while b > 1 and tiers(b) != tiers(1):
        b //= 2
    return b
