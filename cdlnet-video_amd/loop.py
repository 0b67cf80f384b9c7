"""The unrolled-ISTA loop as one autograd node driving the HIP kernels.

Forward (reference model/net.py:76-92, 192-212, 659-675):
    yp, mean, pads, mask_p = pre_process(y)
    z_1     = ST(A_0 yp, tau_0)
    z_{k+1} = ST(z_k - A_k(mask * B_k z_k - yp), tau_k)          k = 1..K-1
    xhat    = post_process(B_0 z_K)
Backward is the hand-derived reverse sweep (what `loss.backward()` does through ATen in the
reference, train.py:98); with du_k = [z_{k+1} != 0] * g_{k+1}:
    dtau_k  = -sum sign(z_{k+1}) du_k
    q_k     = mask * (-A_k^T du_k)
    dA_k    = -du_k (x) r_k,   r_k = mask * B_k z_k - yp  (kept from the forward sweep; it is thin)
    dB_k    =  z_k  (x) q_k
    g_k     = du_k + B_k^T q_k
and, when y / sigma require grad (the forward is a torch graph in both in the reference), with u_0 = A_0 yp:
    dL/dyp  = sum_k A_k^T du_k            (the unmasked sum behind q_k; k = 0 adds the synthesis half of stage 0)
    dL/dc_n = sum_k sum_m t[k,1,m] dtau[k,n,m]     (per-sample threshold gradients, contracted here)
With a noise-level map c[n,pix] (a dense (N,1,*code grid) tensor) the threshold of code element
(n, m, pix) is t[k,0,m] + c[n,pix] t[k,1,m]: the generic sweeps carry the map into their shrinkage epilogues, and
    dt[k,1,m]   = -sum_{n,pix} c[n,pix] sign(z_{k+1}) du_k      (a second, map-weighted partial per row)
    dL/dc[n,pix] = -sum_k sum_m t[k,1,m] sign(z_{k+1}) du_k     (cdl_sigma_grad: a channel reduction per iteration)
    dL/dy   = cdl_preprocess_bwd(dL/dyp, dL/dxhat)  (reflect pad adjoint and the mean)
The gradient with respect to the mask is not produced (it needs mask * B_k z_k at masked-out pixels).
"""
import collections
import types

import torch

from . import ops

# Kernel selection for the forward sweep: "auto" uses the fused MFMA kernels whenever the geometry
# has one (cdl_fused2d_supported) and the shape-generic kernels otherwise; "generic" forces the latter.
# PRECISION applies to the fused 2-D kernels only: "split3" (split-bf16 with three products per multiply: fp32-grade, the
# default), "split4" (all four products: exact fp32 products -- what an objective that differences two forward passes
# needs, see precision_scope / train.mcsure_loss) or "bf16".  "fp32" is a different tier altogether: no fused kernels and no
# matrix cores -- the three-launch iteration on the fp32 VALU kernels (plain fp32 FMAs, several times slower), for the cases
# where 16-17 significant bits per MFMA operand are not enough (cancelling filter gradients: DESIGN.md section 6).
BACKEND = "auto"
ARITHMETIC = tuple(ops.PRECISION) + ("fp32",)
PRECISION = "split3"
# How the fused sweeps store the codes that never leave them (z_1..z_{K-1}, du_k): "blocked" (pixel-blocked
# fp32: same values as "nchw", wider memory accesses; the default), "nchw", or "blocked_bf16" (opt-in bf16
# STORAGE: half the bytes of the dominant tensors, outside the 1e-5 parity gate -- PSNR parity only).
CODE_LAYOUT = "blocked"
# Where a sweep with a noise-level map runs: "generic" (the three-launch tier: the default) or "fused" -- the map forms of the
# fused 2-D kernels wherever _route allows them, the generic tier everywhere else.
MAP_TIER = "generic"
_MAP_TIERS = ("generic", "fused")


def set_map_tier(name):
    global MAP_TIER
    if name not in _MAP_TIERS:
        raise ValueError(name)
    MAP_TIER = name


class map_tier_scope:
    """`with map_tier_scope("fused"): ...` -- sweeps with a noise-level map started inside take that tier (their reverse
    sweeps follow their forward whenever backward() is called); restored on exit, also when the block raises."""

    def __init__(self, name):
        if name not in _MAP_TIERS:
            raise ValueError(name)
        self.name = name

    def __enter__(self):
        global MAP_TIER
        self.saved, MAP_TIER = MAP_TIER, self.name
        return self

    def __exit__(self, *exc):
        global MAP_TIER
        MAP_TIER = self.saved
        return False


# Where a CDLNetVideo sweep with one noise level per FRAME -- c of shape (N,1,D,1,1) -- runs: "generic" (the level is
# expanded to a dense map and takes the map's route: the default) or "fused" -- the tile / grouped strip kernels with one
# threshold row per (sample, frame) wherever _route allows it, the dense map everywhere else.  A knob
# of its own: neither value of MAP_TIER changes what it does.
FRAME_TIER = "generic"


def set_frame_tier(name):
    global FRAME_TIER
    if name not in _MAP_TIERS:
        raise ValueError(name)
    FRAME_TIER = name


class frame_tier_scope:
    """`with frame_tier_scope("fused"): ...` -- network calls with per-frame noise levels started inside take that tier
    (their reverse sweeps follow their forward whenever backward() is called); restored on exit, also when the block raises."""

    def __init__(self, name):
        if name not in _MAP_TIERS:
            raise ValueError(name)
        self.name = name

    def __enter__(self):
        global FRAME_TIER
        self.saved, FRAME_TIER = FRAME_TIER, self.name
        return self

    def __exit__(self, *exc):
        global FRAME_TIER
        FRAME_TIER = self.saved
        return False


def set_backend(name):
    global BACKEND
    if name not in ("auto", "generic"):
        raise ValueError(name)
    BACKEND = name


def set_precision(name):
    global PRECISION
    if name not in ARITHMETIC:
        raise ValueError(name)
    PRECISION = name


class precision_scope:
    """`with precision_scope("split4"): ...` -- the fused 2-D sweeps started inside run in that arithmetic; their reverse
    sweeps use the arithmetic of their forward whenever backward() is called.  `precision_scope("fp32")`: every network
    call started inside (any net of this package) runs, forward and backward, on the fp32 VALU kernels."""

    def __init__(self, name):
        if name not in ARITHMETIC:
            raise ValueError(name)
        self.name = name

    def __enter__(self):
        global PRECISION
        self.saved, PRECISION = PRECISION, self.name
        return self

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self.saved
        return False


def set_code_layout(name):
    global CODE_LAYOUT
    if name not in ops._FUSED_LAYOUTS:              # "rsc" is the strip kernels' own, chosen by ops.fusedg_code_layout
        raise ValueError(name)
    CODE_LAYOUT = name


# Callables to run once per backward pass, queued on the autograd engine from the end of a reverse sweep (they run
# after the engine has accumulated every gradient of that pass): the data-parallel gradient exchange
# (parallel.GradientBucket.attach).
_BACKWARD_END = []
_queued = [False]


def on_backward_end(fn):
    """Register `fn()` to run at the end of every backward pass that contains a reverse sweep of this module;
    returns a callable that removes it."""
    _BACKWARD_END.append(fn)
    return lambda: _BACKWARD_END.remove(fn) if fn in _BACKWARD_END else None


def _queue_backward_end():
    if not _BACKWARD_END or _queued[0]:
        return                                    # e.g. MC-SURE: two sweeps in one pass, one exchange
    _queued[0] = True

    def run():
        _queued[0] = False
        for fn in list(_BACKWARD_END):
            fn()

    torch.autograd.Variable._execution_engine.queue_callback(run)


def _save(ctx, **named):
    """Save tensors for backward by name: each value is None, a tensor or a sequence of tensors (possibly empty).  One
    save_for_backward call with the tensors in order; the layout (name -> None / tensor / length) stays on ctx."""
    flat, layout = [], {}
    for name, v in named.items():
        if v is None:
            layout[name] = None
        elif isinstance(v, torch.Tensor):
            layout[name] = -1
            flat.append(v)
        else:
            layout[name] = len(v)
            flat.extend(v)
    ctx.save_for_backward(*flat)
    ctx.saved_layout = layout


def _saved(ctx):
    """What `_save` saved, under the same names: None as None, tensors as tensors, sequences as tuples."""
    flat = iter(ctx.saved_tensors)
    return types.SimpleNamespace(**{name: None if n is None else next(flat) if n < 0 else tuple(next(flat) for _ in range(n))
                                    for name, n in ctx.saved_layout.items()})


def _sweep_geometry(yp, A, s):
    """Geometry of a sweep from the pre-processed input, the filter banks and the stride: padding P // 2."""
    P = tuple(A[0].shape[2:])
    return ops.Geometry.make(yp.shape[0], yp.shape[1], A[0].shape[0], yp.shape[2:], P, tuple(p // 2 for p in P),
                             [s] * (yp.dim() - 2))


def _map_args(c, t):
    """(cmap, tslope): a noise-level map c -- a dense (N,1,*code grid) tensor (net._noise_scale) -- and the slopes t[:,1]
    as (K,M), what the generic sweeps read beside tau = t[k,0,m]; (None, None) for one level per sample, or none."""
    if c is None or c.dim() <= 1:
        return None, None
    return c, t.detach().reshape(t.shape[0], 2, t.shape[2])[:, 1].contiguous()


def _zero_grads(A, B):
    """The filter gradients of a reverse sweep that got no upstream gradient."""
    return [torch.zeros_like(w) for w in A], [torch.zeros_like(w) for w in B]


def _add_sweeps(first, second):
    """(dA, dB) of two reverse sweeps of one node, summed; `first` is (None, None) where only the second ran."""
    if first[0] is None:
        return second
    return tuple([a + b for a, b in zip(x, y)] for x, y in zip(first, second))


def _forward_generic(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, cmap=None, tslope=None):
    """Whole sweep from one C call (cdl_ista_forward): same launches as the stepwise form below.  cmap (N,1,*code grid)
    with tslope (K,M): the noise-level map; tau then holds t[k,0,m]."""
    keep = keep_codes or keep_resid
    xp, z, codes, resid, _ = ops.ista_forward(g, yp, mask_p, tau, A, B, keep, cmap=cmap, tslope=tslope)
    return xp, z, codes, (resid if keep_resid else []), []


def _forward_generic_stepwise(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, cmap=None, tslope=None):
    """Same sweep driven launch by launch from Python (kept for tests and experiments)."""
    K = len(A)
    codes, resid = [], []
    slope = (lambda k: tslope[k]) if cmap is not None else (lambda k: None)
    z = ops.analysis(g, yp, A[0], 1.0, None, None, tau[0], cmap=cmap, tslope=slope(0))
    codes.append(z)
    for k in range(1, K):
        r = ops.synthesis(g, z, B[k], 1.0, None, mask_p, yp)
        z = ops.analysis(g, r, A[k], -1.0, z, None, tau[k], cmap=cmap, tslope=slope(k))
        if keep_codes:
            codes.append(z)
        if keep_resid:
            resid.append(r)
    xp = ops.synthesis(g, z, B[0], 1.0)
    return xp, z, codes, resid, []


def _forward_fused(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, layout=None, *, keep_maps=False, cmap=None, tslope=None):
    """The whole sweep from one C call (cdl_fused2d_forward): per iteration one fused launch + a thin
    assemble, enqueued back to back with no per-launch host work.  codes[:-1] come back in `layout`
    (default CODE_LAYOUT), codes[-1] = z_K as (N,M,H,W).  keep_maps: the bit maps although nothing is kept (what a
    tangent sweep needs of the primal).  cmap / tslope: the noise-level map, as _forward_generic's."""
    keep = keep_codes or keep_resid
    xp, z, codes, resid, maps = ops.fused_forward(g, yp, mask_p, tau, A, B, keep, PRECISION,
                                                  layout or CODE_LAYOUT, keep_maps=keep_maps, cmap=cmap, tslope=tslope)
    return xp, z, codes, (resid if keep_resid else []), (maps if keep_resid or keep_maps else [])


def _forward_fused_stepwise(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, layout="nchw", *, cmap=None, tslope=None):
    """Same sweep driven launch by launch from Python (kept for tests and experiments)."""
    K = len(A)
    frags = [ops.fused_prep(A[k], B[(k + 1) % K]) for k in range(K)]   # last one pairs A_{K-1} with D = B_0
    patches = ops.fused_patches(g, yp.device)
    codes, resid, maps = [], [], []
    r, z = yp, None
    for k in range(K):
        bits = ops.fused_map(g, yp.device) if keep_resid else None
        z = ops.fused_iter(g, r, z, tau[k], frags[k], 1.0 if k == 0 else -1.0, patches, PRECISION, map_out=bits,
                           lay_in=layout, lay_out="nchw" if k == K - 1 else layout, cmap=cmap,
                           tslope=tslope[k] if cmap is not None else None)
        if keep_codes or k == 0:
            codes.append(z)
        if keep_resid:
            maps.append(bits)
        if k < K - 1:
            r = ops.fused_assemble(g, patches, mask_p, yp, 1.0)
            if keep_resid:
                resid.append(r)
    xp = ops.fused_assemble(g, patches, None, None, 1.0)
    return xp, z, codes, resid, maps


def _forward_fusedg(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, layout="nchw", *, keep_maps=False, planes=False):
    """cdl_fusedg_forward: the fused iteration for C > 1 / 3-D / P in {3,5,7} / M <= 64, and (the strip kernel) for one
    image channel, stride 1 / 2, M <= 192: one fused launch + a thin assemble per iteration.  codes[:-1] come back in
    `layout` ("nchw", or "rsc" where ops.fusedg_code_layout(g) says so), codes[-1] = z_K as (N,M,..).  keep_maps: as
    _forward_fused's.  planes: tau is (K, N*D, M), one threshold row per (sample, frame)."""
    keep = keep_codes or keep_resid
    xp, z, codes, resid, maps = ops.fusedg_forward(g, yp, mask_p, tau, A, B, keep, layout, keep_maps=keep_maps,
                                                   **(dict(planes=True) if planes else {}))
    return xp, z, codes, (resid if keep_resid else []), (maps if keep_resid or keep_maps else [])


def _backward_fusedg(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, layout="nchw", dyp=None, dtau=None,
                     planes=False):
    """cdl_fusedg_backward: per iteration one fused reverse stage (du_k, threshold partials, patches of q_k), a thin
    assemble and the two filter gradients.  `layout`: that of codes[:-1].  planes: c is (N*D), one level per (sample, frame),
    and dtau (K, N*D, M)."""
    if g_xp is None and g_z is None:
        return _zero_grads(A, B)
    return ops.fusedg_backward(g, yp, mask_p, c, list(A), list(B), list(codes), list(resid), g_xp, g_z, dt,
                               maps=list(maps) if maps else None, layout=layout, dyp=dyp, dtau=dtau,
                               **(dict(planes=True) if planes else {}))


def _backward_generic(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, dyp=None, dtau=None,
                      cmap=None, tslope=None, dcmap=None):
    """Reverse sweep from one C call (cdl_ista_backward; dyp / dtau: see ops.fused_backward).  cmap / tslope: the noise-level
    map of the forward in place of c (then None, as dtau); dcmap (nullable) receives dL/dcmap."""
    if g_xp is None and g_z is None:
        return _zero_grads(A, B)
    return ops.ista_backward(g, yp, mask_p, c, list(A), list(B), list(codes), list(resid), g_xp, g_z, dt, dyp=dyp,
                             dtau=dtau, cmap=cmap, tslope=tslope, dcmap=dcmap)


def _backward_generic_stepwise(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, dyp=None, dtau=None,
                               cmap=None, tslope=None, dcmap=None):
    """The same gradients from an independent composition, launch by launch from Python.  cdl_ista_backward runs
    cdl_analysis_rev (the analysis with the gate and the threshold sums in one step) and cdl_wgrad_pair per iteration; this
    twin runs tau_grad (ungated), the gated synthesis, two gated / plain wgrad calls and the gated analysis.  That it shares
    no launch sequence with the C sweep is why it is kept: the tests compare the two, and reach the gated kernels through it."""
    if cmap is not None:
        return _backward_generic_stepwise_map(g, K, yp, mask_p, A, B, codes, resid, g_xp, g_z, dt, dyp, cmap, tslope, dcmap)
    dA, dB = [None] * K, [None] * K
    zK = codes[K - 1]
    if g_xp is not None:
        dB[0] = ops.wgrad(g, zK, g_xp, 1.0)
        gk = ops.analysis(g, g_xp, B[0], 1.0, g_z, None, None)      # B_0^T g_xp (+ g_z)
    else:
        dB[0] = torch.zeros_like(B[0])
        gk = g_z.contiguous() if g_z is not None else torch.zeros_like(zK)
    for k in range(K - 1, 0, -1):
        z_next, z_k, r_k = codes[k], codes[k - 1], resid[k - 1]
        ops.tau_grad(g, gk, z_next, c, dt[k], dtau[k] if dtau is not None else None)
        if dyp is not None:                                         # S = A_k^T du_k; dyp (+)= S; q = -mask S
            q = ops.synthesis(g, gk, A[k], 1.0, z_next, None, None)
            ops.dyp_split(g, q, mask_p, dyp, k < K - 1)
        else:
            q = ops.synthesis(g, gk, A[k], -1.0, z_next, mask_p, None)
        dA[k] = ops.wgrad(g, gk, r_k, -1.0, gate=z_next)
        dB[k] = ops.wgrad(g, z_k, q, 1.0)
        gk = ops.analysis(g, q, B[k], 1.0, gk, z_next, None)
    ops.tau_grad(g, gk, codes[0], c, dt[0], dtau[0] if dtau is not None else None)
    dA[0] = ops.wgrad(g, gk, yp, 1.0, gate=codes[0])
    if dyp is not None:                                             # u_0 = A_0 yp
        ops.dyp_split(g, ops.synthesis(g, gk, A[0], 1.0, codes[0]), None, dyp, K > 1, make_q=False)
    return dA, dB


def _backward_generic_stepwise_map(g, K, yp, mask_p, A, B, codes, resid, g_xp, g_z, dt, dyp, cmap, tslope, dcmap):
    """The stepwise reverse sweep with a noise-level map: the launches of cdl_ista_backward, one op each."""
    dA, dB = [None] * K, [None] * K
    zK = codes[K - 1]
    if g_xp is not None:
        dB[0] = ops.wgrad(g, zK, g_xp, 1.0)
        gk = ops.analysis_rev(g, g_xp, B[0], 1.0, g_z, zK, None, dt[K - 1], cmap=cmap)
    else:
        dB[0] = torch.zeros_like(B[0])
        gk = g_z.clone()
        ops.tau_grad(g, gk, zK, None, dt[K - 1], cmap=cmap, gate=True)
    for k in range(K - 1, -1, -1):                                  # gk = du_k (gated), dt[k] written
        if dcmap is not None:
            ops.sigma_grad(g, gk, codes[k], tslope[k], dcmap, k < K - 1)
        if k == 0:
            break
        if dyp is not None:
            q = ops.synthesis(g, gk, A[k], 1.0, None, None, None)
            ops.dyp_split(g, q, mask_p, dyp, k < K - 1)
        else:
            q = ops.synthesis(g, gk, A[k], -1.0, None, mask_p, None)
        dA[k], dB[k] = ops.wgrad_pair(g, gk, resid[k - 1], -1.0, codes[k - 1], q, 1.0)
        gk = ops.analysis_rev(g, q, B[k], 1.0, gk, codes[k - 1], None, dt[k - 1], cmap=cmap)
    dA[0] = ops.wgrad(g, gk, yp, 1.0)
    if dyp is not None:                                             # u_0 = A_0 yp
        ops.dyp_split(g, ops.synthesis(g, gk, A[0], 1.0), None, dyp, K > 1, make_q=False)
    return dA, dB


def _backward_fused(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, layout=None, precision=None,
                    dyp=None, dtau=None, cmap=None, tslope=None, dcmap=None):
    """Reverse sweep from one C call (cdl_fused2d_backward): per iteration one stage launch (1 fat read +
    the 2-bit map of z_{k+1}, 1 fat write; dA_k rides in it), a thin assemble, one MFMA filter-gradient launch (dB_k: 1 fat
    read) and one launch that reduces dA_k, dB_k and dt[k].  maps: the forward's bit maps (rebuilt from the codes when absent); `layout`: that of codes[:-1].
    cmap / tslope / dcmap: as _backward_generic's."""
    if g_xp is None and g_z is None:
        return _zero_grads(A, B)
    return ops.fused_backward(g, yp, mask_p, c, list(A), list(B), list(codes), list(resid), g_xp, g_z, dt,
                              precision or PRECISION, maps=list(maps) if maps else None, layout=layout or CODE_LAYOUT,
                              dyp=dyp, dtau=dtau, cmap=cmap, tslope=tslope, dcmap=dcmap)


def _backward_fused_stepwise(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, layout="nchw",
                             dyp=None, dtau=None, cmap=None, tslope=None, dcmap=None):
    """Same reverse sweep driven launch by launch from Python (kept for tests and experiments)."""
    assert maps or layout == "nchw"
    prec = PRECISION
    dev = yp.device
    dA, dB = [None] * K, [None] * K
    patches = ops.fused_patches(g, dev)
    ws = ops.fused_wgrad_workspace(g, dev)
    tiles = ops.fused_tiles(g)                    # with a map: the weighted partials behind the plain ones
    dtp = torch.empty(((2 if cmap is not None else 1) * tiles, g.M), device=dev, dtype=torch.float32)
    mp = (lambda k: dict(cmap=cmap, tslope=tslope[k], dcmap=dcmap, dcmap_add=k < K - 1)) if cmap is not None else (lambda k: {})
    thin, du_next = g_xp, g_z
    (dB[0],) = ops.fused_wgrad(g, ws, codes[K - 1], g_xp, 1.0, precision=prec)[:1]
    for k in range(K - 1, -1, -1):
        frags = ops.fused_prep(B[(k + 1) % K], A[k])          # analysis-like bank, synthesis-like bank
        du = ops.fused_stage_bwd(g, thin, du_next, maps[k] if maps else codes[k], frags, patches, dtp,
                                 k >= 1 or dyp is not None, prec, lay_in="nchw" if k == K - 1 else layout, lay_out=layout,
                                 **mp(k))
        ops.fused_dtau_reduce(g, dtp[:tiles], c, dt[k], dtau[k] if dtau is not None else None,
                              weighted=dtp[tiles:] if cmap is not None else None)
        if k == 0 and dyp is not None:                              # u_0 = A_0 yp
            ops.fused_assemble(g, patches, acc=dyp, acc_add=K > 1, write_out=False)
        if k >= 1:
            q = ops.fused_assemble(g, patches, mask_p, None, -1.0, acc=dyp, acc_add=k < K - 1)
            dA[k], dB[k] = ops.fused_wgrad(g, ws, du, resid[k - 1], -1.0, codes[k - 1], q, 1.0, prec, layout=layout)
            thin = q
        else:
            (dA[0],) = ops.fused_wgrad(g, ws, du, yp, 1.0, precision=prec, layout=layout)[:1]
        du_next = du
    return dA, dB


def _arithmetic_aware(cls):
    """Class decorator of the autograd Functions below: a call made under PRECISION == "fp32" runs its forward AND (whenever it
    happens) its backward with the generic entry points pinned to the fp32 VALU kernels (ops.exact_fp32)."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args):
        _queued[0] = False                        # a backward pass that raised after queueing its end must not mute the next
        ctx.exact = PRECISION == "fp32"
        with ops.exact_fp32(ctx.exact):
            return fwd(ctx, *args)

    def backward(ctx, *grads):
        with ops.exact_fp32(ctx.exact):
            return bwd(ctx, *grads)

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


def _no_data_gradients(ctx, names=((0, "y"), (1, "mask"), (2, "sigma"))):
    """The CSR reverse sweeps produce parameter and neighbour-code gradients only, UnrolledISTA's no mask gradient.  The
    reference's loop is differentiable in the observation, the mask and sigma (no caller in the reference uses the
    mask's); asking for what a sweep does not produce must fail loudly rather than return a silent None."""
    for idx, name in names:
        if ctx.needs_input_grad[idx]:
            raise NotImplementedError(f"cdlnet_video_amd: the gradient with respect to `{name}` is not implemented "
                                      f"(the HIP reverse sweep returns parameter gradients only); detach() it")


def _route(g, exact, is_map, frames=False):
    """The tier of a sweep: "fused" (the 2-D MFMA kernels), "fusedg" (the tile / strip kernels) or "generic".  The fused
    tiers are matrix-core kernels that read tau[n,m]: the "fp32" arithmetic (`exact`) and a noise-level map run the generic --
    unless MAP_TIER is "fused" and the sweep is one the 2-D kernels' map forms exist for: split3 arithmetic, fp32 code storage,
    a geometry of the 2-D tier (the tile / strip kernels take no map).  frames: the map is one level per (sample, frame),
    (N,1,D,1,1) -- with FRAME_TIER "fused" the tile / grouped strip kernels take it as a threshold row per plane, where there
    is more than one frame and one of the two takes the geometry (with D > 1 the strip kernel proper, which is 2-D, never does)."""
    if BACKEND != "auto" or exact:
        return "generic"
    if is_map and frames and FRAME_TIER == "fused" and g.dims[0] > 1 and ops.fusedg_supported(g):
        return "fusedg"
    if is_map:
        fused_map = MAP_TIER == "fused" and PRECISION == "split3" and CODE_LAYOUT in ("nchw", "blocked")
        return "fused" if fused_map and ops.fused_supported(g) else "generic"
    if ops.fused_supported(g):
        return "fused"
    return "fusedg" if ops.fusedg_supported(g) else "generic"


# What the nodes below need of a tier, one argument convention per role.  `st` is the routed context (it carries layout and
# precision); mp the map keywords of _map_args (the generic tier and the fused 2-D one: what _route sends a map to); keep_gates: keep what gates a tangent sweep although
# nothing else is kept -- the bit maps on the fused tiers, all K codes on the generic one.  The entries name the sweeps
# through the module when they are CALLED: a test that replaces loop._forward_generic by its stepwise twin reaches every node.
#   layout(g, keep, handed_out, tangent) -> layout of the codes that stay inside the sweeps (None: the reference's only)
#   forward(st, g, yp, mask_p, tau, A, B, keep_codes, keep_resid, keep_gates, **mp) -> (xp, z, codes, resid, maps)
#   reverse(st, g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps, dyp, dtau, **mp) -> (dA, dB)
#   tangent(st, g, vp, mask_p, A, B, codes, maps, keep, last) -> (xdp, zd, rd)           (codes, maps: the primal's)
#   tangent_reverse(st, g, K, vp, mask_p, A, B, codes, maps, zd, rd, g_xdp, g_zd) -> (dA, dB)
#   negated_dA: the tangent sweep keeps -rd_k, so its reverse sweep's dA_k (k >= 1) comes out negated
_Tier = collections.namedtuple("_Tier", "layout forward reverse tangent tangent_reverse negated_dA")


def _tangent_reverse_fused(name):
    """The tangent net is linear: on the fused tiers its reverse sweep is the tier's own with vp, zd, -rd for yp, codes,
    resid, the primal's maps, and neither thresholds (their output is never returned) nor data gradients."""
    return lambda st, g, K, vp, mask_p, A, B, codes, maps, zd, rd, g_xdp, g_zd: _TIERS[name].reverse(
        st, g, K, vp, mask_p, None, A, B, zd, rd, g_xdp, g_zd, vp.new_empty((K, 2, g.M)), maps)


def _planes(st):
    """The keyword that switches a sweep of the fused generic tier to one threshold row per (sample, frame): set where
    _forward_sweep routed per-frame levels there (st.frames), absent otherwise -- the sweeps then get today's arguments."""
    return dict(planes=True) if getattr(st, "frames", False) else {}


def _frame_levels(g, c):
    """Whether c holds one noise level per (sample, frame) of a clip: (N,1,D,1,1) against an in-plane code grid larger than
    one pixel (net._noise_scale hands it over in this form under FRAME_TIER "fused")."""
    return (c is not None and c.dim() == 5 and g.ndim == 3 and tuple(c.shape[3:]) == (1, 1)
            and tuple(g.code_spatial[1:]) != (1, 1))


def _dense_levels(g, c):
    """Per-frame levels as the dense map the generic tier reads: what net._noise_scale expands them to without the knob."""
    return c.expand((g.N, 1) + tuple(g.code_spatial)).contiguous()


_TIERS = {
    "fused": _Tier(
        layout=lambda g, keep, handed_out, tangent: "nchw" if handed_out else CODE_LAYOUT,
        forward=lambda st, g, yp, mask_p, tau, A, B, keep_codes, keep_resid, keep_gates=False, **mp: _forward_fused(
            g, yp, mask_p, tau, A, B, keep_codes, keep_resid, st.layout, keep_maps=keep_gates, **mp),
        reverse=lambda st, g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps, dyp=None, dtau=None, **mp: _backward_fused(
            g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps, layout=st.layout, precision=st.precision,
            dyp=dyp, dtau=dtau, **mp),
        tangent=lambda st, g, vp, mask_p, A, B, codes, maps, keep, last: _tangent_fused(
            g, vp, mask_p, A, B, maps, keep, st.layout, st.precision, last=last),
        tangent_reverse=_tangent_reverse_fused("fused"), negated_dA=True),
    "fusedg": _Tier(                               # handed-out codes are (N,M,..), and cdl_fusedg_tangent takes nothing else
        layout=lambda g, keep, handed_out, tangent: "nchw" if handed_out or tangent else ops.fusedg_code_layout(g, training=keep),
        forward=lambda st, g, yp, mask_p, tau, A, B, keep_codes, keep_resid, keep_gates=False: _forward_fusedg(
            g, yp, mask_p, tau, A, B, keep_codes, keep_resid, st.layout, keep_maps=keep_gates, **_planes(st)),
        reverse=lambda st, g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps, dyp=None, dtau=None: _backward_fusedg(
            g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps, layout=st.layout, dyp=dyp, dtau=dtau,
            **(_planes(st) if c is not None else {})),          # (a tangent's reverse sweep reads no level: the plain form)
        tangent=lambda st, g, vp, mask_p, A, B, codes, maps, keep, last: _tangent_fusedg(
            g, vp, mask_p, A, B, maps, keep, last=last),
        tangent_reverse=_tangent_reverse_fused("fusedg"), negated_dA=True),
    "generic": _Tier(
        layout=lambda g, keep, handed_out, tangent: None,
        forward=lambda st, g, yp, mask_p, tau, A, B, keep_codes, keep_resid, keep_gates=False, **mp: _forward_generic(
            g, yp, mask_p, tau, A, B, keep_codes or keep_gates, keep_resid, **mp),
        reverse=lambda st, g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps, dyp=None, dtau=None, **mp:
            _backward_generic(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, dyp=dyp, dtau=dtau, **mp),
        tangent=lambda st, g, vp, mask_p, A, B, codes, maps, keep, last: _tangent_generic(
            g, vp, mask_p, A, B, codes, keep, last=last),
        tangent_reverse=lambda st, g, K, vp, mask_p, A, B, codes, maps, zd, rd, g_xdp, g_zd: _tangent_backward_generic(
            g, K, vp, mask_p, A, B, codes, zd, rd, g_xdp if g_xdp is not None else torch.zeros_like(vp), g_zd),
        negated_dA=False),                         # (g_xdp None, a loss on zd_K alone: a zero image gradient to the sweep)
}


def _forward_sweep(ctx, g, yp, mask_p, c, t, A, B, keep, want_codes, keep_maps=False, tangent=False):
    """The tier choice and the forward sweep of one pre-processed batch: (xp, z, codes, resid, maps).  `ctx` (an autograd
    context, or any namespace carrying `exact`) receives what the reverse sweep reads: tier (and fused / fusedg as flags),
    is_map, layout, precision.  UnrolledISTA.forward, TangentISTA.forward and run_windows all go through here, so a window
    and a tangent's primal take exactly the tier a sample of their geometry takes.  want_codes: the codes are handed to the
    caller (forward_generator), as (N,M,..); tangent: a tangent sweep follows, in a layout it reads; keep_maps: _Tier's keep_gates."""
    frames = _frame_levels(g, c)
    ctx.tier = _route(g, ctx.exact, c is not None and c.dim() > 1, **(dict(frames=True) if frames else {}))
    ctx.frames = frames and ctx.tier == "fusedg"   # per-frame levels stay on the fused generic tier: a threshold row per plane
    if frames and not ctx.frames:
        c = _dense_levels(g, c)                    # any other route: the dense map, as without FRAME_TIER
    cmap, tslope = (None, None) if ctx.frames else _map_args(c, t)      # with a map tau holds t[k,0,m] for every sample
    ctx.is_map = cmap is not None
    if ctx.frames:                                 # t[k,0] + c[n,d] * t[k,1]: cdl_thresholds with N * D levels
        tau = ops.thresholds(t, c.reshape(-1), g.N * g.dims[0])
    else:
        tau = ops.thresholds(t, None if ctx.is_map else c, g.N)
    ctx.fused, ctx.fusedg = ctx.tier == "fused", ctx.tier == "fusedg"
    tier = _TIERS[ctx.tier]
    ctx.layout = tier.layout(g, keep, want_codes, tangent)
    ctx.precision = PRECISION                      # the reverse sweep runs in the forward's arithmetic
    return tier.forward(ctx, g, yp, mask_p, tau, A, B, keep or want_codes, keep, keep_maps,
                        **(dict(cmap=cmap, tslope=tslope) if ctx.is_map else {}))


def _reverse_sweep(ctx, sv, g_xp, g_z, dt, want_y=False, want_c=False):
    """The primal's reverse sweep of a routed context (what _forward_sweep left on ctx; sv: what the node saved): (dA, dB,
    dyp, dtau, dcmap), dt (K,2,M) filled in place.  dyp (with want_y), dtau (K,N,M) or -- with a noise-level map -- dcmap (with
    want_c) only when asked for: otherwise the sweeps get NULLs and run exactly the parameter-only launches."""
    K, g, dev = ctx.K, ctx.geom, sv.yp.device
    live = g_xp is not None or g_z is not None
    dyp = torch.empty(g.image_shape(), device=dev, dtype=torch.float32) if want_y and live else None
    frames = getattr(ctx, "frames", False)         # per-frame levels on the fused generic tier: N * D "samples"
    c = sv.c.reshape(-1) if frames else sv.c
    if not frames and _frame_levels(g, c):         # per-frame levels that took another route: the dense map of the forward
        c = _dense_levels(g, c)
    rows = g.N * g.dims[0] if frames else g.N
    dtau = torch.empty((K, rows, g.M), device=dev, dtype=torch.float32) if want_c and live and not ctx.is_map else None
    cmap, tslope = (None, None) if frames else _map_args(c, sv.t)
    dcmap = torch.empty_like(cmap) if want_c and live and ctx.is_map else None      # dL/dc comes back as a map
    mp = dict(cmap=cmap, tslope=tslope, dcmap=dcmap) if ctx.is_map else {}
    dA, dB = _TIERS[ctx.tier].reverse(ctx, g, K, sv.yp, sv.mask_p, None if ctx.is_map else c, sv.A, sv.B, sv.codes,
                                      sv.resid, g_xp, g_z, dt, sv.maps, dyp, dtau, **mp)
    if dcmap is not None and dcmap.shape != sv.c.shape:       # expanded per-frame levels: the adjoint of the expansion
        dcmap = dcmap.sum(dim=(3, 4), keepdim=True)
    return dA, dB, dyp, dtau, dcmap


@_arithmetic_aware
class UnrolledISTA(torch.autograd.Function):
    """(y, mask, c, t, A_0..A_{K-1}, B_0..B_{K-1}) -> (xhat, z_K[, z_1..z_{K-1}])."""

    @staticmethod
    def forward(ctx, y, mask, c, t, cfg, *weights):
        K, s = cfg["K"], cfg["s"]
        A, B = weights[:K], weights[K:]
        yp, mean, pads, mask_p = ops.preprocess(y, s, mask)
        g = _sweep_geometry(yp, A, s)

        ctx.set_materialize_grads(False)          # an unused z output must not cost a fat zero tensor
        _no_data_gradients(ctx, ((1, "mask"),))   # y and sigma (through c): dL/dyp and dtau from the sweeps
        keep = any(ctx.needs_input_grad)          # all False under torch.no_grad()
        ctx.want_y = ctx.needs_input_grad[0]
        ctx.want_c = ctx.needs_input_grad[2] and c is not None
        want_codes = cfg.get("all_codes", False)
        xp, z, codes, resid, maps = _forward_sweep(ctx, g, yp, mask_p, c, t, A, B, keep, want_codes)
        xhat = ops.postprocess(xp, mean, pads)

        ctx.geom, ctx.pads, ctx.K = g, pads, K
        if keep:
            # the adjoint of preprocess needs the unpadded mask (its per-sample sum is taken in cdl_preprocess_bwd)
            _save(ctx, yp=yp, mask_p=mask_p, c=c, t=t, A=A, B=B, codes=codes, resid=resid, maps=maps,
                  y_mask=mask if ctx.want_y else None)
        outs = (xhat, z)
        if want_codes:
            extra = tuple(codes[:-1])
            ctx.mark_non_differentiable(*extra)
            outs = outs + extra
        return outs

    @staticmethod
    def backward(ctx, g_xhat, g_z, *_unused):
        K, g = ctx.K, ctx.geom
        sv = _saved(ctx)       # codes z_1..z_K, resid r_1..r_{K-1}, fused tiers: maps, the bit maps of z_1..z_K
        dt = torch.zeros((K, 2, g.M), device=sv.yp.device, dtype=torch.float32)
        g_xp = ops.postprocess_bwd(g_xhat.contiguous(), ctx.pads) if g_xhat is not None else None
        g_z = g_z.contiguous() if g_z is not None else None
        dA, dB, dyp, dtau, dc = _reverse_sweep(ctx, sv, g_xp, g_z, dt, ctx.want_y, ctx.want_c)
        dy = None
        if dyp is not None:                            # a loss on z only: no mean term
            dy = ops.preprocess_bwd(dyp, ctx.pads, g_xhat.contiguous() if g_xhat is not None else None, sv.y_mask)
        if dtau is not None:                           # tau[k,n,m] = t[k,0,m] + c[n] t[k,1,m] (per-frame levels: n = (sample, frame))
            dc = torch.einsum("knm,km->n", dtau, sv.t.detach().reshape(K, 2, g.M)[:, 1]).reshape(sv.c.shape)

        _queue_backward_end()
        return (dy, None, dc, dt.reshape(sv.t.shape), None, *dA, *dB)


# ------------------------------------------------------------------------------------------
# Forward-mode tangent of the plain loop: with the supports G_k = [z_{k+1} != 0] of the primal fixed
# the loop is affine in y, and a direction v in y propagates through the same recursion with the shrinkage replaced by G_k:
#     zd_1 = G_0 A_0 vp      rd_k = mask B_k zd_k - vp      zd_{k+1} = G_k (zd_k - A_k rd_k)      xdot = post(B_0 zd_K)
# (vp, the mean added back: preprocess(v)).  No threshold appears.  The tangent net is linear, so its reverse sweep is the
# primal's with codes -> zd, residuals -> rd, yp -> vp, the PRIMAL's gates, and no threshold / data gradient.
def _tangent_generic(g, vp, mask_p, A, B, gates, keep, last=False):
    """Whole generic tangent sweep from one C call (cdl_tangent_forward): (xdp, zd, rd); `last`: see ops.tangent_forward."""
    return ops.tangent_forward(g, vp, mask_p, A, B, gates, keep, last=last)


def _tangent_generic_stepwise(g, vp, mask_p, A, B, gates, keep):
    """Same sweep driven launch by launch from Python (kept for tests and experiments)."""
    K = len(A)
    dts = torch.empty(2 * g.M, device=vp.device, dtype=torch.float32)      # threshold sums of the gated step: never read
    zd, rd = [], []
    z = ops.analysis_rev(g, vp, A[0], 1.0, None, gates[0], None, dts)
    zd.append(z)
    for k in range(1, K):
        r = ops.synthesis(g, z, B[k], 1.0, None, mask_p, vp)
        z = ops.analysis_rev(g, r, A[k], -1.0, z, gates[k], None, dts)
        zd.append(z)
        rd.append(r)
    xdp = ops.synthesis(g, z, B[0], 1.0)
    return xdp, (zd if keep else []), (rd if keep else [])


def _tangent_backward_generic(g, K, vp, mask_p, A, B, gates, zd, rd, g_xp, g_zd=None):
    """Reverse sweep of the generic tangent sweep from one C call (cdl_tangent_backward): (dA, dB)."""
    return ops.tangent_backward(g, vp, mask_p, list(A), list(B), list(gates), list(zd), list(rd), g_xp, g_zd)


def _tangent_backward_generic_stepwise(g, K, vp, mask_p, A, B, gates, zd, rd, g_xp, g_zd=None):
    """Same reverse sweep driven launch by launch from Python (kept for tests and experiments)."""
    dA, dB = [None] * K, [None] * K
    dts = torch.empty(2 * g.M, device=vp.device, dtype=torch.float32)
    dB[0] = ops.wgrad(g, zd[K - 1], g_xp, 1.0)
    gk = ops.analysis_rev(g, g_xp, B[0], 1.0, g_zd, gates[K - 1], None, dts)
    for k in range(K - 1, 0, -1):
        q = ops.synthesis(g, gk, A[k], -1.0, None, mask_p, None)
        dA[k], dB[k] = ops.wgrad_pair(g, gk, rd[k - 1], -1.0, zd[k - 1], q, 1.0)
        gk = ops.analysis_rev(g, q, B[k], 1.0, gk, gates[k - 1], None, dts)
    dA[0] = ops.wgrad(g, gk, vp, 1.0)
    return dA, dB


def _tangent_fused(g, vp, mask_p, A, B, maps, keep, layout=None, precision=None, last=False):
    """Whole tangent sweep on the fused 2-D kernels from one C call (cdl_fused2d_tangent): per iteration one reverse-stage
    launch with the forward's prepared pair and the primal's bit map, and one assemble.  Returns (xdp, zd, nrd): nrd are
    the NEGATED residuals -rd_k (the stages' thin operand)."""
    return ops.fused_tangent(g, vp, mask_p, A, B, maps, keep, precision or PRECISION, layout or CODE_LAYOUT, last=last)


def _tangent_fused_stepwise(g, vp, mask_p, A, B, maps, keep, layout="nchw", precision=None):
    """Same sweep driven launch by launch from Python (kept for tests and experiments)."""
    K = len(A)
    prec = precision or PRECISION
    frags = [ops.fused_prep(A[k], B[(k + 1) % K]) for k in range(K)]   # the forward's pairs
    patches = ops.fused_patches(g, vp.device)
    dtp = torch.empty((ops.fused_tiles(g), g.M), device=vp.device, dtype=torch.float32)
    nvp = torch.neg(vp)
    zd, nrd = [], []
    thin, z = vp, None
    for k in range(K):
        z = ops.fused_stage_bwd(g, thin, z, maps[k], frags[k], patches, dtp, True, prec,
                                lay_in=layout if k else "nchw", lay_out="nchw" if k == K - 1 else layout)
        zd.append(z)
        if k < K - 1:
            thin = ops.fused_assemble(g, patches, mask_p, nvp, -1.0)
            nrd.append(thin)
    xdp = ops.fused_assemble(g, patches, None, None, 1.0)
    return xdp, (zd if keep else []), (nrd if keep else [])


def _tangent_fusedg(g, vp, mask_p, A, B, maps, keep, last=False):
    """cdl_fusedg_tangent: the same construction on the tile / strip kernels (codes in the reference's layout)."""
    return ops.fusedg_tangent(g, vp, mask_p, A, B, maps, keep, last=last)


@_arithmetic_aware
class TangentISTA(torch.autograd.Function):
    """(y, v, mask, c, t, A_0..A_{K-1}, B_0..B_{K-1}) -> (xhat, xdot): the primal of UnrolledISTA and its directional
    derivative in y along v at the primal's supports.  The tangent follows the primal's tier (fused 2-D / fused generic /
    generic).  Gradients for t (from xhat alone) and both filter banks (the sum of the two reverse sweeps).
    With cfg["codes"] (the no-neighbour branch of the CSR nets' jvp_recurrent) the outputs are (xhat, xdot, z_K, zd_K) and
    the reverse sweeps take the codes' upstream gradients as well."""

    @staticmethod
    def forward(ctx, y, v, mask, c, t, cfg, *weights):
        K, s = cfg["K"], cfg["s"]
        A, B = weights[:K], weights[K:]
        yp, mean, pads, mask_p = ops.preprocess(y, s, mask)
        vp, vmean, _, _ = ops.preprocess(v, s, mask)          # linear: the same mean rule, mask and reflect pad
        g = _sweep_geometry(yp, A, s)

        ctx.set_materialize_grads(False)
        _no_data_gradients(ctx, ((0, "y"), (1, "v"), (2, "mask"), (3, "sigma")))
        keep = any(ctx.needs_input_grad)
        want_codes = cfg.get("codes", False)
        # the primal, as UnrolledISTA runs it (net.jvp refuses blocked_bf16; so does the C sweep), then its tier's tangent
        xp, z, codes, resid, maps = _forward_sweep(ctx, g, yp, mask_p, c, t, A, B, keep, False, keep_maps=True, tangent=True)
        xdp, zd, rd = _TIERS[ctx.tier].tangent(ctx, g, vp, mask_p, A, B, codes, maps, keep, want_codes)
        zdK = zd[-1] if want_codes else None           # (N,M,..) on every tier; the ping-pong table's last when nothing is kept
        if not keep:
            zd = []
        xhat = ops.postprocess(xp, mean, pads)
        xdot = ops.postprocess(xdp, vmean, pads)

        ctx.geom, ctx.pads, ctx.K = g, pads, K
        if keep:
            _save(ctx, yp=yp, vp=vp, mask_p=mask_p, c=c, t=t, A=A, B=B, codes=codes, resid=resid, zd=zd, rd=rd, maps=maps)
        return (xhat, xdot, z, zdK) if want_codes else (xhat, xdot)

    @staticmethod
    def backward(ctx, g_xhat, g_xdot, g_z=None, g_zd=None):
        K, g = ctx.K, ctx.geom
        sv = _saved(ctx)
        tier = _TIERS[ctx.tier]
        dt = torch.zeros((K, 2, g.M), device=sv.yp.device, dtype=torch.float32)
        dA = dB = None
        g_z = g_z.contiguous() if g_z is not None else None
        g_zd = g_zd.contiguous() if g_zd is not None else None
        if g_xhat is not None or g_z is not None:      # the primal's reverse sweep, as UnrolledISTA runs it
            g_xp = ops.postprocess_bwd(g_xhat.contiguous(), ctx.pads) if g_xhat is not None else None
            dA, dB = _reverse_sweep(ctx, sv, g_xp, g_z, dt)[:2]
        if g_xdot is not None or g_zd is not None:     # the tangent's: same sweep, other operands, the primal's gates
            g_xdp = ops.postprocess_bwd(g_xdot.contiguous(), ctx.pads) if g_xdot is not None else None
            tA, tB = tier.tangent_reverse(ctx, g, K, sv.vp, sv.mask_p, sv.A, sv.B, sv.codes, sv.maps, sv.zd, sv.rd, g_xdp, g_zd)
            if tier.negated_dA:
                tA = [tA[0]] + [torch.neg(w) for w in tA[1:]]
            dA, dB = _add_sweeps((dA, dB), (tA, tB))
        if dA is None:
            dA, dB = _zero_grads(sv.A, sv.B)
        _queue_backward_end()
        return (None, None, None, None, dt.reshape(sv.t.shape), None, *dA, *dB)


# ------------------------------------------------------------------------------------------
# CSR temporal variants (reference model/net.py:426-463, 525-568):
# the same loop with the shrinkage replaced by prox_CSR / prox_CSR_f2 around a neighbour frame's code.
#     u_0 = A_0 yp                       z_1     = prox(u_0; zp[, za], lam_0, gam_0)
#     u_k = z_k - A_k(mask B_k z_k - yp) z_{k+1} = prox(u_k; ...)
# The reverse sweep needs u_k (the derivative masks of the nested shrinkages are not recoverable from
# z_{k+1}), so the training forward keeps u_k next to z_k (both written by the analysis kernel, whose
# epilogue is the proximal map: cdl_analysis_prox); everything else is _backward_generic with the gating
# done by cdl_prox_csr_bwd, which also accumulates the neighbour-code gradients.
# A noise-level map: cmap (N,1,*code grid) with tslope (K,3,M), the slopes of lam, gam1, gam2;
# lam / gam1 / gam2 then hold the constant parts t[k,0,m], g1[k,0,m], g2[k,0,m] for every sample.
def _forward_csr(g, yp, mask_p, lam, gam1, gam2, zp, za, A, B, keep, cmap=None, tslope=None):
    xp, z, codes, resid, us = ops.ista_forward(g, yp, mask_p, lam, A, B, keep, zp, za, gam1, gam2, cmap=cmap, tslope=tslope)
    return xp, z, us, codes, resid


def _csr_slopes(t, g1, g2):
    """(K,3,M): t[:,1], g1[:,1], g2[:,1] (zeros without g2) -- the slopes the CSR kernels read with a noise-level map."""
    K, M = t.shape[0], t.shape[2]
    rows = [p.detach().reshape(K, 2, M)[:, 1] for p in (t, g1)]
    rows.append(g2.detach().reshape(K, 2, M)[:, 1] if g2 is not None else torch.zeros_like(rows[0]))
    return torch.stack(rows, dim=1).contiguous()


def _forward_csr_stepwise(g, yp, mask_p, lam, gam1, gam2, zp, za, A, B, keep, cmap=None, tslope=None):
    K = len(A)
    us, codes, resid = [], [], []
    g2 = (lambda k: gam2[k]) if za is not None else (lambda k: None)
    mp = (lambda k: dict(cmap=cmap, tslope=tslope[k])) if cmap is not None else (lambda k: {})
    new = lambda: torch.empty(g.code_shape(), device=yp.device, dtype=torch.float32)
    u = new() if keep else None
    z = ops.analysis_prox(g, yp, A[0], 1.0, None, zp, lam[0], gam1[0], za, g2(0), u_out=u, **mp(0))
    spare = None if keep else new()                      # inference: z ping-pongs between two buffers
    for k in range(1, K):
        if keep:
            us.append(u)
            codes.append(z)
            u = new()
        r = ops.synthesis(g, z, B[k], 1.0, None, mask_p, yp)
        z_next = ops.analysis_prox(g, r, A[k], -1.0, z, zp, lam[k], gam1[k], za, g2(k), u_out=u, out=spare, **mp(k))
        spare, z = (None, z_next) if keep else (z, z_next)
        if keep:
            resid.append(r)
    if keep:
        us.append(u)
        codes.append(z)
    xp = ops.synthesis(g, z, B[0], 1.0)
    return xp, z, us, codes, resid


@_arithmetic_aware
class TemporalISTA(torch.autograd.Function):
    """(y, mask, c, z_prev, z_after|None, t, g1, g2|None, A.., B..) -> (xhat, z_K); gradients for the
    neighbour codes, the three threshold families and both filter banks, and -- when asked for -- for y and c.  c: None,
    one level per sample (N,), or a noise-level map (N,1,*code grid) that all three threshold families follow; its
    gradient comes back in the same form."""

    @staticmethod
    def forward(ctx, y, mask, c, zp, za, t, g1, g2, cfg, *weights):
        K, s = cfg["K"], cfg["s"]
        A, B = weights[:K], weights[K:]
        yp, mean, pads, mask_p = ops.preprocess(y, s, mask)
        g = _sweep_geometry(yp, A, s)
        N = g.N
        if tuple(zp.shape) != g.code_shape() or (za is not None and tuple(za.shape) != g.code_shape()):
            raise ValueError(f"neighbour code shape {tuple(zp.shape)} does not match this frame's {g.code_shape()}")
        zp = zp.contiguous()
        za = za.contiguous() if za is not None else None
        ctx.is_map = c is not None and c.dim() > 1
        cs = None if ctx.is_map else c                 # a map: the thresholds' constant parts, the slopes beside them
        lam, gam1 = ops.thresholds(t, cs, N), ops.thresholds(g1, cs, N)
        gam2 = ops.thresholds(g2, cs, N) if za is not None else None
        mp = dict(cmap=c, tslope=_csr_slopes(t, g1, g2 if za is not None else None)) if ctx.is_map else {}
        ctx.set_materialize_grads(False)
        _no_data_gradients(ctx, ((1, "mask"),))
        keep = any(ctx.needs_input_grad)
        ctx.want_y = ctx.needs_input_grad[0]
        ctx.want_c = ctx.needs_input_grad[2] and c is not None
        xp, z, us, codes, resid = _forward_csr(g, yp, mask_p, lam, gam1, gam2, zp, za, A, B, keep, **mp)
        xhat = ops.postprocess(xp, mean, pads)
        ctx.geom, ctx.pads, ctx.K = g, pads, K
        if keep:
            _save(ctx, yp=yp, mask_p=mask_p, c=c, zp=zp, za=za, t=t, g1=g1, g2=g2 if za is not None else None, lam=lam,
                  gam1=gam1, gam2=gam2, A=A, B=B, us=us, codes=codes, resid=resid,
                  y_mask=mask if ctx.want_y else None)       # preprocess_bwd's unpadded mask
        return xhat, z

    @staticmethod
    def backward(ctx, g_xhat, g_z):
        K, g = ctx.K, ctx.geom
        sv = _saved(ctx)
        yp, mask_p, c, zp, za, t, g1, g2, y_mask = sv.yp, sv.mask_p, sv.c, sv.zp, sv.za, sv.t, sv.g1, sv.g2, sv.y_mask
        lam, gam1, gam2, A, B, us, codes, resid = sv.lam, sv.gam1, sv.gam2, sv.A, sv.B, sv.us, sv.codes, sv.resid
        dev = yp.device
        dt = torch.zeros((K, 2, g.M), device=dev, dtype=torch.float32)
        dg1 = torch.zeros_like(dt)
        dg2 = torch.zeros_like(dt) if za is not None else None
        need_zp, need_za = ctx.needs_input_grad[3], za is not None and ctx.needs_input_grad[4]
        gzp = torch.zeros_like(zp) if need_zp else None
        gza = torch.zeros_like(zp) if need_za else None
        g_xp = ops.postprocess_bwd(g_xhat.contiguous(), ctx.pads) if g_xhat is not None else None
        g_z = g_z.contiguous() if g_z is not None else None
        dy = dc = None
        if g_xp is None and g_z is None:
            dA, dB = _zero_grads(A, B)
        else:
            # data gradients only when asked for: otherwise the sweep gets NULLs and runs the parameter-only launches
            dyp = torch.empty(g.image_shape(), device=dev, dtype=torch.float32) if ctx.want_y else None
            dtau = torch.zeros((K, 3, g.N, g.M), device=dev, dtype=torch.float32) \
                if ctx.want_c and not ctx.is_map else None
            mp = {}
            if ctx.is_map:
                dc = torch.empty_like(c) if ctx.want_c else None
                mp = dict(cmap=c, tslope=_csr_slopes(t, g1, g2 if za is not None else None), dcmap=dc)
            dA, dB = _backward_csr(g, K, yp, mask_p, None if ctx.is_map else c, A, B, codes, resid, us, zp, za, lam, gam1,
                                   gam2, g_xp, g_z, dt, dg1, dg2, gzp, gza, dyp=dyp, dtau=dtau, **mp)
            if dyp is not None:                        # a loss on z only: no mean term
                dy = ops.preprocess_bwd(dyp, ctx.pads, g_xhat.contiguous() if g_xhat is not None else None, y_mask)
            if dtau is not None:                       # lam[k,n,m] = t[k,0,m] + c[n] t[k,1,m], and the same for gam1, gam2
                dc = torch.einsum("kfnm,kfm->n", dtau, _csr_slopes(t, g1, g2 if za is not None else None))
        _queue_backward_end()
        return (dy, None, dc, gzp, gza, dt.reshape(t.shape), dg1.reshape(g1.shape),
                dg2.reshape(g2.shape) if dg2 is not None else None, None, *dA, *dB)


def _backward_csr(g, K, yp, mask_p, c, A, B, codes, resid, us, zp, za, lam, gam1, gam2, g_xp, g_z, dt, dg1, dg2, gzp, gza,
                  dyp=None, dtau=None, cmap=None, tslope=None, dcmap=None):
    """Reverse sweep of the CSR loop from one C call (cdl_ista_backward's CSR branch): (dA, dB); fills dt, dg1[, dg2] and
    accumulates into gzp / gza (nullable).  dyp (thin), dtau (K,3,N,M): the data gradients; cmap / tslope (K,3,M) / dcmap:
    a noise-level map in the place of c, and its gradient."""
    return ops.ista_backward(g, yp, mask_p, c, list(A), list(B), list(codes), list(resid), g_xp, g_z, dt, list(us), zp, za,
                             lam, gam1, gam2, dg1, dg2, gzp, gza, dyp, dtau, cmap=cmap, tslope=tslope, dcmap=dcmap)


def _backward_csr_stepwise(g, K, yp, mask_p, c, A, B, codes, resid, us, zp, za, lam, gam1, gam2, g_xp, g_z, dt, dg1, dg2,
                           gzp, gza, dyp=None, dtau=None, cmap=None, tslope=None, dcmap=None):
    """Same reverse sweep driven launch by launch from Python (kept for tests and experiments)."""
    dA, dB = [None] * K, [None] * K
    if dcmap is not None:
        dcmap.zero_()
    if g_xp is not None:
        dB[0] = ops.wgrad(g, codes[K - 1], g_xp, 1.0)
        gk = ops.analysis(g, g_xp, B[0], 1.0, g_z, None, None)       # B_0^T g_xp (+ g_z)
    else:
        dB[0] = torch.zeros_like(B[0])
        gk = g_z.clone()
    for k in range(K - 1, -1, -1):                                   # gk: dL/dz_{k+1} -> dL/du_k in place
        mp = dict(cmap=cmap, tslope=tslope[k], dcmap=dcmap) if cmap is not None else {}
        ops.prox_csr_bwd(g, gk, us[k], zp, lam[k], gam1[k], c, dt[k], dg1[k], za, gam2[k] if za is not None else None,
                         dg2[k] if za is not None else None, gzp, gza, out=gk, dsum_n=dtau[k] if dtau is not None else None,
                         **mp)
        if k == 0:
            break
        if dyp is not None:                                          # S = A_k^T du_k; dyp (+)= S; q = -mask S
            q = ops.synthesis(g, gk, A[k], 1.0, None, None, None)
            ops.dyp_split(g, q, mask_p, dyp, k < K - 1)
        else:
            q = ops.synthesis(g, gk, A[k], -1.0, None, mask_p, None)
        dA[k], dB[k] = ops.wgrad_pair(g, gk, resid[k - 1], -1.0, codes[k - 1], q, 1.0)
        gk = ops.analysis(g, q, B[k], 1.0, gk, None, None)
    dA[0] = ops.wgrad(g, gk, yp, 1.0)
    if dyp is not None:                                              # u_0 = A_0 yp
        ops.dyp_split(g, ops.synthesis(g, gk, A[0], 1.0), None, dyp, K > 1, make_q=False)
    return dA, dB


# ------------------------------------------------------------------------------------------
# Forward-mode tangent of the CSR loop.  prox_CSR / prox_CSR_f2 are piecewise linear in (u, z_prev,
# z_after): at the primal's gates (read off u_k, the neighbour codes and the thresholds; ops.prox_csr_tangent) a direction
# (v, zd_prev, zd_after) in (y, z_prev, z_after) propagates through
#     ud_0 = A_0 vp     rd_k = mask B_k zd_k - vp     ud_k = zd_k - A_k rd_k     zd_{k+1} = Jprox_k(ud_k; zd_prev, zd_after)
#     xdot = post(B_0 zd_K)
# with no threshold in any value.  The tangent net is linear in (vp, zd_prev, zd_after), and the transpose of Jprox_k is
# what cdl_prox_csr_bwd applies, so its reverse sweep is the primal's (_backward_csr) with yp -> vp, codes -> zd,
# residuals -> rd and the PRIMAL's u_k, neighbour codes and thresholds: it yields the filter gradients and
# dL/dzd_prev, dL/dzd_after; its threshold sums are discarded (the gates are piecewise constant).
# Under a noise-level map the gates are read at the primal's per-element thresholds: cmap with
# tslope (K,3,M) as in _forward_csr, lam / gam* the constant parts, handed to the forward and the reverse tangent sweep alike.
def _tangent_csr(g, vp, mask_p, lam, gam1, gam2, zp, za, zdp, zda, A, B, us, keep, cmap=None, tslope=None):
    """Whole CSR tangent sweep from one C call (cdl_csr_tangent_forward): (xdp, zd_K, zd, rd)."""
    return ops.csr_tangent_forward(g, vp, mask_p, lam, gam1, gam2, zp, za, zdp, zda, A, B, us, keep, cmap=cmap, tslope=tslope)


def _tangent_csr_stepwise(g, vp, mask_p, lam, gam1, gam2, zp, za, zdp, zda, A, B, us, keep, cmap=None, tslope=None):
    """Same sweep driven launch by launch from Python (kept for tests and experiments)."""
    K = len(A)
    g2 = (lambda k: gam2[k]) if za is not None else (lambda k: None)
    mp = (lambda k: dict(cmap=cmap, tslope=tslope[k])) if cmap is not None else (lambda k: {})
    zd, rd = [], []
    z = ops.analysis_prox_tangent(g, vp, A[0], 1.0, None, us[0], zp, lam[0], gam1[0], za, g2(0), zdp, zda, **mp(0))
    zd.append(z)
    for k in range(1, K):
        r = ops.synthesis(g, z, B[k], 1.0, None, mask_p, vp)
        z = ops.analysis_prox_tangent(g, r, A[k], -1.0, z, us[k], zp, lam[k], gam1[k], za, g2(k), zdp, zda, **mp(k))
        zd.append(z)
        rd.append(r)
    xdp = ops.synthesis(g, z, B[0], 1.0)
    return xdp, z, (zd if keep else []), (rd if keep else [])


def _tangent_backward_csr(g, K, vp, mask_p, A, B, zd, rd, us, zp, za, lam, gam1, gam2, g_xdp, g_zd, gzdp, gzda,
                          sweep=_backward_csr, cmap=None, tslope=None):
    """Reverse sweep of the CSR tangent sweep: (dA, dB), accumulating dL/dzd_prev, dL/dzd_after into gzdp / gzda (nullable).
    `sweep`: _backward_csr (one C call) or _backward_csr_stepwise.  cmap / tslope: the primal's noise-level map (no map
    gradient leaves the tangent: the gates are piecewise constant in it)."""
    sink = torch.empty((3, K, 2, g.M), device=vp.device, dtype=torch.float32)       # threshold sums nobody reads
    return sweep(g, K, vp, mask_p, None, A, B, zd, rd, us, zp, za, lam, gam1, gam2, g_xdp, g_zd, sink[0], sink[1],
                 sink[2] if za is not None else None, gzdp, gzda, cmap=cmap, tslope=tslope)


@_arithmetic_aware
class TangentTemporalISTA(torch.autograd.Function):
    """(y, v, mask, c, z_prev, zd_prev|None, z_after|None, zd_after|None, t, g1, g2|None, A.., B..) -> (xhat, xdot, z_K, zd_K):
    the primal of TemporalISTA and its derivative along (v, zd_prev, zd_after) at the primal's gates.  Gradients for the
    neighbour codes and the three threshold families (from xhat and z_K alone), for the neighbour tangents (from xdot and zd_K
    alone) and for both filter banks (the sum of the two reverse sweeps).  c: None, one level per sample (N,), or a
    noise-level map (N,1,*code grid) as TemporalISTA takes it (no gradient for c here)."""

    @staticmethod
    def forward(ctx, y, v, mask, c, zp, zdp, za, zda, t, g1, g2, cfg, *weights):
        K, s = cfg["K"], cfg["s"]
        A, B = weights[:K], weights[K:]
        yp, mean, pads, mask_p = ops.preprocess(y, s, mask)
        vp, vmean, _, _ = ops.preprocess(v, s, mask)          # linear: the same mean rule, mask and reflect pad
        g = _sweep_geometry(yp, A, s)
        N = g.N
        for name, x in (("z_prev", zp), ("zdot_prev", zdp), ("z_after", za), ("zdot_after", zda)):
            if x is not None and tuple(x.shape) != g.code_shape():
                raise ValueError(f"{name}: shape {tuple(x.shape)} does not match this frame's code shape {g.code_shape()}")
        zp, zdp, za, zda = (x.contiguous() if x is not None else None for x in (zp, zdp, za, zda))
        ctx.is_map = c is not None and c.dim() > 1
        cs = None if ctx.is_map else c                 # a map: the thresholds' constant parts, the slopes beside them
        lam, gam1 = ops.thresholds(t, cs, N), ops.thresholds(g1, cs, N)
        gam2 = ops.thresholds(g2, cs, N) if za is not None else None
        mp = dict(cmap=c, tslope=_csr_slopes(t, g1, g2 if za is not None else None)) if ctx.is_map else {}
        ctx.set_materialize_grads(False)
        _no_data_gradients(ctx, ((0, "y"), (1, "v"), (2, "mask"), (3, "sigma")))
        keep = any(ctx.needs_input_grad)
        # the gates are read off the primal's u_k: all K are kept whatever `keep` says
        xp, z, us, codes, resid = _forward_csr(g, yp, mask_p, lam, gam1, gam2, zp, za, A, B, True, **mp)
        xdp, zdK, zd, rd = _tangent_csr(g, vp, mask_p, lam, gam1, gam2, zp, za, zdp, zda, A, B, us, keep, **mp)
        xhat = ops.postprocess(xp, mean, pads)
        xdot = ops.postprocess(xdp, vmean, pads)
        ctx.geom, ctx.pads, ctx.K = g, pads, K
        if keep:
            _save(ctx, yp=yp, vp=vp, mask_p=mask_p, c=c, zp=zp, za=za, t=t, g1=g1, g2=g2 if za is not None else None,
                  lam=lam, gam1=gam1, gam2=gam2, A=A, B=B, us=us, codes=codes, resid=resid, zd=zd, rd=rd)
        return xhat, xdot, z, zdK

    @staticmethod
    def backward(ctx, g_xhat, g_xdot, g_z, g_zd):
        K, g = ctx.K, ctx.geom
        sv = _saved(ctx)
        yp, vp, mask_p, c, zp, za, t, g1, g2 = sv.yp, sv.vp, sv.mask_p, sv.c, sv.zp, sv.za, sv.t, sv.g1, sv.g2
        lam, gam1, gam2, A, B, us, codes, resid = sv.lam, sv.gam1, sv.gam2, sv.A, sv.B, sv.us, sv.codes, sv.resid
        zd, rd = sv.zd, sv.rd
        dev = yp.device
        dt = torch.zeros((K, 2, g.M), device=dev, dtype=torch.float32)
        dg1 = torch.zeros_like(dt)
        dg2 = torch.zeros_like(dt) if za is not None else None
        need = ctx.needs_input_grad
        new = lambda want: torch.zeros_like(zp) if want else None
        gzp, gzdp = new(need[4]), new(need[5])
        gza, gzda = new(za is not None and need[6]), new(za is not None and need[7])
        g_z = g_z.contiguous() if g_z is not None else None
        g_zd = g_zd.contiguous() if g_zd is not None else None
        dA = dB = None
        # a map takes c's place in both reverse sweeps (dt[:,1], dg*[:,1] are then the map-weighted sums)
        mp = dict(cmap=c, tslope=_csr_slopes(t, g1, g2 if za is not None else None)) if ctx.is_map else {}
        if g_xhat is not None or g_z is not None:      # the primal's reverse sweep, as TemporalISTA runs it
            g_xp = ops.postprocess_bwd(g_xhat.contiguous(), ctx.pads) if g_xhat is not None else None
            dA, dB = _backward_csr(g, K, yp, mask_p, None if ctx.is_map else c, A, B, codes, resid, us, zp, za, lam, gam1,
                                   gam2, g_xp, g_z, dt, dg1, dg2, gzp, gza, **mp)
        if g_xdot is not None or g_zd is not None:     # the tangent's: same sweep, other operands, the primal's gates
            g_xdp = ops.postprocess_bwd(g_xdot.contiguous(), ctx.pads) if g_xdot is not None else None
            tA, tB = _tangent_backward_csr(g, K, vp, mask_p, A, B, zd, rd, us, zp, za, lam, gam1, gam2, g_xdp, g_zd, gzdp,
                                           gzda, **mp)
            dA, dB = _add_sweeps((dA, dB), (tA, tB))
        if dA is None:
            dA, dB = _zero_grads(A, B)
        _queue_backward_end()
        return (None, None, None, None, gzp, gzdp, gza, gzda, dt.reshape(t.shape), dg1.reshape(g1.shape),
                dg2.reshape(g2.shape) if dg2 is not None else None, None, *dA, *dB)


# ------------------------------------------------------------------------------------------
# CDLNetVideo(residual=True) (reference model/net.py:199-212): a ResidualBlock
# rewrites the code after every iteration, so the sweep is a chain of per-iteration autograd nodes -- one ISTA
# iteration (the launches of _forward/_backward_generic_stepwise for one k), one block, ..., the synthesis.
@_arithmetic_aware
class _ISTAIteration(torch.autograd.Function):
    """(z_k | None, t_k (2,M..), A_k, B_k) -> z_{k+1} = ST(z_k - A_k(mask B_k z_k - yp), tau_k)."""

    @staticmethod
    def forward(ctx, zin, t_k, wA, wB, g, yp, mask_p, c):
        is_map = c is not None and c.dim() > 1         # noise-level map: see UnrolledISTA
        tau = ops.thresholds(t_k.reshape((1,) + tuple(t_k.shape)), None if is_map else c, g.N)[0]
        kw = dict(cmap=c, tslope=t_k.detach().reshape(2, g.M)[1].contiguous()) if is_map else {}
        if zin is None:
            r = yp
            z = ops.analysis(g, yp, wA, 1.0, None, None, tau, **kw)
        else:
            r = ops.synthesis(g, zin, wB, 1.0, None, mask_p, yp)
            z = ops.analysis(g, r, wA, -1.0, zin, None, tau, **kw)
        ctx.g, ctx.first, ctx.t_shape = g, zin is None, tuple(t_k.shape)
        ctx.mask_p, ctx.c = mask_p, c
        _save(ctx, zin=zin, r=r, z=z, wA=wA, wB=wB)
        return z

    @staticmethod
    def backward(ctx, gz):
        g = ctx.g
        sv = _saved(ctx)
        zin, r, z, wA, wB = sv.zin, sv.r, sv.z, sv.wA, sv.wB
        gk = gz.contiguous()
        dt_k = torch.zeros((2, g.M), device=gk.device, dtype=torch.float32)
        if ctx.c is not None and ctx.c.dim() > 1:
            ops.tau_grad(g, gk, z, None, dt_k, cmap=ctx.c)
        else:
            ops.tau_grad(g, gk, z, ctx.c, dt_k)
        dt_k = dt_k.reshape(ctx.t_shape)
        if ctx.first:
            dA = ops.wgrad(g, gk, r, 1.0, gate=z)
            return None, dt_k, dA, None, None, None, None, None
        q = ops.synthesis(g, gk, wA, -1.0, z, ctx.mask_p, None)
        dA = ops.wgrad(g, gk, r, -1.0, gate=z)
        dB = ops.wgrad(g, zin, q, 1.0)
        gzin = ops.analysis(g, q, wB, 1.0, gk, z, None)
        return gzin, dt_k, dA, dB, None, None, None, None


@_arithmetic_aware
class ResidualBlockFn(torch.autograd.Function):
    """(x, w1, w2) -> relu(conv2(relu(conv1 x)) + x)  (net.py:113-120)."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        g = ops.residual_geometry(x, w1)
        x = x.contiguous()                    # what the kernels read is what backward must see
        h, out = ops.residual_forward(g, x, w1, w2)
        ctx.g = g
        ctx.save_for_backward(x, h, out, w1, w2)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, h, out, w1, w2 = ctx.saved_tensors
        dx, dw1, dw2 = ops.residual_backward(ctx.g, x, h, out, w1, w2, g_out.contiguous())
        return dx, dw1, dw2


@_arithmetic_aware
class _Dictionary(torch.autograd.Function):
    """(z_K, B_0) -> xhat = post_process(D z_K)."""

    @staticmethod
    def forward(ctx, z, wB, g, mean, pads):
        xp = ops.synthesis(g, z, wB, 1.0)
        ctx.g, ctx.pads = g, pads
        ctx.save_for_backward(z, wB)
        return ops.postprocess(xp, mean, pads)

    @staticmethod
    def backward(ctx, g_xhat):
        z, wB = ctx.saved_tensors
        g_xp = ops.postprocess_bwd(g_xhat.contiguous(), ctx.pads)
        dB = ops.wgrad(ctx.g, z, g_xp, 1.0)
        gz = ops.analysis(ctx.g, g_xp, wB, 1.0, None, None, None)
        _queue_backward_end()
        return gz, dB, None, None, None


def run_residual(y, mask, c, t, A, B, s, blocks, all_codes=False):
    """CDLNetVideo.forward with residual=True: blocks[k] = (w1, w2) applied after iteration k.
    Returns (xhat, z) or, with all_codes, (xhat, z, ST outputs of every iteration) as forward_generator
    yields them (net.py:218-224: the code BEFORE its block)."""
    K = len(A)
    if torch.is_grad_enabled() and (y.requires_grad or (torch.is_tensor(mask) and mask.requires_grad)
                                    or (c is not None and c.requires_grad)):
        raise NotImplementedError("cdlnet_video_amd: gradients with respect to y / mask / sigma are not implemented")
    yp, mean, pads, mask_p = ops.preprocess(y, s, mask)
    g = _sweep_geometry(yp, A, s)
    if _frame_levels(g, c):                        # the chain of per-iteration nodes runs the generic operators: a dense map
        c = _dense_levels(g, c)
    z, shrunk = None, []
    for k in range(K):
        z = _ISTAIteration.apply(z, t[k], A[k], B[k], g, yp, mask_p, c)
        shrunk.append(z)
        z = ResidualBlockFn.apply(z, *blocks[k])
    xhat = _Dictionary.apply(z, B[0], g, mean, pads)
    return (xhat, z, *shrunk) if all_codes else (xhat, z)


def run_csr(y, mask, c, z_prev, z_after, t, g1, g2, A, B, s):
    """Front end of the neighbour branches; the no-neighbour branch is `run`."""
    cfg = {"K": len(A), "s": int(s)}
    return TemporalISTA.apply(y, mask, c, z_prev, z_after, t, g1, g2, cfg, *A, *B)


def run_tangent(y, v, mask, c, t, A, B, s, codes=False):
    """Front end of net.jvp: (xhat, xdot); with `codes` (jvp_recurrent without a neighbour) (xhat, xdot, z_K, zd_K)."""
    cfg = {"K": len(A), "s": int(s), "codes": bool(codes)}
    return TangentISTA.apply(y, v, mask, c, t, cfg, *A, *B)


def run_csr_tangent(y, v, mask, c, z_prev, zd_prev, z_after, zd_after, t, g1, g2, A, B, s):
    """Front end of the neighbour branches of jvp_recurrent: (xhat, xdot, z_K, zd_K)."""
    cfg = {"K": len(A), "s": int(s)}
    return TangentTemporalISTA.apply(y, v, mask, c, z_prev, zd_prev, z_after, zd_after, t, g1, g2, cfg, *A, *B)


def run(y, mask, c, t, A, B, s, all_codes=False):
    """Convenience front end used by the modules."""
    cfg = {"K": len(A), "s": int(s), "all_codes": bool(all_codes)}
    return UnrolledISTA.apply(y, mask, c, t, cfg, *A, *B)


def run_windows(yp, mask_p, c, t, A, B, s, plan, *, blend="crop", max_batch=None, sweep=None):
    """Inference on a PRE-PROCESSED frame cut into the windows of `plan` (windowed.plan_windows):
    xp, shaped like yp.  The windows -- one shape per plan -- are stacked along the batch axis, at most `max_batch`
    (sample, window) pairs per sweep (None: all of them), each batch runs the forward sweep of the tier its geometry takes
    (_forward_sweep: what a sample of that shape takes in UnrolledISTA), and the results are cropped to their cores or
    cross-faded into xp (`blend`: windowed.Plan.assemble).  c: None, one level per sample (N,), or a map (N,1,*code grid),
    which is cropped with its window.  No autograd graph is built.
    `sweep(yp_w, mask_w, c_w) -> xp_w` replaces the device sweep (t, A, B are then not read): the planner and the assembly
    against a restatement of the loop, on the CPU."""
    N = yp.shape[0]
    if sweep is None:
        def sweep(yp_w, mask_w, c_w):
            st = types.SimpleNamespace(exact=PRECISION == "fp32")
            with ops.exact_fp32(st.exact):
                return _forward_sweep(st, _sweep_geometry(yp_w, A, s), yp_w, mask_w, c_w, t, A, B, False, False)[0]
    is_map = c is not None and c.dim() > 1
    with torch.no_grad():
        if len(plan.windows) == 1 and (max_batch is None or max_batch >= N):      # the frame itself: nothing to copy
            return sweep(yp, mask_p, c)
        pairs = [(w, n) for w in range(len(plan.windows)) for n in range(N)]
        step = len(pairs) if max_batch is None else max(1, int(max_batch))
        outs = [[None] * N for _ in plan.windows]
        for i in range(0, len(pairs), step):
            group = pairs[i:i + step]
            yp_w = plan.gather(yp, group)
            mask_w = plan.gather(mask_p, group) if mask_p is not None else None
            if is_map:
                c_w = plan.gather(c, group, scale=s)
            else:
                c_w = c[[n for _, n in group]].contiguous() if c is not None else None
            xp_w = sweep(yp_w, mask_w, c_w)
            for j, (w, n) in enumerate(group):
                outs[w][n] = xp_w[j:j + 1]
        return plan.assemble([torch.cat(per_sample, 0) for per_sample in outs], blend)
