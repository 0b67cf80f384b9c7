"""The building blocks of the nets as differentiable functions.

The reference's `net.A[k]`, `net.B[k]`, `net.D`, `ST`, `prox_CSR`, `prox_CSR_f2`, `pre_process` and `post_process` are torch
code, differentiable in every argument, and people who change the loop compose them and call `backward()`.  Here each is
an autograd `Function` over the HIP entry points: the forward is the launch the nets' own sweeps make, the backward is the
adjoint kernel of the same library (the adjoint of `analysis` is `synthesis` and vice versa, `cdl_wgrad`,
`cdl_tau_grad_gate`, `cdl_prox_csr_b_bwd`, `cdl_preprocess_bwd` / `cdl_postprocess_bwd`).  A call made under
`precision_scope("fp32")` runs its backward on the same tier; every Function is once-differentiable.

Thresholds of the pointwise maps are python numbers or tensors that broadcast to the code shape (N, M, *spatial) -- after
left-padding with 1s each axis is 1 or the code's extent; a gradient comes back in the shape the threshold was given.
What is not produced raises: the gradient with respect to a mask, and any second derivative.
"""
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import loop, ops

__all__ = ["analysis", "synthesis", "shrink", "ST", "prox_csr", "prox_csr_f2", "analysis_shrink", "pre_process",
           "post_process"]      # section 23's blocks (the list is pinned); analysis_prox and ista_csr (section 24) are public beside it


# ------------------------------------------------------------------------------------------ argument checks
def _on_device(fn, **tensors):
    for name, t in tensors.items():
        if torch.is_tensor(t) and not t.is_cuda:
            raise RuntimeError(f"cdlnet_video_amd.functional.{fn}: `{name}` is on {t.device}. This package has no CPU "
                               "compute path; the operators run in HIP kernels on a ROCm device.")


def _no_mask_gradient(mask):
    if torch.is_tensor(mask) and mask.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("cdlnet_video_amd: the gradient with respect to `mask` is not implemented "
                                  "(the HIP reverse sweep returns parameter gradients only); detach() it")


def _geometry(fn, image_shape, w, stride):
    if not torch.is_tensor(w) or w.dim() not in (4, 5) or len(image_shape) != w.dim():
        raise ValueError(f"{fn}: expected (N,C,*spatial) data and (M,C,*P) filters of the same rank, 2-D or 3-D")
    if image_shape[1] != w.shape[1]:
        raise ValueError(f"{fn}: the data has {image_shape[1]} channels, the filters {w.shape[1]}")
    P = tuple(w.shape[2:])
    return ops.Geometry.make(image_shape[0], w.shape[1], w.shape[0], image_shape[2:], P, tuple(p // 2 for p in P), stride)


def _threshold(fn, name, t, code_shape, device, rows_only=False):
    """A threshold in the form the kernels read: float32, contiguous, of the code's rank, its first two axes 1 or full and
    its spatial axes all 1 or all full (ops.bcast_strides).  Formed by differentiable views of `t`, so autograd returns
    the gradient in the shape `t` was given; a partly spatial threshold (one level per frame, (N,1,D,1,1)) is expanded to
    the full code grid here -- 1/M of a code tensor unless it also has channel extent."""
    code_shape = tuple(code_shape)
    if isinstance(t, numbers.Number):
        return torch.full((1,) * len(code_shape), float(t), dtype=torch.float32, device=device)
    if not torch.is_tensor(t):                                          # a list, as torch.as_tensor takes it
        t = torch.as_tensor(t, dtype=torch.float32, device=device)
    if t.dim() > len(code_shape):
        raise ValueError(f"{fn}: `{name}` of shape {tuple(t.shape)} does not broadcast to the code shape {code_shape}")
    shape = (1,) * (len(code_shape) - t.dim()) + tuple(t.shape)
    if any(a not in (1, b) for a, b in zip(shape, code_shape)):
        raise ValueError(f"{fn}: `{name}` of shape {tuple(t.shape)} does not broadcast to the code shape {code_shape}")
    spatial = any(a != 1 for a in shape[2:])
    if spatial and rows_only:
        raise ValueError(f"{fn}: `{name}` of shape {tuple(t.shape)} varies over the spatial axes; the analysis epilogue takes "
                         f"one threshold per (sample, channel), a broadcast form of {code_shape[:2] + (1,) * len(shape[2:])}")
    t = t.to(device=device, dtype=torch.float32).reshape(shape)     # a threshold on another device is moved to the code's
    if rows_only:
        return t.expand(code_shape[:2] + shape[2:]).reshape(code_shape[:2]).contiguous()
    if spatial and shape[2:] != code_shape[2:]:
        t = t.expand(shape[:2] + code_shape[2:])
    return t.contiguous()


def _sum_to(grad, like):
    return grad if grad.shape == like.shape else grad.sum_to_size(like.shape)


# ------------------------------------------------------------------------------------------ linear operators
@loop._arithmetic_aware
class _Analysis(torch.autograd.Function):
    """(x, w, add | None) -> add + alpha * A x."""

    @staticmethod
    def forward(ctx, x, w, add, g, alpha):
        x = x.contiguous()
        ctx.g, ctx.alpha = g, alpha
        ctx.save_for_backward(x, w)
        return ops.analysis(g, x, w, alpha, add)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, w = ctx.saved_tensors
        gout = gout.contiguous()
        dx = ops.synthesis(ctx.g, gout, w, ctx.alpha) if ctx.needs_input_grad[0] else None
        dw = ops.wgrad(ctx.g, gout, x, ctx.alpha) if ctx.needs_input_grad[1] else None
        return dx, dw, (gout if ctx.needs_input_grad[2] else None), None, None


@loop._arithmetic_aware
class _Synthesis(torch.autograd.Function):
    """(z, w, mask | None, sub | None) -> mask * (alpha * B z) - sub."""

    @staticmethod
    def forward(ctx, z, w, mask, sub, g, alpha):
        z = z.contiguous()
        ctx.g, ctx.alpha = g, alpha
        loop._save(ctx, z=z, w=w, mask=mask)
        return ops.synthesis(g, z, w, alpha, None, mask, sub)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        sv = loop._saved(ctx)
        z, w = sv.z, sv.w
        gout = gout.contiguous()
        q = gout * sv.mask if sv.mask is not None else gout                         # thin
        dz = ops.analysis(ctx.g, q, w, ctx.alpha) if ctx.needs_input_grad[0] else None
        dw = ops.wgrad(ctx.g, z, q, ctx.alpha) if ctx.needs_input_grad[1] else None
        return dz, dw, None, (-gout if ctx.needs_input_grad[3] else None), None, None


def analysis(x, w, stride=1, alpha=1.0, add=None):
    """add + alpha * A x: the strided correlation of x (N,C,*sp) with the filters w (M,C,*P), 2-D or 3-D, zero padding
    P//2 (the geometry rules of ops.Geometry.make).  Differentiable in x (ops.synthesis with the same w), w (ops.wgrad)
    and add."""
    g = _geometry("analysis", tuple(x.shape), w, stride)
    if add is not None and tuple(add.shape) != g.code_shape():
        raise ValueError(f"analysis: `add` of shape {tuple(add.shape)} is not the code shape {g.code_shape()}")
    _on_device("analysis", x=x, w=w, add=add)
    return _Analysis.apply(x, w, add, g, float(alpha))


def synthesis(z, w, stride=1, alpha=1.0, mask=None, sub=None):
    """mask * (alpha * B z) - sub: the transposed correlation of the codes z (N,M,*sp) back to the image grid sp * stride
    (what cdl_synthesis computes).  Differentiable in z (ops.analysis of the masked upstream gradient), w (ops.wgrad)
    and sub; a mask that requires grad raises."""
    _no_mask_gradient(mask)
    if not torch.is_tensor(w) or w.dim() != z.dim() or z.shape[1] != w.shape[0]:
        raise ValueError("synthesis: expected (N,M,*spatial) codes and (M,C,*P) filters of the same rank")
    s = [stride] * (z.dim() - 2) if isinstance(stride, int) else list(stride)
    image = (z.shape[0], w.shape[1]) + tuple(int(d) * int(v) for d, v in zip(z.shape[2:], s))
    g = _geometry("synthesis", image, w, stride)
    for name, t in (("mask", mask), ("sub", sub)):
        if t is not None and tuple(t.shape) != g.image_shape():
            raise ValueError(f"synthesis: `{name}` of shape {tuple(t.shape)} is not the image shape {g.image_shape()}")
    _on_device("synthesis", z=z, w=w, mask=mask, sub=sub)
    if mask is not None:
        mask = mask.detach()
    return _Synthesis.apply(z, w, mask, sub, g, float(alpha))


# ------------------------------------------------------------------------------------------ pointwise maps
def _rows_geometry(code_shape):
    """The (1, rows) view of a code tensor: cdl_tau_grad's dt0 is then the per-row sum."""
    sp = tuple(code_shape[2:])
    return ops.Geometry.make(1, 1, code_shape[0] * code_shape[1], sp, (1,) * len(sp), (0,) * len(sp), 1)


def _code_geometry(code_shape):
    sp = tuple(code_shape[2:])
    return ops.Geometry.make(code_shape[0], 1, code_shape[1], sp, (1,) * len(sp), (0,) * len(sp), 1)


@loop._arithmetic_aware
class _Shrink(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        x = x.contiguous()
        ctx.save_for_backward(x, t)
        return ops.shrink_b(x, t)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, t = ctx.saved_tensors
        gout = gout.contiguous()
        if not ctx.needs_input_grad[1]:
            return ops.shrink_b_bwd(gout, x, t), None
        spatial = any(d != 1 for d in t.shape[2:])
        if spatial and t.shape[1] != 1:                                   # the full form: one value per code element
            el = torch.empty_like(x)
            gx = ops.shrink_b_bwd(gout, x, t, el)
            return (gx if ctx.needs_input_grad[0] else None), _sum_to(el, t)
        gx = ops.shrink_b_bwd(gout, x, t)
        if spatial:                                                       # shared over the channels: cdl_sigma_grad
            g = _code_geometry(x.shape)
            dt = torch.empty((x.shape[0], 1) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
            ops.sigma_grad(g, gx, x, torch.ones(g.M, device=x.device, dtype=torch.float32), dt, False)
        else:                                                             # the row form: cdl_tau_grad's row sums
            g = _rows_geometry(x.shape)
            dt = torch.empty((2, g.M), device=x.device, dtype=torch.float32)
            ops.tau_grad(g, gx, x, None, dt)
            dt = dt[0].reshape(tuple(x.shape[:2]) + (1,) * (x.dim() - 2))
        return (gx if ctx.needs_input_grad[0] else None), _sum_to(dt, t)


def shrink(x, t):
    """ST(x, t) = sign(x) * relu(|x| - t) (model/net.py:11-14) over a code tensor x (N,M,*sp); t a number or a tensor
    broadcastable to x.  Differentiable in x and t as autograd differentiates the expression (sign has zero gradient)."""
    if not torch.is_tensor(x) or x.dim() < 3:
        raise ValueError("shrink: expected an (N,M,*spatial) tensor")
    t = _threshold("shrink", "t", t, x.shape, x.device)
    _on_device("shrink", x=x)
    return _Shrink.apply(x, t)


ST = shrink


@loop._arithmetic_aware
class _Prox(torch.autograd.Function):
    """(u, z_prev, z_after | None, lam, gam1, gam2 | None) -> prox_CSR / prox_CSR_f2."""

    @staticmethod
    def forward(ctx, u, zp, za, lam, g1, g2):
        u, zp = u.contiguous(), zp.contiguous()
        za = za.contiguous() if za is not None else None
        ctx.g = _code_geometry(u.shape)
        ctx.f2 = za is not None
        loop._save(ctx, u=u, zp=zp, lam=lam, g1=g1, za=za, g2=g2 if ctx.f2 else None)
        return ops.prox_csr_b(ctx.g, u, zp, lam, g1, za, g2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        sv = loop._saved(ctx)
        u, zp, lam, g1, za, g2 = sv.u, sv.zp, sv.lam, sv.g1, sv.za, sv.g2
        need = ctx.needs_input_grad
        gzp = torch.zeros_like(u) if need[1] else None
        gza = torch.zeros_like(u) if ctx.f2 and need[2] else None
        gu, dl, d1, d2 = ops.prox_csr_b_bwd(ctx.g, gz.contiguous(), u, zp, lam, g1, za, g2,
                                            want=(need[3], need[4], ctx.f2 and need[5]), gz_prev=gzp, gz_after=gza)
        return (gu if need[0] else None, gzp, gza, _sum_to(dl, lam) if dl is not None else None,
                _sum_to(d1, g1) if d1 is not None else None, _sum_to(d2, g2) if d2 is not None else None)


def _prox(fn, u, z_prev, z_after, lambd, gamma1, gamma2):
    if not torch.is_tensor(u) or u.dim() not in (4, 5):
        raise ValueError(f"{fn}: expected (N,M,H,W) or (N,M,D,H,W) codes")
    for name, z in (("z_prev", z_prev), ("z_after", z_after)):
        if z is not None and (not torch.is_tensor(z) or tuple(z.shape) != tuple(u.shape)):
            raise ValueError(f"{fn}: `{name}` must be a tensor shaped like u {tuple(u.shape)}")
    lam = _threshold(fn, "lambd", lambd, u.shape, u.device)
    g1 = _threshold(fn, "gamma1" if z_after is not None else "gamma", gamma1, u.shape, u.device)
    g2 = _threshold(fn, "gamma2", gamma2, u.shape, u.device) if z_after is not None else None
    _on_device(fn, u=u, z_prev=z_prev, z_after=z_after)
    return _Prox.apply(u, z_prev, z_after, lam, g1, g2)


def prox_csr(u, z_prev, lambd, gamma):
    """prox_CSR of the reference (model/net.py:229-242); lambd, gamma: numbers or tensors broadcastable to u.
    Differentiable in every tensor argument."""
    return _prox("prox_csr", u, z_prev, None, lambd, gamma, None)


def prox_csr_f2(u, z_prev, z_after, lambd, gamma1, gamma2):
    """prox_CSR_f2 of the reference (model/net.py:244-262), likewise."""
    if z_after is None:
        raise ValueError("prox_csr_f2: z_after is required (prox_csr is the one-neighbour map)")
    return _prox("prox_csr_f2", u, z_prev, z_after, lambd, gamma1, gamma2)


# ------------------------------------------------------------------------------------------ analysis + shrinkage
@loop._arithmetic_aware
class _AnalysisShrink(torch.autograd.Function):
    """(x, w, tau (N,M), add | None) -> z = ST(add + alpha * A x, tau), the shrinkage in the analysis epilogue."""

    @staticmethod
    def forward(ctx, x, w, tau, add, g, alpha):
        x = x.contiguous()
        z = ops.analysis(g, x, w, alpha, add, None, tau)
        ctx.g, ctx.alpha = g, alpha
        ctx.save_for_backward(x, w, z)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        g = ctx.g
        x, w, z = ctx.saved_tensors
        need = ctx.needs_input_grad
        # the gradient of `add` is the upstream gradient at the support of z: gated into a copy; otherwise the gate
        # rides on the reads of the two operator launches
        gk = gz.clone(memory_format=torch.contiguous_format) if need[3] else gz.contiguous()
        dtau = None
        if need[2] or need[3]:
            dt_k = torch.empty((2, g.M), device=gk.device, dtype=torch.float32)
            dtau = torch.empty((g.N, g.M), device=gk.device, dtype=torch.float32) if need[2] else None
            ops.tau_grad(g, gk, z, None, dt_k, dtau, gate=need[3])
        dx = ops.synthesis(g, gk, w, ctx.alpha, z) if need[0] else None
        dw = ops.wgrad(g, gk, x, ctx.alpha, gate=z) if need[1] else None
        return dx, dw, dtau, (gk if need[3] else None), None, None


def analysis_shrink(x, w, t, stride=1, alpha=1.0, add=None):
    """ST(add + alpha * A x, t) with the shrinkage in the analysis kernel's epilogue: the launch one iteration of the
    nets' stepwise sweep makes.  t: a number or a tensor broadcastable to (N, M, 1, ..) -- one threshold per (sample,
    channel).  The backward runs at the support of the output; differentiable in x, w, t and add."""
    g = _geometry("analysis_shrink", tuple(x.shape), w, stride)
    if add is not None and tuple(add.shape) != g.code_shape():
        raise ValueError(f"analysis_shrink: `add` of shape {tuple(add.shape)} is not the code shape {g.code_shape()}")
    tau = _threshold("analysis_shrink", "t", t, g.code_shape(), x.device, rows_only=True)
    if tau.dim() != 2:                                                   # a number
        tau = tau.reshape(1, 1).expand(g.N, g.M).contiguous()
    _on_device("analysis_shrink", x=x, w=w, add=add)
    return _AnalysisShrink.apply(x, w, tau, add, g, float(alpha))


# ------------------------------------------------------------------------------------------ analysis + CSR map
@loop._arithmetic_aware
class _AnalysisProx(torch.autograd.Function):
    """(x, w, add | None, z_prev, z_after | None, thr, slopes | None, cmap | None) -> z = prox(add + alpha * A x), the CSR
    map in the analysis kernel's epilogue.  Row form: thr (3,N,M) = lam, gam1, gam2 per (sample, channel).  Map form: thr
    (3,M) the constant parts and slopes (3,M), cmap (N,1,*code grid): lam = thr[0,m] + cmap[n,pix] * slopes[0,m] etc.
    The third plane is unread without z_after."""

    @staticmethod
    def forward(ctx, x, w, add, zp, za, thr, slopes, cmap, g, alpha):
        x, zp = x.contiguous(), zp.contiguous()
        za = za.contiguous() if za is not None else None
        add = add.contiguous() if add is not None else None
        rows = thr if cmap is None else thr[:, None, :].expand(3, g.N, g.M).contiguous()
        keep = any(ctx.needs_input_grad)
        u = torch.empty(g.code_shape(), device=x.device, dtype=torch.float32) if keep else None
        mp = dict(cmap=cmap, tslope=slopes) if cmap is not None else {}
        z = ops.analysis_prox(g, x, w, alpha, add, zp, rows[0], rows[1], za, rows[2] if za is not None else None,
                              u_out=u, **mp)
        ctx.g, ctx.alpha, ctx.f2, ctx.mapped = g, alpha, za is not None, cmap is not None
        if keep:
            loop._save(ctx, x=x, w=w, zp=zp, za=za, rows=rows, slopes=slopes if ctx.mapped else None, cmap=cmap, u=u)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        g, need = ctx.g, ctx.needs_input_grad
        sv = loop._saved(ctx)
        x, w, zp, za, rows, slopes, cmap, u = sv.x, sv.w, sv.zp, sv.za, sv.rows, sv.slopes, sv.cmap, sv.u
        new = lambda *shape: torch.zeros(shape, device=gz.device, dtype=torch.float32)
        gzp = torch.zeros_like(u) if need[3] else None
        gza = torch.zeros_like(u) if ctx.f2 and need[4] else None
        dt = new(3, 2, g.M)                                             # [sum s, sum cmap s] per family
        dsum = new(3, g.N, g.M) if not ctx.mapped else None             # row form: the sums per (sample, channel)
        dcmap = torch.zeros_like(cmap) if ctx.mapped and need[7] else None
        mp = dict(cmap=cmap, tslope=slopes, dcmap=dcmap) if ctx.mapped else dict(dsum_n=dsum)
        gu = ops.prox_csr_bwd(g, gz.contiguous(), u, zp, rows[0], rows[1], None, dt[0], dt[1], za,
                              rows[2] if ctx.f2 else None, dt[2] if ctx.f2 else None, gzp, gza, **mp)
        dx = ops.synthesis(g, gu, w, ctx.alpha) if need[0] else None
        dw = ops.wgrad(g, gu, x, ctx.alpha) if need[1] else None
        dthr = (dt[:, 0] if ctx.mapped else dsum) if need[5] else None
        dslopes = dt[:, 1] if ctx.mapped and need[6] else None
        return dx, dw, (gu if need[2] else None), gzp, gza, dthr, dslopes, dcmap, None, None


def _is_map_form(t):
    return isinstance(t, (tuple, list)) and len(t) == 3 and torch.is_tensor(t[1])


def analysis_prox(x, w, z_prev, lambd, gamma1, z_after=None, gamma2=None, stride=1, alpha=1.0, add=None):
    """prox_CSR / prox_CSR_f2 of (add + alpha * A x; z_prev[, z_after]) with the proximal map in the analysis kernel's
    epilogue: the launch one iteration of the CSR nets' sweep makes, beside analysis_shrink.  The pre-shrinkage tensor is
    written once, for the backward, and never read back in the forward.  Thresholds:

    * numbers or tensors that broadcast to (N, M, 1, ..) -- one value per (sample, channel): the fused kernel's row form;
    * every threshold a triple `(t0, c, t1)` meaning `t0 + c * t1` with t0, t1 per channel (broadcast forms of (1, M, 1, ..))
      and ONE noise-level map c (the same tensor in every triple) that broadcasts to (N, 1, *code grid): the fused kernel's
      map form, `(cmap, slopes)` at the C ABI -- no threshold and no threshold gradient of the codes' size is formed, the
      bits are those of the tensor torch's broadcast `t0 + c * t1` would give;
    * any other tensor that broadcasts to the code shape: analysis followed by prox_csr / prox_csr_f2 (the `_b` form).

    Differentiable in x, w, add, z_prev, z_after and every threshold tensor, each gradient in the shape given."""
    fn = "analysis_prox"
    g = _geometry(fn, tuple(x.shape), w, stride)
    cs = g.code_shape()
    for name, t in (("add", add), ("z_prev", z_prev), ("z_after", z_after)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != cs):
            raise ValueError(f"{fn}: `{name}` of shape {tuple(t.shape)} is not the code shape {cs}")
    if z_prev is None:
        raise ValueError(f"{fn}: z_prev is required (analysis_shrink is the block without a neighbour code)")
    f2 = z_after is not None
    named = [("lambd", lambd), ("gamma1" if f2 else "gamma", gamma1)] + ([("gamma2", gamma2)] if f2 else [])
    if f2 and gamma2 is None:
        raise ValueError(f"{fn}: gamma2 is required with z_after")
    _on_device(fn, x=x, w=w, add=add, z_prev=z_prev, z_after=z_after)
    dev = x.device
    per_channel = (1,) + cs[1:]
    zeros = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.float32)
    if any(_is_map_form(t) for _, t in named):
        if not all(_is_map_form(t) for _, t in named) or any(t[1] is not named[0][1][1] for _, t in named):
            raise ValueError(f"{fn}: with a noise-level map every threshold is a triple (t0, c, t1) with the same map c")
        c = named[0][1][1]
        want = (g.N, 1) + cs[2:]
        shape = (1,) * (len(want) - c.dim()) + tuple(c.shape) if c.dim() <= len(want) else None
        if shape is None or any(a not in (1, b) for a, b in zip(shape, want)):
            raise ValueError(f"{fn}: the map of shape {tuple(c.shape)} does not broadcast to the code grid {want}")
        cmap = c.to(device=dev, dtype=torch.float32).reshape(shape).expand(want).contiguous()
        row = lambda name, t: _threshold(fn, name, t, per_channel, dev, rows_only=True).reshape(-1).expand(g.M)
        thr = [row(name + "[0]", t[0]) for name, t in named] + ([] if f2 else [zeros(g.M)])
        slopes = [row(name + "[2]", t[2]) for name, t in named] + ([] if f2 else [zeros(g.M)])
        return _AnalysisProx.apply(x, w, add, z_prev, z_after, torch.stack(thr).contiguous(),
                                   torch.stack(slopes).contiguous(), cmap, g, float(alpha))
    full = [(name, _threshold(fn, name, t, cs, dev)) for name, t in named]
    if any(any(d != 1 for d in t.shape[2:]) for _, t in full):          # spatial extent: the broadcast form, two launches
        u = analysis(x, w, stride, alpha, add)
        return _prox(fn, u, z_prev, z_after, lambd, gamma1, gamma2 if f2 else None)
    rows = [t.expand(cs[:2] + t.shape[2:]).reshape(cs[:2]) for _, t in full] + ([] if f2 else [zeros(g.N, g.M)])
    return _AnalysisProx.apply(x, w, add, z_prev, z_after, torch.stack(rows).contiguous(), None, None, g, float(alpha))


# ------------------------------------------------------------------------------------------ the whole CSR loop
def ista_csr(y, z_prev, z_after, sigma, mask, t, g1, g2, A, B, stride):
    """The K iterations of a CSR net with neighbour codes and the final synthesis, as ONE autograd node over the one-call
    sweeps (loop.TemporalISTA): returns (xhat, z_K).

    y (N,C,H,W) noisy frame; z_prev, z_after (None: the one-neighbour map prox_CSR, g2 unused) neighbour codes; t, g1, g2 the
    (K,2,M,1,1) threshold parameters; A, B the K analysis / synthesis filters (the final synthesis is B[0]).  sigma: None
    (no noise-adaptive part), a float, one level per sample, or a noise-level map that broadcasts to (N,1,*code grid) --
    classified as the nets classify it (net._noise_scale), with the same ValueErrors; with a map the three threshold
    families t, g1, g2 all follow it, as the reference's broadcast does.  Differentiable in the filters, t, g1, g2, z_prev,
    z_after, y, and sigma (the gradient comes back in the shape sigma was given).  A mask that requires grad raises."""
    from .net import _code_grid, _mask_tensor, _noise_scale
    _no_mask_gradient(mask)
    if z_prev is None:
        raise ValueError("ista_csr: z_prev is required (without a neighbour code the loop is the plain one, loop.run)")
    if y.dim() != 4:
        raise ValueError("ista_csr: expected an (N,C,H,W) frame")
    _on_device("ista_csr", y=y, z_prev=z_prev, z_after=z_after)
    y = y.to(torch.float32)
    c = _noise_scale(sigma, True, y.shape[0], y.device, _code_grid(y.shape[2:], int(stride)))
    mask_t = _mask_tensor(mask.detach() if torch.is_tensor(mask) else mask, y)
    return loop.run_csr(y, mask_t, c, z_prev, z_after, t, g1, g2 if z_after is not None else None, list(A), list(B), int(stride))


# ------------------------------------------------------------------------------------------ pre / post
@loop._arithmetic_aware
class _PreProcess(torch.autograd.Function):
    """(y, mask | None) -> (yp, mean (N,1,..), mask_p | empty)."""

    @staticmethod
    def forward(ctx, y, mask, s):
        yp, mean, pads, mask_p = ops.preprocess(y.contiguous(), s, mask)
        ctx.pads, ctx.shape = pads, tuple(y.shape)
        loop._save(ctx, mask=mask)
        mask_p = mask_p if mask_p is not None else yp.new_empty(0)
        ctx.mark_non_differentiable(mask_p)
        ctx.set_materialize_grads(False)
        return yp, mean.reshape((-1,) + (1,) * (y.dim() - 1)), mask_p

    @staticmethod
    @once_differentiable
    def backward(ctx, g_yp, g_mean, _g_mask):
        mask = loop._saved(ctx).mask
        if g_yp is None and g_mean is None:
            return None, None, None
        pads = ctx.pads
        if g_yp is None:
            nd = len(ctx.shape) - 2
            padded = tuple(d + pads[2 * (nd - 1 - i)] + pads[2 * (nd - 1 - i) + 1] for i, d in enumerate(ctx.shape[2:]))
            g_yp = g_mean.new_zeros(ctx.shape[:2] + padded)
        # cdl_preprocess_bwd takes the mean's path as the per-sample sum of an image-shaped gradient: spread the gradient
        # of the mean evenly (a thin tensor)
        gx = None
        if g_mean is not None:
            per = 1
            for d in ctx.shape[1:]:
                per *= d
            gx = (g_mean / per).expand(ctx.shape).contiguous()
        return ops.preprocess_bwd(g_yp.contiguous(), pads, gx, mask), None, None


@loop._arithmetic_aware
class _PostProcess(torch.autograd.Function):
    """(xp, mean (N,1,..)) -> crop(xp) + mean."""

    @staticmethod
    def forward(ctx, xp, mean, pads):
        ctx.pads = pads
        return ops.postprocess(xp.contiguous(), mean.reshape(-1).contiguous(), pads)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        g_xp = ops.postprocess_bwd(g, ctx.pads) if ctx.needs_input_grad[0] else None
        g_mean = g.sum(dim=tuple(range(1, g.dim())), keepdim=True) if ctx.needs_input_grad[1] else None     # thin
        return g_xp, g_mean, None


def pre_process(y, stride, mask=1):
    """The reference's pre_process / pre_process_3d (model/utils.py:5-22, 70-87): mean subtraction (over the sampled
    pixels with a mask) and reflect padding to a multiple of the stride.  Returns (yp, params, mask_p) with params =
    [mean (N,1,..), pad] for post_process and mask_p the padded mask (1 without one).  Differentiable in y, through yp
    and through the mean."""
    _no_mask_gradient(mask)
    if torch.is_tensor(mask):
        if tuple(mask.shape) != tuple(y.shape):
            mask = torch.broadcast_to(mask, y.shape)
        mask_t = mask.detach().to(torch.float32).contiguous()
    elif mask is None or mask == 1:
        mask_t = None
    else:
        raise ValueError("mask must be 1 (no mask) or a tensor shaped like y")
    if y.dim() not in (4, 5):
        raise ValueError("pre_process: expected (N,C,H,W) or (N,C,D,H,W)")
    _on_device("pre_process", y=y, mask=mask_t)
    yp, mean, mask_p = _PreProcess.apply(y.to(torch.float32), mask_t, int(stride))
    return yp, [mean, ops.stride_pads(y.shape[2:], int(stride))], (mask_p if mask_t is not None else 1)


def post_process(xp, params):
    """The reference's post_process / post_process_3d (model/utils.py:24-33, 89-101): crops the stride padding and adds
    the mean back; like the reference's it pops both from `params`.  Differentiable in xp and in the mean."""
    pads = params.pop()
    mean = params.pop()
    _on_device("post_process", xp=xp, mean=mean)
    return _PostProcess.apply(xp, mean, tuple(pads))
