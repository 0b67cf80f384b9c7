"""Float64 restatement of the arithmetic of the sparse matrix-core tier -- k_ana_m (cdl_analysis_mfma.hip), k_synth_m with its
assembles (cdl_synth_mfma.hip) and k_wgm with k_wgm_fold (cdl_wgrad_mfma.hip); DESIGN.md section 35 -- used by
test_generic_arith_cpu.py and test_gpu_generic_cells.py.  The parts, the kept products, the bound and the acceptance
predicates are fused2d_arith_restate's, imported unchanged; what this module adds is the tier's operators and epilogues,
written from the definitions in the three kernels' header comments with torch's conv* / conv_transpose* (and one matrix
product over an im2col written out here) in float64: nothing of the kernels' tiles, fragments, patches or partial banks.

Parts.  Every conversion of the three files is the compiler's `(__bf16)float`, round to nearest even: k_ana_prep and the
plane staging of k_ana_m; k_synth_prep and both code splits of k_synth_m (registers, KSM = 4; per k-step, KSM = 0); st_write /
pack_bf16, the stride-2 staging and both fat splits (kstep, the slow path) of k_wgm.  hi = (__bf16)x, lo = (__bf16)(x - hi);
the kept products are hi.hi + hi.lo + lo.hi ("split3") in all three.

Geometry.  Stride s on ALL spatial axes, depth included (cdl_geom's sd follows s in every net); padding P // 2 per axis;
output_padding = s - 1; rectangular planes: the shipped 9 x 9 x 5 bank is P = (Pd, Ph, Pw) = (9, 9, 5), nine depth taps of
9 x 5 planes.

Bound.  b = n_e * 2^-23 * S_e elementwise, derived in fused2d_arith_restate's docstring for a sum taken in ANY order.  It is loose
for the long sums of this tier (the filter gradients add N * Dz * Hz * Wz terms per element, the synthesis M * taps / s^nd):
`exact_inputs` is the second instrument -- operands on which every partial sum in every order is an fp32 number, so that a
correct kernel equals the model bit for bit.

Layout of the operands: images (N,C,[D,]H,W); codes (N,M,[D/s,]H/s,W/s); banks (M,C,[Pd,]Ph,Pw); thresholds (N,M); cmap
(N,1,*code spatial); tslope (M) or (3,M); all float32 CPU tensors.
"""
import torch
import torch.nn.functional as F

import fused2d_arith_restate as R2
from fused2d_arith_restate import (EPS, _KEPT, _product, _with_term, bf16_rne, honest_product, parts,  # noqa: F401
                                   violations_fp32, zeros_off_support)

PRECISION = "split3"                        # the one arithmetic of this tier


# ------------------------------------------------------------------------------------------------ operators
def _geometry(w, s):
    """(stride, padding, output_padding) per axis of a bank (M,C,[Pd,]Ph,Pw): stride s on every spatial axis."""
    nd = w.dim() - 2
    return (s,) * nd, tuple(p // 2 for p in w.shape[2:]), (s - 1,) * nd


def analysis(x, w, s=1):
    """A x: (N,C,[D,]H,W) x (M,C,[Pd,]Ph,Pw) -> (N,M,[D/s,]H/s,W/s); out[m][z] = sum_{c,k} w[m][c][k] x[c][s z - P/2 + k]."""
    stride, pad, _ = _geometry(w, s)
    return (F.conv2d if w.dim() == 4 else F.conv3d)(x, w, stride=stride, padding=pad)


def synthesis(z, w, s=1):
    """B z: the adjoint of `analysis` with the same bank, output_padding = s - 1 on every axis."""
    stride, pad, opad = _geometry(w, s)
    return (F.conv_transpose2d if w.dim() == 4 else F.conv_transpose3d)(z, w, stride=stride, padding=pad, output_padding=opad)


def im2col(x, P, s=1):
    """(N, C, taps, code pixels) with [n][c][k][z] = x[n][c][s z - P/2 + k] (zero outside the image), taps and pixels in
    row-major order of ([Pd,]Ph,Pw) and of the code grid."""
    nd = len(P)
    pad = [q for p in reversed(P) for q in (p // 2, p // 2)]
    xp = F.pad(x, pad)
    Z = [d // s for d in x.shape[2:]]
    cols = []
    for k in range(int(torch.tensor(P).prod())):
        idx, r = [], k
        for p in reversed(P):
            idx.append(r % p)
            r //= p
        idx = idx[::-1]
        sl = (slice(None), slice(None)) + tuple(slice(idx[a], idx[a] + s * Z[a], s) for a in range(nd))
        cols.append(xp[sl].reshape(x.shape[0], x.shape[1], -1))
    return torch.stack(cols, dim=2)


def filter_grad(Fc, x, P, s=1):
    """F (x) im2col(x): (N,M,*code) x (N,C,*image) -> (M,C,*P); out[m][c][k] = sum_{n,z} F[n][m][z] x[n][c][s z - P/2 + k]."""
    col = im2col(x, tuple(P), s)                                             # (N, C, T, Z)
    N, C, T, Z = col.shape
    out = Fc.reshape(N, Fc.shape[1], Z).transpose(0, 1).reshape(Fc.shape[1], N * Z) @ col.permute(0, 3, 1, 2).reshape(N * Z, C * T)
    return out.reshape((Fc.shape[1], C) + tuple(P))


def _flat(x):
    """A code tensor with its depth folded into its rows, (N,M,D*H,W): what the 2-D module's elementwise helpers take."""
    return x.reshape(x.shape[0], x.shape[1], -1, x.shape[-1])


def _rows(t, like):
    """A per-(sample, channel) or per-channel row broadcast over the code grid of `like`."""
    return t.reshape(t.shape + (1,) * (like.dim() - t.dim()))


def thresholds(tau, like, cmap=None, tslope=None):
    """The thresholds of an epilogue as the kernels form them, in float32 (cdl_map_threshold: the product is rounded, then
    the sum): tau[n,m], or tau[n,m] + cmap[n,pix] * tslope[m]; returned as float64, broadcastable to the codes."""
    t = _rows(tau.float(), like)
    if cmap is not None:
        t = t + cmap.float() * tslope.float().reshape((1, -1) + (1,) * (like.dim() - 2))
    return t.double()


def shrink(u, thr):
    """ST(u, t) = sign(u) relu(|u| - t) (cdl_shrink): for t >= 0 the clamp form u - clamp(u, -t, t) and 1-Lipschitz; for
    t < 0 it jumps by 2 |t| at u = 0 and is 1-Lipschitz on either side."""
    return torch.sign(u) * (u.abs() - thr).clamp_min(0.0)


def dtau_sums(du, on, neg, c):
    """(dt (2,M), b) of a reverse step from ITS output: dt[0][m] = sum -sign(zsup) du, dt[1][m] = sum_n c[n] (the same over
    sample n); fused2d_arith_restate.dtau_sums."""
    return R2.dtau_sums(_flat(du), _flat(on), _flat(neg), c)


def dtau_sums_map(du, on, neg, cmap):
    """The map form (k_ana_m<REV, MAP>, k_ana_tau_final<true>): dt[0] as above, dt[1][m] = sum_{n,pix} cmap[n,pix] t[n,m,pix]
    with t = -sign(zsup) du, each term one fma into the running sum; (dt (2,M), b)."""
    d = du.double()
    t = torch.where(neg, d, -d) * on
    cm = cmap.double()
    dims = (0,) + tuple(range(2, d.dim()))
    nz = ((d != 0) & on).double()
    dt = torch.stack([t.sum(dim=dims), (cm * t).sum(dim=dims)])
    S = torch.stack([t.abs().sum(dim=dims), (cm.abs() * t.abs()).sum(dim=dims)])
    n = torch.stack([nz.sum(dim=dims), (nz * (cm != 0)).sum(dim=dims) + 1])
    return dt, n * EPS * S


# ------------------------------------------------------------------------------------------------ the forms of the kernels
def analysis_core(x, w, s=1, kept=None):
    """(value, S, n) of the kept products of A x: what every form of one (x, w) shares (the costly part of the model)."""
    return _product(lambda a, b: analysis(a, b, s), parts(x), parts(w), PRECISION, kept)


def analysis_form(x, w, s=1, alpha=1.0, zin=None, gate=None, tau=None, cmap=None, tslope=None, zsup=None, kept=None,
                  with_u=False, core=None):
    """k_ana_m: base = zin ? (gate ? [gate != 0] zin : zin) : 0, u = base + alpha acc, then
        plain u | ST(u, tau[n,m]) | ST(u, tau + cmap tslope) | reverse [zsup != 0] u
    (value, b), and with_u (value, b, u): the pre-shrinkage value the CSR epilogues and the sign-mixed comparison need.
    core: analysis_core(x, w, s) computed once for several forms.
    alpha is a power of two in every caller (exact); u = fma(alpha, acc, base) is one rounding, which the n-th unit covers."""
    val, S, n = analysis_core(x, w, s, kept) if core is None else core
    val, S = alpha * val, abs(alpha) * S
    if zin is not None:
        base = zin if gate is None else zin * (gate != 0)
        val, S, n = _with_term(val, S, n, base)
    b = n * EPS * S
    u = val
    if zsup is not None:
        on = (zsup != 0)
        val, b = val * on, b * on
    elif tau is not None:
        val = shrink(val, thresholds(tau, val, cmap, tslope))
    return (val, b, u) if with_u else (val, b)


def synth_form(z, w, s=1, gate=None, mask=None, sub=None, alpha=1.0, kept=None):
    """k_synth_m + k_synth_assemble[4]: mask * alpha * B([gate != 0] z) - sub; (value, b).  alpha = +-1 in every caller."""
    zg = z if gate is None else z * (gate != 0)
    val, S, n = _product(lambda a, b: synthesis(a, b, s), parts(zg), parts(w), PRECISION, kept)
    m = 1.0 if mask is None else mask.double()
    val, S, n = m * alpha * val, m * abs(alpha) * S, m * n
    val, S, n = _with_term(val, S, n, sub, -1.0)
    return val, n * EPS * S


def wgrad_value(Fc, x, P, s=1, alpha=1.0, gate=None):
    """The value of wgrad_form without its bound (a third of the work): what an exact-input comparison needs."""
    a, b = parts(Fc if gate is None else Fc * (gate != 0)), parts(x)
    return alpha * sum(filter_grad(a[i], b[j], P, s) for (i, j) in _KEPT[PRECISION])


def wgrad_form(Fc, x, P, s=1, alpha=1.0, gate=None, kept=None):
    """k_wgm + k_wgm_fold: alpha * ([gate != 0] F) (x) im2col(x); (value (M,C,*P), b).  The pair is two of these."""
    Fg = Fc if gate is None else Fc * (gate != 0)
    val, S, n = _product(lambda a, b: filter_grad(a, b, P, s), parts(Fg), parts(x), PRECISION, kept)
    return alpha * val, (n + 1) * EPS * abs(alpha) * S


# ---- the CSR epilogue (cdl_prox_csr1 / cdl_prox_csr2 of cdl_common.h), pointwise in float32 with the reference's order of
# operations (contraction off): applied to the DEVICE's own u it must reproduce the device's z value for value.
def _st32(x, t):
    return torch.sign(x) * (x.abs() - t).clamp_min(0.0)


def prox_csr32(u, zp, lam, g1, za=None, g2=None):
    """prox_CSR (za None) / prox_CSR_f2, every operand float32 and broadcastable to u."""
    assert u.dtype == torch.float32
    sg = torch.sign
    if za is None:
        s_ = sg(zp)
        ls = lam * s_
        a = (u - zp) - ls
        tg = g1 * lam
        m = (_st32(a, tg) + zp) + ls
        return _st32(m, lam)
    l1, l2 = lam * g1, lam * g2
    ca = (zp + lam * sg(zp)) + l2 * sg(zp - za)
    cb = (za + lam * sg(za)) + l1 * sg(za - zp)
    a = u - ca
    sa = sg(a)
    b = (_st32(a, g1 * lam) - cb) + l1 * sa
    m = (_st32(b, g2 * lam) + cb) - l1 * sa
    return _st32(m, lam)


def prox_thresholds32(lam, g1, g2, like, cmap=None, tslope=None):
    """The (lam, gam1, gam2) of cdl_prox_apply / cdl_prox_apply_map in float32, broadcastable to the codes; tslope (3,M)."""
    out = []
    for i, t in enumerate((lam, g1, g2)):
        if t is None:
            out.append(None)
            continue
        r = _rows(t.float(), like)
        if cmap is not None:
            r = r + cmap.float() * tslope.float()[i].reshape((1, -1) + (1,) * (like.dim() - 2))
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ acceptance
def mismatches(got, model):
    """Number of elements that are NOT equal in value to the model (a NaN is a mismatch; -0 equals +0)."""
    return int((~(got.double() == model.double())).sum())


def quanta_off(got, model, quantum):
    """(mismatching elements, largest |got - model| in quanta) of an exact-input comparison."""
    err = (got.double() - model.double()).abs() / quantum
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
    return int((err != 0).sum()), float(err.max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ test content
def code_shape(N, M, sp, s):
    return (N, M) + tuple(d // s for d in sp)


def stage_inputs(N, C, M, P, sp, s, seed, tau_sign_mixed=False):
    """The data recipe of the cell tests: P the filter extents ([Pd,]Ph,Pw), sp the image extents ([D,]H,W), s the stride.  A
    dict of float32 CPU tensors: x, x2, sub, w, w2, z / F (sparse codes), u (dense code), gate (sparse), tau (positive, or
    sign-mixed), c, cmap, tslope, tslope3, mask, and the CSR operands zp, za, lam, g1, g2."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.randn(sh, generator=gen)
    ish, csh, fsh = (N, C) + tuple(sp), code_shape(N, M, sp, s), (M, C) + tuple(P)
    d = dict(x=rnd(*ish), x2=rnd(*ish), sub=rnd(*ish), w=0.1 * rnd(*fsh), w2=0.1 * rnd(*fsh))
    d["z"] = rnd(*csh) * (torch.rand(csh, generator=gen) < 0.4)
    d["u"] = rnd(*csh)
    d["gate"] = rnd(*csh) * (torch.rand(csh, generator=gen) < 0.3)
    d["tau"] = 0.3 * torch.rand(N, M, generator=gen)
    if tau_sign_mixed:
        d["tau"] = d["tau"] - 0.1
    d["c"] = torch.rand(N, generator=gen)
    d["cmap"] = torch.rand((N, 1) + csh[2:], generator=gen)
    d["tslope"] = 0.2 * torch.rand(M, generator=gen)
    d["tslope3"] = 0.2 * torch.rand(3, M, generator=gen)
    d["mask"] = (torch.rand(ish, generator=gen) < 0.5).float()
    d["zp"] = 0.3 * rnd(*csh) * (torch.rand(csh, generator=gen) < 0.5)
    d["za"] = 0.3 * rnd(*csh) * (torch.rand(csh, generator=gen) < 0.5)
    d["lam"] = 0.2 * torch.rand(N, M, generator=gen) + 0.01
    d["g1"] = 1.2 * torch.rand(N, M, generator=gen) + 0.01
    d["g2"] = 1.2 * torch.rand(N, M, generator=gen) + 0.01
    return d


CAP_QUANTA = 2.0 ** 21        # per output element, the sum of the absolute kept products in quanta (2^24 is what fp32 needs)


def _exact_operand(shape, density, integer, gen):
    """Values whose parts are hi in {0, +-1} with lo in {0, +-2^-9} (x = +-1, +-(1 + 2^-9), +-(1 - 2^-9): the last is a tie that
    round-to-nearest-EVEN resolves to hi = 1), or integers {0, +-1, +-2} with no lo part."""
    on = torch.rand(shape, generator=gen) < density
    sg = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    if integer:
        mag = torch.randint(1, 3, shape, generator=gen).float()
    else:
        mag = 1.0 + (torch.randint(0, 3, shape, generator=gen).float() - 1.0) * 2.0 ** -9
    return sg * mag * on


def exact_inputs(N, C, M, P, sp, s, seed, integer=False, density=(0.5, 0.25, 0.25), only=None):
    """Exactly-summable operands of a geometry: x, x2 (images, density[0]), w, w2 (banks, density[1]), z, u, gate (codes,
    density[2]; u dense, gate half) and F, F2: codes for the filter gradient with ONE non-zero channel per code pixel
    (density 1 / M, order 1 %: every code pixel of every tile is hit).  `quantum`: 2^-9, or 1 for the integer-only variant.
    Under the cap (`exact_cap_ok`) every partial sum of kept products in every order is a multiple of the quantum below
    2^24 quanta, so an fp32 accumulation is exact.  only: the names wanted (each tensor has a generator of its own, so a
    subset is the same data)."""
    ish, csh, fsh = (N, C) + tuple(sp), code_shape(N, M, sp, s), (M, C) + tuple(P)
    recipe = dict(x=(ish, density[0]), x2=(ish, density[0]), w=(fsh, density[1]), w2=(fsh, density[1]), z=(csh, density[2]),
                  u=(csh, 1.0), gate=(csh, 0.5), F=None, F2=None)
    d = dict(quantum=1.0 if integer else 2.0 ** -9)
    for i, (k, r) in enumerate(recipe.items()):
        if only is not None and k not in only:
            continue
        gen = torch.Generator().manual_seed(1000 * seed + i)
        if r is not None:
            d[k] = _exact_operand(r[0], r[1], integer, gen)
        else:
            ch = torch.randint(0, M, (N, 1) + csh[2:], generator=gen)
            d[k] = torch.zeros(csh).scatter_(1, ch, _exact_operand((N, 1) + csh[2:], 1.0, integer, gen))
    return d


def exact_term_quanta(integer):
    """Upper bound, in quanta, of |hi.hi| + |hi.lo| + |lo.hi| of one term a * b of two exact operands: (1 + 2 2^-9) / 2^-9,
    or 2 * 2 for the integers."""
    return 4.0 if integer else 514.0


def exact_cap_ok(S, quantum):
    """The summability condition on a model's S_e (the bound b divided by n_e 2^-23 is not kept, so callers pass the abs
    sum itself): max S_e / quantum < 2^21."""
    return float(S.max()) / quantum < CAP_QUANTA


def abs_sum(op, a32, b32, kept=None):
    """S_e of op(a, b): the same operator over the absolute values of the kept parts (what `_product` returns second)."""
    return _product(op, parts(a32), parts(b32), PRECISION, kept)[1]
