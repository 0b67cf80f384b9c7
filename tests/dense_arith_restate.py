"""Float64 restatement of the arithmetic of the dense matrix-core tier -- k_dense<MT> and the four k_dense_vgg<MODE> forms with
k_dense_prep, k_dense_wgrad<VEC> with k_dense_wfold (cdl_dense_mfma.hip); DESIGN.md section 39 -- used by
test_dense_arith_cpu.py and test_gpu_dense_cells.py.  The parts, the kept products, the bound, the predicates and the
exactly-summable inputs are fused2d_arith_restate's / generic_arith_restate's, imported unchanged; what this module adds is the
tier's forms, written from the header comments of the file with torch's conv2d/3d and conv_transpose2d/3d in float64:
nothing of the kernels' tiles, fragments, stages or partial banks.

Parts.  Every conversion of the file is the compiler's `(__bf16)float`, round to nearest even: k_dense_prep (the weight
fragments of both roles), the window staging of dense_body (the unpool form included), split8 and the halo elements of
k_dense_wgrad.  hi = (__bf16)x, lo = (__bf16)(x - hi); every k-step is three MFMAs per accumulator tile, lo.hi, hi.lo, hi.hi
("split3").

Geometry.  Unit stride, many channels on both sides, odd rectangular planes up to 5 x 5, any odd Pd, padding P // 2.  The
analysis role maps (N,C,..) to (N,M,..) with the bank (M,C,P); the transposed role is its adjoint with the same bank (the
flipped bank, input and output channels swapped).

Bound.  b = n_e * 2^-23 * S_e (fused2d_arith_restate's docstring): n_e - 1 units for a sum of n_e terms in any order, `add` and
`sub` counted as terms; the n_e-th unit covers the two further roundings of an epilogue (alpha * acc, the shrinkage's
subtraction) at 2^-24 S each.  alpha * acc + add may or may not be contracted into one fma: one rounding or two.  With alpha a
power of two the product is exact and both are the same number; for any other alpha one more unit is added, which admits
either.  mask is 0 / 1 in every caller (exact).  ReLU and a shrinkage with tau >= 0 are 1-Lipschitz, so b carries through them;
a shrinkage with tau < 0 jumps at 0 and is compared only where |u| > b.

Layout of the operands: images (N,C,[D,]H,W); codes (N,M,[D,]H,W); banks (M,C,[Pd,]Ph,Pw); thresholds (N,M)."""
import math

import torch

import generic_arith_restate as G
from fused2d_arith_restate import (EPS, _KEPT, _product, _with_term, bf16_rne, honest_product, parts,  # noqa: F401
                                   violations_fp32, zeros_off_support)
from generic_arith_restate import (CAP_QUANTA, abs_sum, analysis, dtau_sums, exact_cap_ok, exact_inputs,  # noqa: F401
                                   exact_term_quanta, filter_grad, im2col, mismatches, quanta_off, shrink, synthesis,
                                   thresholds)

PRECISION = "split3"


def _pow2(a):
    m, _ = math.frexp(abs(a))
    return m == 0.5


def conv(x, w, transpose=False):
    """The tier's operator at unit stride: A x (the analysis role) or B x (the transposed role, the same bank)."""
    return synthesis(x, w, 1) if transpose else analysis(x, w, 1)


# ------------------------------------------------------------------------------------------------ k_dense / k_dense_vgg
def dense_core(x, w, transpose=False, in_gate=None, kept=None):
    """(value, S, n) of the kept products of conv([in_gate != 0] x): what every form of one (x, w, in_gate) shares."""
    xg = x if in_gate is None else x * (in_gate != 0)
    return _product(lambda a, b: conv(a, b, transpose), parts(xg), parts(w), PRECISION, kept)


def dense_form(x, w, transpose=False, alpha=1.0, in_gate=None, mask=None, add=None, add_gate=None, sub=None, tau=None,
               relu=False, out_gate=None, kept=None, with_u=False, core=None):
    """k_dense's epilogue, in the order of its header comment:
        v = alpha conv([in_gate != 0] x);  v *= mask;  v += add [where add_gate != 0];  v -= sub;  v = ST(v, tau[n,m]);
        v = max(v, 0);  v = 0 where out_gate == 0
    (value, b), and with_u (value, b, u): u the value in front of the shrinkage.  core: dense_core of the same operands."""
    val, S, n = dense_core(x, w, transpose, in_gate, kept) if core is None else core
    val, S = alpha * val, abs(alpha) * S
    if mask is not None:
        m = mask.double()
        val, S, n = m * val, m.abs() * S, n * (m != 0)
    if add is not None:
        val, S, n = _with_term(val, S, n, add if add_gate is None else add * (add_gate != 0))
    val, S, n = _with_term(val, S, n, sub, -1.0)
    b = (n + (0 if _pow2(alpha) else 1)) * EPS * S
    u = val
    if tau is not None:
        val = shrink(val, thresholds(tau, val))
    if relu:
        val = val.clamp_min(0.0)
    if out_gate is not None:
        on = out_gate != 0
        val, b = val * on, b * on
    return (val, b, u) if with_u else (val, b)


def _bias_like(bias, like):
    return bias.reshape((1, -1) + (1,) * (like.dim() - 2)).expand(like.shape)


def vgg_bias(x, w, bias, core=None):
    """DM_BIAS: relu(conv(x) + bias[o]); (value, b)."""
    c = dense_core(x, w) if core is None else core
    return dense_form(x, w, add=_bias_like(bias, c[0]), relu=True, core=c)


def pool_first_max(h):
    """The 2 x 2 stride-2 floor-mode max-pool of h (..., H, W), in h's dtype: (pooled, codes uint8).  The code is the
    position 0..3 of the maximum in row-major order in the window; the first maximum wins a tie."""
    H, W = h.shape[-2:]
    Hp, Wp = H // 2, W // 2
    v = h[..., :2 * Hp, :2 * Wp].reshape(h.shape[:-2] + (Hp, 2, Wp, 2)).transpose(-3, -2).reshape(h.shape[:-2] + (Hp, Wp, 4))
    mx = v[..., 0].clone()
    code = torch.zeros(mx.shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        better = v[..., k] > mx
        mx = torch.where(better, v[..., k], mx)
        code = torch.where(better, torch.full_like(code, k), code)
    return mx, code


def vgg_pool(x, w, bias, core=None):
    """DM_POOL: the pool of vgg_bias; (value, b, codes).  A maximum is 1-Lipschitz in the sup norm, so the bound of a
    pooled element is the largest bound in its window (the codes are those of the MODEL's values: a device whose values
    differ inside b may pick another element of a near-tied window)."""
    val, b = vgg_bias(x, w, bias, core)
    pooled, codes = pool_first_max(val)
    return pooled, pool_first_max(b)[0], codes


def vgg_diff(fx, fy):
    """DM_DIFF from the two feature tensors, in their dtype: d = fx - fy, the seeds d [fx > 0] and d [fy > 0], and the
    float64 sum of d^2; (d, seed_x, seed_y, sum)."""
    d = fx - fy
    zero = torch.zeros_like(d)
    return d, torch.where(fx > 0, d, zero), torch.where(fy > 0, d, zero), float((d.double() ** 2).sum())


def unpool_place(gp, codes, H, W):
    """A pooled gradient (..., H//2, W//2) placed at its argmax codes in (..., H, W); a dropped odd row or column gets
    nothing."""
    Hp, Wp = gp.shape[-2:]
    out = torch.zeros(gp.shape[:-2] + (H, W), dtype=gp.dtype)
    for k in range(4):
        out[..., k // 2:2 * Hp:2, k % 2:2 * Wp:2] = torch.where(codes == k, gp, torch.zeros_like(gp))
    return out


def vgg_unpool(gp, codes, w, H, W, out_gate=None):
    """DM_UNPOOL: the transposed convolution of the placed gradient, then the output gate; (value, b)."""
    return dense_form(unpool_place(gp, codes, H, W), w, transpose=True, out_gate=out_gate)


# ------------------------------------------------------------------------------------------------ k_dense_wgrad + k_dense_wfold
def wgrad_form(Fc, x, P, alpha=1.0, gate=None, kept=None):
    """alpha * ([gate != 0] G) (x) im2col(x) for 3 x 3 planes and any odd Pd; (value (M,C,*P), b)."""
    return G.wgrad_form(Fc, x, P, 1, alpha, gate, kept)


def wgrad_value(Fc, x, P, alpha=1.0, gate=None):
    return G.wgrad_value(Fc, x, P, 1, alpha, gate)


WTX, WTY, WG_TOTAL = 32, 4, 255


def wgrad_plan(N, C, M, D, H, W, Pd):
    """wgrad_plan of cdl_dense_mfma.hip restated: None where the tier refuses, otherwise a dict with the tile grid, the
    tile count, the workgroups per (kd, channel group), the channel groups, and per kd the tiles that are depth-valid."""
    if not (16 <= C <= 64 and M >= 16 and Pd % 2 == 1):
        return None
    tx, ty = -(-W // WTX), -(-H // WTY)
    nt = N * D * tx * ty
    if nt < 8:
        return None
    og = -(-M // 64)
    nwg = WG_TOTAL // (Pd * og)
    if nwg >= 8:
        nwg &= ~7
    nwg = min(max(nwg, 1), nt)
    valid = [sum(1 for t in range(nt) if 0 <= (t // (tx * ty)) % D + kd - Pd // 2 < D) for kd in range(Pd)]
    walked = [max(sum(1 for t in range(wg, nt, nwg) if 0 <= (t // (tx * ty)) % D + kd - Pd // 2 < D) for wg in range(nwg))
              for kd in range(Pd)]
    return dict(tilesX=tx, tilesY=ty, ntiles=nt, nwg=nwg, ogroups=og, valid=valid, walked=walked, vec=W % 4 == 0,
                narrow=[C <= 32 and M - 64 * g <= 32 for g in range(og)])


# ------------------------------------------------------------------------------------------------ test content
def stage_inputs(N, C, M, P, sp, seed, tau_sign_mixed=False):
    """generic_arith_restate's data recipe at unit stride, with an image-shaped sparse gate (`igate`) and add (`x2`)."""
    d = G.stage_inputs(N, C, M, P, sp, 1, seed, tau_sign_mixed)
    gen = torch.Generator().manual_seed(seed + 77)
    ish = (N, C) + tuple(sp)
    d["igate"] = torch.randn(ish, generator=gen) * (torch.rand(ish, generator=gen) < 0.3)
    return d
