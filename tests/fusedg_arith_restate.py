"""Float64 restatement of the arithmetic of the fused generic tier -- the tile kernel k_stage_g (cdl_fusedg.hip), the grouped
strip kernel k_stripg (cdl_stripg.hip) and the strip kernel k_strip (cdl_strip.hip) with their assembles (DESIGN.md section
33) -- used by test_fusedg_arith_cpu.py and test_gpu_fusedg_cells.py.  The parts, the kept products, the bound and the
acceptance predicates are fused2d_arith_restate's, imported; what this module adds is the operators of this tier's
geometries (C > 1, depth taps, stride 2), written from the definitions (oracle/cdl_oracle.py `analysis` / `synthesis`) with
torch's conv* / conv_transpose* in float64: nothing of the kernels' tiles, strips, segments, rings or patch sums.

Parts.  The three kernels split the filter banks (k_prep_g, k_prep_s), the thin rows they stage and the accumulator tiles in
front of the synthesis product as hi = (__bf16)x, lo = (__bf16)(x - hi), every conversion round-to-nearest-even; three products
hi.hi + hi.lo + lo.hi are kept ("split3"), four by the tile kernel's FOUR instances ("split4").

Bound.  b = n_e * 2^-23 * S_e elementwise, as in the 2-D module (its docstring has the derivation): S_e the same operator on
the absolute values of the parts (plus |base|, |sub|), n_e the same operator on the non-zero indicators.  The derivation
assumes no summation order, so it covers the DPP chains of the col2im, the register rings, the fixed-order patch sums of the
assembles, and the sgn * zin that the strip kernels preload into the accumulator.

Layout of the operands: images r, thin, mask, sub (N,C,[D,]H,W); codes (N,M,[D,]Hz,Wz) with Hz = H / s, Wz = W / s; filter
banks (M,C,[Pd,]P,P); tau (N,M); c (N); all float32 CPU tensors.  `s` is the stride in the plane (1 in depth).
"""
import torch
import torch.nn.functional as F

import fused2d_arith_restate as R2
from fused2d_arith_restate import (EPS, _KEPT, _product, _with_term, bf16_rne, honest_product, parts,  # noqa: F401
                                   violations_bf16, violations_fp32, zeros_off_support)

PRECISIONS = ("split3", "split4")           # the arithmetics the tier's entry points accept (the tile kernel: both)


# ------------------------------------------------------------------------------------------------ operators
def _geometry(w, s):
    """(stride, padding, output_padding) per axis of a bank (M,C,[Pd,]P,P): stride s in the plane, 1 in depth."""
    nd = w.dim() - 2
    stride = (1,) * (nd - 2) + (s, s)
    return stride, tuple(p // 2 for p in w.shape[2:]), tuple(st - 1 for st in stride)


def analysis(r, w, s=1):
    """A r: (N,C,[D,]H,W) x (M,C,[Pd,]P,P) -> (N,M,[D,]H/s,W/s), the strided correlation of the reference."""
    stride, pad, _ = _geometry(w, s)
    return (F.conv2d if w.dim() == 4 else F.conv3d)(r, w, stride=stride, padding=pad)


def synthesis(z, w, s=1):
    """B z: (N,M,[D,]Hz,Wz) x (M,C,[Pd,]P,P) -> (N,C,[D,]s Hz,s Wz): the adjoint of `analysis`, output_padding = s - 1."""
    stride, pad, opad = _geometry(w, s)
    return (F.conv_transpose2d if w.dim() == 4 else F.conv_transpose3d)(z, w, stride=stride, padding=pad, output_padding=opad)


def _flat(x):
    """A code tensor with its depth folded into its rows, (N,M,D*H,W): what the 2-D module's elementwise helpers take."""
    return x.reshape(x.shape[0], x.shape[1], -1, x.shape[-1])


def shrink(u, tau):
    return R2.shrink(_flat(u), tau).reshape(u.shape)


def dtau_sums(du, on, neg, c):
    """The threshold-gradient sums of a reverse stage from ITS du: (dt (2,M), b); fused2d_arith_restate.dtau_sums."""
    return R2.dtau_sums(_flat(du), _flat(on), _flat(neg), c)


# ------------------------------------------------------------------------------------------------ operations
def forward_stage(r, wA, tau, base, sgn, precision, kept=None, s=1):
    """First / forward stage z' = ST(base + sgn A r, tau): (z', b).  base None: the first stage."""
    val, S, n = _product(lambda a, b: analysis(a, b, s), parts(r), parts(wA), precision, kept)
    u, S, n = _with_term(sgn * val, S, n, base)
    return shrink(u, tau), n * EPS * S


def reverse_stage(thin, w1, on, base, precision, kept=None, s=1):
    """Reverse stage du = [on] (base + corr(thin; w1)): (du, b).  `on` (bool, as the codes): the support bit of the map."""
    val, S, n = _product(lambda a, b: analysis(a, b, s), parts(thin), parts(w1), precision, kept)
    val, S, n = _with_term(val, S, n, base)
    return val * on, n * EPS * S * on


def synth_assemble(z, wB, precision, blk16=False, mask=None, sub=None, alpha=1.0, kept=None, s=1):
    """The synthesis half with fusedg_assemble's arguments: mask * alpha * (B z) - sub at image resolution; (value, b).
    alpha is +-1 in every caller (exact)."""
    val, S, n = _product(lambda a, b: synthesis(a, b, s), parts(z, blk16), parts(wB), precision, kept)
    m = 1.0 if mask is None else mask.double()
    val, S, n = m * alpha * val, m * abs(alpha) * S, m * n
    val, S, n = _with_term(val, S, n, sub, -1.0)
    return val, n * EPS * S


# ------------------------------------------------------------------------------------------------ test content
def bayer_mask(N, H, W):
    """The RGGB mosaic as an (N,3,H,W) float mask: one colour per pixel."""
    m = torch.zeros(N, 3, H, W)
    m[:, 0, 0::2, 0::2] = 1
    m[:, 1, 0::2, 1::2] = 1
    m[:, 1, 1::2, 0::2] = 1
    m[:, 2, 1::2, 1::2] = 1
    return m


def stage_inputs(N, C, M, P, sp, s, seed, bayer=False):
    """The data recipe of the cell tests for a geometry of this tier: P the filter extents ([Pd,]P,P), sp the image extents
    ([D,]H,W), s the stride in the plane.  A dict of float32 CPU tensors (r, thin, sub, wA, wB, zin sparse, base, gate
    sparse, tau, c, mask: random, or the Bayer mosaic of a C = 3 plane)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.randn(sh, generator=gen)
    ish = (N, C) + tuple(sp)
    csh = (N, M) + tuple(sp[:-2]) + (sp[-2] // s, sp[-1] // s)
    fsh = (M, C) + tuple(P)
    d = dict(r=rnd(*ish), thin=rnd(*ish), sub=rnd(*ish), wA=0.1 * rnd(*fsh), wB=0.1 * rnd(*fsh))
    d["zin"] = rnd(*csh) * (torch.rand(csh, generator=gen) < 0.4)
    d["base"] = rnd(*csh)
    d["gate"] = rnd(*csh) * (torch.rand(csh, generator=gen) < 0.3)
    d["tau"] = 0.3 * torch.rand(N, M, generator=gen)
    d["c"] = torch.rand(N, generator=gen)
    if bayer:
        assert C == 3 and len(sp) == 2
        d["mask"] = bayer_mask(N, *sp)
    else:
        d["mask"] = (torch.rand(ish, generator=gen) < 0.5).float()
    return d


def crafted_split4_inputs(N, C, M, P, sp, seed):
    """fused2d_arith_restate.crafted_split4_inputs for G = C * Pd groups: (r (N,C,[D,]H,W), w (M,C,[Pd,]P,P)) with every
    element x = hi (1 + 2^-9), hi a bf16 value with a random 8-bit significand (x is an fp32 value and splits back into exactly
    hi and lo = 2^-9 hi), and one tap per filter, drawn over (group, i, j): an output element is ONE tap's four products, so
    n_e <= 4 and b <= 4 * 2^-23 |x w| against lo . lo = 2^-18 |x w|, a factor of 7.9."""
    gen = torch.Generator().manual_seed(seed)

    def operand(*shape):
        sig = torch.randint(129, 256, shape, generator=gen).double()          # 8 bits, never a power of two
        ex = torch.randint(-3, 2, shape, generator=gen)
        sg = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        hi = sg * torch.ldexp(sig, ex - 8)
        x = (hi * (1 + 2.0 ** -9)).float()
        assert torch.equal(x.double(), hi * (1 + 2.0 ** -9))
        return x

    r = operand(N, C, *sp)
    w = torch.zeros((M, C) + tuple(P))
    taps = w[0].numel()
    tap = torch.randint(0, taps, (M,), generator=gen)
    w.view(M, taps)[torch.arange(M), tap] = 0.25 * operand(M)
    return r, w


# ------------------------------------------------------------------------------------------------ exactly-summable stages
# the three recipes of fused2d_arith_restate (its comment has them) at this tier's geometries.  The
# generator, the cap and the quantum rules are generic_arith_restate's and the 2-D module's, imported; what is added is the
# shapes (C > 1, depth, stride 2), the Bayer mosaic and this module's operators.
from generic_arith_restate import CAP_QUANTA, _exact_operand, exact_cap_ok, exact_inputs, exact_term_quanta  # noqa: E402,F401
from fused2d_arith_restate import (EXACT_HELD, RECIPES, cap_quanta, exact_stage_operands, hi_only,  # noqa: E402,F401
                                   operand_quantum, product_quantum, violations_exact)


def exact_stage_inputs(recipe, precision, N, C, M, P, sp, s, seed, first=False, bayer=False):
    """The exact operands of one stage of a geometry of this tier (stage_inputs' arguments): fused2d_arith_restate's
    exact_stage_operands, the mask the Bayer mosaic where the cell has it."""
    ish = (N, C) + tuple(sp)
    csh = (N, M) + tuple(sp[:-2]) + (sp[-2] // s, sp[-1] // s)
    e = exact_stage_operands(recipe, precision, ish, csh, (M, C) + tuple(P), seed, first)
    if bayer:
        assert C == 3 and len(sp) == 2
        e["mask"] = bayer_mask(N, *sp)
    return e


def exact_stage_model(mode, e, precision, s=1, masked=True):
    """{output: (value, S_e, quantum)}: fused2d_arith_restate.exact_stage_model with this module's strided operators; mode
    first | fwd | bwd | bwd0.  masked False: the assemble runs without a mask."""
    return R2.exact_stage_model(mode, e, precision, masked=masked,
                                ops=(lambda a, b: analysis(a, b, s), lambda a, b: synthesis(a, b, s)))
