"""Float64 restatement of the three arithmetics of the fused 2-D kernels (cdl_fused2d.hip), used by
test_fused2d_arith_cpu.py and test_gpu_fused_cells.py.  Written from the definitions, in plain torch on the CPU: parts by a
rounding written out here, operators by torch's conv2d / conv_transpose2d in float64, nothing of the kernels' loop structure.

Parts.  An fp32 operand x enters a matrix product as hi = bf16_rne(x) and lo = bf16_rne(x - hi); x - hi is exact in fp32.
Every conversion the kernels make (prep_one for the filter banks, store_run_copies and k_wgrad2d's thin_write for the thin
tiles, the hi / lo splits of the accumulator registers in front of the synthesis GEMM and of the dA_k product, bf16_round of
a code stored as bf16) is the compiler's `(__bf16)float`, which is round-to-nearest-even on gfx950: none truncates, so one
rounding serves all.  An operand read from a bf16-stored buffer, or rounded for one (the stage rounds z' / du before it
feeds the synthesis GEMM, the map and the dA_k product when its output is bf16-stored), has no lo part.

Kept products of a x b:   bf16  hi.hi      split3  hi.hi + hi.lo + lo.hi      split4  hi.hi + hi.lo + lo.hi + lo.lo
A product of two bf16 values is exact in fp32, so the only error of a kernel that implements the definition is that of its
fp32 additions.

Bound.  Every operation returns (value, b) with b = n_e * 2^-23 * S_e elementwise: S_e the same sum over the absolute values
of the parts (plus |base|, |sub|), n_e the number of non-zero terms added into the element (the same operator on the
operands' non-zero indicators).  A sum of n terms taken in ANY order, with adds that round within one ulp (2^-23 = twice fp32's
unit roundoff: matrix-core adds need not round to nearest), is within (n - 1) 2^-23 S of the exact sum; the one or two
further fp32 operations of an epilogue (u = fma(sgn, acc, base), the shrinkage's subtraction, alpha * sum, - sub) each add
at most 2^-24 S, which the n-th unit covers.  The shrinkage is 1-Lipschitz, so the bound of u holds for ST(u, tau).

Layout of the operands: r, thin, T (N,1,H,W); codes (N,M,H,W); filter banks (M,1,P,P); tau (N,M); all float32 CPU tensors.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -23
PRECISIONS = ("split3", "bf16", "split4")
_KEPT = {"bf16": ((0, 0),), "split3": ((0, 0), (0, 1), (1, 0)), "split4": ((0, 0), (0, 1), (1, 0), (1, 1))}


# ------------------------------------------------------------------------------------------------ parts
def bf16_rne(v):
    """Nearest bf16 value (8 significant bits, ties to even, fp32's exponent range with gradual underflow) of a float32 or
    float64 tensor, as float64.  Straight from the definition: |v| = m 2^e with m in [0.5, 1) is rounded to a multiple of
    2^(e - 8); below the normal range the quantum stays 2^-133."""
    v = v.double()
    _, e = torch.frexp(v)
    e = e.clamp_min(-125)
    q = torch.round(torch.ldexp(v, 8 - e))                   # torch.round: halves to even
    return torch.ldexp(q, e - 8)


def bf16_trunc(v):
    """bf16 by dropping the low bits (round toward zero): what the kernels do NOT do; a mutation of the CPU test."""
    v = v.double()
    _, e = torch.frexp(v)
    e = e.clamp_min(-125)
    return torch.ldexp(torch.trunc(torch.ldexp(v, 8 - e)), e - 8)


def parts(x, blk16=False):
    """(hi, lo) of an fp32 operand, float64.  blk16: the operand is stored as (or first rounded to) bf16: no lo part."""
    assert x.dtype == torch.float32
    hi = bf16_rne(x)
    if blk16:
        return hi, torch.zeros_like(hi)
    return hi, bf16_rne(x - hi.float())


# ------------------------------------------------------------------------------------------------ operators
def analysis(r, w):
    """A r: (N,1,H,W) x (M,1,P,P) -> (N,M,H,W); out[m,y,x] = sum_ij w[m,i,j] r[y - P/2 + i, x - P/2 + j]."""
    return F.conv2d(r, w, padding=w.shape[-1] // 2)


def synthesis(z, w):
    """B z: (N,M,H,W) x (M,1,P,P) -> (N,1,H,W); the adjoint of `analysis` with the same bank."""
    return F.conv_transpose2d(z, w, padding=w.shape[-1] // 2)


def filter_grad(X, T, P):
    """du (x) im2col(T): (N,M,H,W) x (N,1,H,W) -> (M,1,P,P); out[m,i,j] = sum_nyx X[n,m,y,x] T[n, y - P/2 + i, x - P/2 + j]."""
    out = F.conv2d(T.transpose(0, 1), X.transpose(0, 1), padding=P // 2)      # (1, M, P, P)
    return out.transpose(0, 1)


def _product(op, a, b, precision, kept=None):
    """(value, S, n) of op(a, b) with a, b given as parts: the kept products, the same sum over absolute values, and the
    count of non-zero terms."""
    val = S = n = None
    for (i, j) in (_KEPT[precision] if kept is None else kept):
        v = op(a[i], b[j])
        s = op(a[i].abs(), b[j].abs())
        c = op((a[i] != 0).double(), (b[j] != 0).double())
        val, S, n = (v, s, c) if val is None else (val + v, S + s, n + c)
    return val, S, torch.round(n)


def _with_term(val, S, n, term, sign=1.0):
    """One more fp32 term (a base, a subtrahend) added to a sum."""
    if term is None:
        return val, S, n
    t = term.double()
    return val + sign * t, S + t.abs(), n + (t != 0).double()


def shrink(u, tau):
    """ST(u, tau) = u - clamp(u, -tau, tau), tau >= 0 per (n, m)."""
    t = tau.double()[:, :, None, None]
    return u - torch.minimum(torch.maximum(u, -t), t)


# ------------------------------------------------------------------------------------------------ operations
def forward_stage(r, wA, tau, base, sgn, precision, kept=None):
    """First / forward stage z' = ST(base + sgn A r, tau) BEFORE any rounding for bf16 storage (the acceptance predicate
    rounds): (z', b).  base None: the first stage.  A base read from a bf16-stored buffer is an exact fp32 term."""
    val, S, n = _product(analysis, parts(r), parts(wA), precision, kept)
    u, S, n = _with_term(sgn * val, S, n, base)
    return shrink(u, tau), n * EPS * S


def reverse_stage(thin, w1, on, base, precision, kept=None):
    """Reverse stage du = [on] (base + corr(thin; w1)) before any rounding for bf16 storage: (du, b).  `on` (bool, as the
    codes): the support bit of the map; base None: the sweep's first reverse stage."""
    val, S, n = _product(analysis, parts(thin), parts(w1), precision, kept)
    val, S, n = _with_term(val, S, n, base)
    return val * on, n * EPS * S * on


def dtau_sums(du, on, neg, c):
    """The threshold-gradient sums of a reverse stage from ITS du (N,M,H,W fp32): dt (2, M) with dt[0][m] = sum -sign(z') du,
    dt[1][m] = sum_n c[n] (the same over image n); (dt, b).  `neg`: the sign bit of the map."""
    d = du.double()
    t = torch.where(neg, d, -d) * on
    cn = torch.ones(du.shape[0], dtype=torch.float64) if c is None else c.double()
    per = t.sum(dim=(2, 3))                                                  # (N, M)
    pa = d.abs().mul(on).sum(dim=(2, 3))
    cnt = ((d != 0) & on).double().sum(dim=(2, 3))
    dt = torch.stack([per.sum(0), (cn[:, None] * per).sum(0)])
    S = torch.stack([pa.sum(0), (cn.abs()[:, None] * pa).sum(0)])
    n = torch.stack([cnt.sum(0), (cnt * (cn != 0)[:, None]).sum(0) + 1])     # the product with c[n] rounds once more
    return dt, n * EPS * S


def synth_assemble(z, wB, precision, blk16=False, mask=None, sub=None, alpha=1.0, kept=None):
    """The synthesis half with fused_assemble's arguments: mask * alpha * (B z) - sub; (value, b).  blk16: z is a bf16-stored
    code (no lo part).  alpha is +-1 in every caller (exact); another alpha costs one rounding, which n_e covers."""
    val, S, n = _product(synthesis, parts(z, blk16), parts(wB), precision, kept)
    m = 1.0 if mask is None else mask.double()
    val, S, n = m * alpha * val, m * abs(alpha) * S, m * n
    val, S, n = _with_term(val, S, n, sub, -1.0)
    return val, n * EPS * S


def wgrad(X, T, alpha, P, precision, blk16=False, kept=None):
    """The filter gradient alpha * X (x) im2col(T): (value (M,1,P,P), b).  blk16: X is a bf16-stored code."""
    val, S, n = _product(lambda a, b: filter_grad(a, b, P), parts(X, blk16), parts(T), precision, kept)
    return alpha * val, (n + 1) * EPS * abs(alpha) * S


# ------------------------------------------------------------------------------------------------ acceptance
def violations_fp32(got, model, b):
    """(number of elements that do NOT satisfy |got - model| <= b, worst |err| / b over the elements with b > 0) of an fp32
    output.  Where b == 0 the model is an exact zero and so must the output be.  The count is of the negated predicate, so
    a NaN (in the output, or in a model fed a NaN output of the device) is a violation, never a pass; it makes `worst`
    infinite."""
    err = (got.double() - model).abs()
    bad = int((~(err <= b)).sum())
    pos = b > 0
    ratio = err[pos] / b[pos]
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if bool(pos.any()) else 0.0
    return bad, worst


def violations_bf16(got, model, b):
    """(number of elements NOT inside [bf16_rne(model - b), bf16_rne(model + b)], worst |got - bf16_rne(model)| in units of
    b + one bf16 step of the model) of a bf16-stored output (given as bf16 or as the fp32 values it decodes to).  A NaN is
    a violation, as in violations_fp32."""
    g = got.double()
    lo, hi = bf16_rne(model - b), bf16_rne(model + b)
    bad = int((~((g >= lo) & (g <= hi))).sum())
    step = (bf16_rne(model.abs() * (1 + 2.0 ** -7)) - bf16_rne(model.abs())).abs() + 2.0 ** -133
    ratio = (g - bf16_rne(model)).abs() / (b + step)
    worst = float(torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio).max())
    return bad, worst


def zeros_off_support(got, on):
    """Number of elements with the map bit off that are not exact zeros (a NaN is not a zero)."""
    return int((~(got.double() == 0) & ~on).sum())


# ------------------------------------------------------------------------------------------------ an honest fp32 version
def honest_product(op, a32, b32, precision, kept=None, blk16_a=False):
    """op(a, b) the way an fp32 implementation of the definition computes it: the kept products one by one through torch's
    float32 operator, summed in float32.  Used by the CPU test to show that the bound admits a correct implementation."""
    a = [p.float() for p in parts(a32, blk16_a)]
    b = [p.float() for p in parts(b32)]
    out = None
    for (i, j) in (_KEPT[precision] if kept is None else kept):
        v = op(a[i], b[j])
        out = v if out is None else out + v
    return out


# ------------------------------------------------------------------------------------------------ test content
def stage_inputs(N, M, P, H, W, seed):
    """The data recipe of the cell tests: a dict of float32 CPU tensors (r, thin, r2, wA, wB, zin sparse, base, gate sparse,
    tau, c, mask, sub)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen)
    d = dict(r=rnd(N, 1, H, W), thin=rnd(N, 1, H, W), r2=rnd(N, 1, H, W), sub=rnd(N, 1, H, W),
             wA=0.1 * rnd(M, 1, P, P), wB=0.1 * rnd(M, 1, P, P))
    d["zin"] = rnd(N, M, H, W) * (torch.rand(N, M, H, W, generator=gen) < 0.4)
    d["base"] = rnd(N, M, H, W)
    d["gate"] = rnd(N, M, H, W) * (torch.rand(N, M, H, W, generator=gen) < 0.3)
    d["tau"] = 0.3 * torch.rand(N, M, generator=gen)
    d["c"] = torch.rand(N, generator=gen)
    d["mask"] = (torch.rand(N, 1, H, W, generator=gen) < 0.5).float()
    return d


def crafted_split4_inputs(N, M, P, H, W, seed):
    """Inputs on which the lo . lo products are visible: (r, w) with every element x = hi + lo, |lo| = 2^-9 |hi| (hi a bf16
    value with a random 8-bit significand, lo of hi's sign: x is an fp32 value and splits back into exactly these parts),
    and single-tap filters, so that an output element is ONE tap's four products: n_e <= 4, b <= 4 * 2^-23 |x w| (1 + 2^-9)^2
    against lo . lo = 2^-18 |x w|, a factor of 7.9."""
    gen = torch.Generator().manual_seed(seed)

    def operand(*shape):
        sig = torch.randint(129, 256, shape, generator=gen).double()          # 8 bits, never a power of two
        ex = torch.randint(-3, 2, shape, generator=gen)
        sg = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        hi = sg * torch.ldexp(sig, ex - 8)
        x = (hi * (1 + 2.0 ** -9)).float()
        assert torch.equal(x.double(), hi * (1 + 2.0 ** -9))
        return x

    r = operand(N, 1, H, W)
    w = torch.zeros(M, 1, P, P)
    tap = torch.randint(0, P * P, (M,), generator=gen)
    w.view(M, P * P)[torch.arange(M), tap] = 0.25 * operand(M)
    return r, w


# ------------------------------------------------------------------------------------------------ exactly-summable stages
# DESIGN.md section 41.  The bound above grows with the number of terms and rounding errors with its square root, so in the
# long sums (synthesis, threshold sums, filter gradients) a wrong kernel passes it.  The second instrument is
# generic_arith_restate's: operands whose kept products are multiples of one quantum and few enough that every partial sum in
# every order is an fp32 number (S_e / quantum < CAP_QUANTA), so a correct kernel EQUALS the model.  A stage is two chained
# halves and the second half's operand is the first half's output, so three recipes are needed:
#   "int"    every operand an integer in {0, +-1, +-2}, tau integer per (n, m), c powers of two: every intermediate is an
#            integer below 2^8 with no lo part and the whole launch, its assemble and its reductions are exact (quantum 1);
#   "hilo-a" r / thin, wA, base hi + lo operands (hi in {0, +-1}, lo in {0, +-2^-9}), tau multiples of 2^-9: the ANALYSIS half
#            is exact (quantum 2^-9); z' then carries up to 15 bits and the synthesis half is held to b;
#   "hilo-p" the analysis half passes a hi + lo operand through the registers (an all-zero wA bank with tau in {0, 2}, or
#            single-tap +-1 filters with tau = 0 in a first stage), so the SYNTHESIS half, the threshold sums and the dA_k
#            ride get hi + lo operands and are exact.
# The quantum follows from the arithmetic: bf16 keeps hi.hi (integers here); split3 adds hi.lo + lo.hi (2^-9); split4 adds lo.lo
# (2^-18), under which the cap would ask for S_e < 8 -- so under split4 the filter banks (and the thin operand of a filter
# gradient) carry no lo part, and lo.lo stays with the crafted-input tests.  The generic module is imported where it is used:
# it imports this one.
RECIPES = ("int", "hilo-a", "hilo-p")
EXACT_HELD = {"int": ("code", "thin", "dt", "dA"), "hilo-a": ("code",), "hilo-p": ("code", "thin", "dt", "dA")}


def _G():
    import generic_arith_restate as G
    return G


def hi_only(x):
    """The operand with its lo part removed (a bf16 value as fp32)."""
    return bf16_rne(x).float()


def product_quantum(precision, a32, b32):
    """The quantum of the kept products of two exact operands, derived from their parts: 1 where only hi.hi is kept or neither
    has a lo part, 2^-9 where one side's lo meets the other's hi, 2^-18 where lo.lo is kept and both sides have a lo part."""
    la, lb = bool(parts(a32)[1].any()), bool(parts(b32)[1].any())
    kept = _KEPT[precision]
    q = 1.0
    if ((1, 0) in kept and la) or ((0, 1) in kept and lb):
        q = 2.0 ** -9
    if (1, 1) in kept and la and lb:
        q = 2.0 ** -18
    return q


def operand_quantum(x32):
    """The quantum of an fp32 term added as it is (a base, a threshold, a subtrahend): 2^-9 if it has a lo part, else 1."""
    return 2.0 ** -9 if bool(parts(x32)[1].any()) else 1.0


def exact_stage_operands(recipe, precision, ish, csh, fsh, seed, first=False, density=(0.5, 0.25, 0.5)):
    """The operands of one stage under a recipe, for any geometry of the fused tiers: images of shape ish (r, thin, r2, sub,
    mask), codes of shape csh (zin, base, gate), banks of shape fsh (wA, wB), tau (N, M), c (N).  density: images, banks,
    gate.  first: the pass-through bank of a FIRST stage (single taps) instead of the all-zero one.  Every tensor has a
    generator of its own."""
    G = _G()
    N, M = csh[:2]
    integer = recipe == "int"
    gens = iter(torch.Generator().manual_seed(1000 * seed + i) for i in range(32))
    op = lambda shape, dens, integ=integer: G._exact_operand(tuple(shape), dens, integ, next(gens))
    e = dict(recipe=recipe, r=op(ish, density[0]), thin=op(ish, density[0]), r2=op(ish, density[0]), sub=op(ish, density[0]),
             wA=op(fsh, density[1]), wB=op(fsh, density[1]), zin=op(csh, 0.4), base=op(csh, 1.0), gate=op(csh, density[2], True))
    e["mask"] = (torch.rand(ish, generator=next(gens)) < 0.5).float()
    e["c"] = torch.exp2(torch.arange(N) % 3 - 1.0)                           # 1/2, 1, 2, ...
    g = next(gens)
    if integer:
        e["tau"] = torch.randint(0, 4, (N, M), generator=g).float()
        e["tau"][:, M // 3] = 1024.0                                         # silences a whole channel
    elif recipe == "hilo-a":
        e["tau"] = torch.randint(0, 600, (N, M), generator=g).float() * 2.0 ** -9 * (torch.rand(N, M, generator=g) < 0.8)
    else:
        e["tau"] = 2.0 * (torch.rand(N, M, generator=g) < 0.3).float()
        e["tau"][:, M // 3] = 2.0
        e["tau"][:, 0] = 0.0
        # the reverse forms: ONE non-zero channel per code pixel (generic_arith_restate.exact_inputs' F), so that the threshold
        # sums and the filter gradients stay under the cap
        ch = torch.randint(0, M, (N, 1) + tuple(csh[2:]), generator=g)
        e["base"] = torch.zeros(csh).scatter_(1, ch, op((N, 1) + tuple(csh[2:]), 1.0))
        e["wA"] = torch.zeros(fsh)
        if first:
            taps = e["wA"][0].numel()
            e["wA"].view(M, taps)[torch.arange(M), torch.randint(0, taps, (M,), generator=g)] = \
                torch.randint(0, 2, (M,), generator=g).float() * 2 - 1
            e["tau"] = torch.zeros(N, M)
    if precision == "split4" and not integer:
        e["wA"], e["wB"], e["r2"] = hi_only(e["wA"]), hi_only(e["wB"]), hi_only(e["r2"])
    return e


def exact_stage_inputs(recipe, precision, N, M, P, H, W, seed, first=False):
    """exact_stage_operands at the 2-D tier's geometry (one image channel, P x P filters)."""
    return exact_stage_operands(recipe, precision, (N, 1, H, W), (N, M, H, W), (M, 1, P, P), seed, first)


def _value_and_abs(op, a, b, precision):
    """(value, S_e) of the kept products: `_product` without the term count."""
    val = S = None
    for (i, j) in _KEPT[precision]:
        v, s = op(a[i], b[j]), op(a[i].abs(), b[j].abs())
        val, S = (v, s) if val is None else (val + v, S + s)
    return val, S


def _rows(x):
    """A code tensor with its depth (if any) folded into its rows, (N,M,D*H,W): what the elementwise helpers above take."""
    return x.reshape(x.shape[0], x.shape[1], -1, x.shape[-1])


def exact_stage_model(mode, e, precision, blk16_in=False, blk16_out=False, masked=True, ride=False, ops=None, wgrad_P=None):
    """{output: (value, S_e, quantum)} of one stage on exact operands, each half fed the MODEL's own output of the half before
    it: "code" (z' / du as stored: bf16_rne of it for a bf16-stored output), "thin" (the assembled r_next = mask B z' - sub of
    a forward stage, q = -mask B du of a reverse one), "dt" and "dA" (reverse stages).  The synthesis half and the dA_k ride
    take the code as stored; the threshold sums take du_k BEFORE its rounding for a bf16-stored buffer (k_stage adds the
    register value in its epilogue, in front of bf16_round: the sums are the more accurate for it, and an fp32 input layout
    shows the difference).  mode: first | fwd | bwd | bwd0 (a reverse stage without base).  ops: (analysis, synthesis) of the
    geometry, this module's by default.  Which outputs a recipe holds to equality is EXACT_HELD; the cap is asserted on
    S_e / quantum by the CPU tests."""
    ana, syn = (analysis, synthesis) if ops is None else ops
    stored = lambda x: bf16_rne(x).float() if blk16_in else x
    if mode in ("first", "fwd"):
        val, S = _value_and_abs(ana, parts(e["r"]), parts(e["wA"]), precision)
        q = product_quantum(precision, e["r"], e["wA"])
        if mode == "fwd":
            val, S = stored(e["zin"]).double() - val, S + stored(e["zin"]).double().abs()
            q = min(q, operand_quantum(stored(e["zin"])))
        code, S = shrink(_rows(val), e["tau"]).reshape(val.shape), S + e["tau"].double().reshape(e["tau"].shape + (1,) * (val.dim() - 2))
        q = min(q, operand_quantum(e["tau"]))
    else:
        val, S = _value_and_abs(ana, parts(e["thin"]), parts(e["wA"]), precision)
        q = product_quantum(precision, e["thin"], e["wA"])
        if mode == "bwd":
            val, S = val + stored(e["base"]).double(), S + stored(e["base"]).double().abs()
            q = min(q, operand_quantum(stored(e["base"])))
        on = e["gate"] != 0
        code, S = val * on, S * on
    full = code                                              # a bf16-stored du_k enters the threshold sums BEFORE its rounding
    if blk16_out:
        code = bf16_rne(code)
    out = {"code": (code, S, q)}
    z = code.float()
    assert torch.equal(z.double(), code), "the code of an exact recipe is an fp32 number"
    val, S = _value_and_abs(syn, parts(z, blk16_out), parts(e["wB"]), precision)
    q = product_quantum(precision, z, e["wB"])
    m = e["mask"].double() if masked else 1.0
    if mode in ("first", "fwd"):
        out["thin"] = (m * val - e["sub"].double(), m * S + e["sub"].double().abs(), min(q, operand_quantum(e["sub"])))
    else:
        out["thin"] = (-(m * val), m * S, q)
        assert torch.equal(full.float().double(), full)
        zf, onf, negf = _rows(full.float()), _rows(on), _rows(e["gate"] < 0)
        dt, _ = dtau_sums(zf, onf, negf, e["c"])
        pa = zf.double().abs().mul(onf).sum(dim=(2, 3))
        out["dt"] = (dt, torch.stack([pa.sum(0), (e["c"].double().abs()[:, None] * pa).sum(0)]),
                     operand_quantum(full.float()) * min(1.0, float(e["c"].min())))
        if ride:
            val, S = _value_and_abs(lambda a, b: filter_grad(a, b, wgrad_P), parts(z, blk16_out), parts(e["r2"]), precision)
            out["dA"] = (-val, S, product_quantum(precision, z, e["r2"]))
    return out


def exact_wgrad_model(X, T, alpha, P, precision, blk16=False):
    """(value, S_e, quantum) of k_wgrad2d's alpha * X (x) im2col(T) on exact operands; alpha = +-1."""
    Xs = hi_only(X) if blk16 else X
    val, S = _value_and_abs(lambda a, b: filter_grad(a, b, P), parts(Xs, blk16), parts(T), precision)
    return alpha * val, S, product_quantum(precision, Xs, T)


def cap_quanta(S, quantum):
    """The largest S_e of an output in quanta: what the cap (generic_arith_restate.CAP_QUANTA) is asserted on."""
    return float(S.max()) / quantum if S.numel() else 0.0


def violations_exact(got, model, quantum=1.0):
    """(number of elements that are NOT equal in value to the model, largest |got - model| in quanta): the predicate of the
    exact inputs.  The count is of the negated predicate, so a NaN is a violation (and makes `worst` infinite); -0 equals +0.
    A bf16-stored output is compared as the values it decodes to, against a model that is bf16_rne of the exact value."""
    g, m = got.double(), model.double()
    bad = int((~(g == m)).sum())
    err = (g - m).abs() / quantum
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
    return bad, (float(err.max()) if err.numel() else 0.0)
