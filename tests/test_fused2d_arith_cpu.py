"""The float64 model of the fused 2-D arithmetics (fused2d_arith_restate.py) and its bound, on the CPU: an honest fp32
implementation of the definition (the kept products one by one through torch's float32 conv2d, summed in float32) stays
inside the bound in every mode and operation at the shapes of test_gpu_fused_cells.py; implementations that are subtly
wrong leave it.  Thresholds of the mutation counts are reasoned in the tests, not measured.  Second part (DESIGN.md section
41): the exactly-summable stage inputs -- the recipes, the cap for every input of the GPU cells, an honest fp32 evaluation
equal to the model in two summation orders, and the table of mutants the bound lets through and equality does not."""
import functools

import pytest
import torch

import fused2d_arith_restate as R

N, H, W = 2, 40, 150
MP = [(64, 7), (32, 5), (64, 3)]


@functools.lru_cache(maxsize=None)
def _data(M, P):
    return R.stage_inputs(N, M, P, H, W, seed=5 + M + P)


def _shrink32(u, tau):
    t = tau[:, :, None, None]
    return u - torch.minimum(torch.maximum(u, -t), t)


def _honest_forward(d, precision, first, kept=None, wA=None):
    acc = R.honest_product(R.analysis, d["r"], d["wA"] if wA is None else wA, precision, kept)
    u = acc if first else d["zin"] - acc
    return _shrink32(u, d["tau"])


def _honest_reverse(d, precision, on, kept=None, w1=None):
    acc = R.honest_product(R.analysis, d["thin"], d["wA"] if w1 is None else w1, precision, kept)
    return (d["base"] + acc) * on


def test_parts_are_torchs_bfloat16_bit_for_bit():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(1 << 16, generator=gen) * torch.exp2(torch.randint(-30, 30, (1 << 16,), generator=gen).float())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 1.0 - 2.0 ** -9, 2.0 ** -130, 0.0, -0.0,
                         3.3895313892515355e38, 2.0 ** -126 * (1 + 2.0 ** -8)])
    x = torch.cat([x, ties])
    hi, lo = R.parts(x)
    want_hi = x.bfloat16().float()
    assert torch.equal(hi.float().view(torch.int32), want_hi.view(torch.int32))
    assert torch.equal(hi, want_hi.double())
    want_lo = (x - want_hi).bfloat16().float()
    assert torch.equal(lo, want_lo.double())
    # float64 arguments are rounded once, not through fp32: 1 + 2^-8 + 2^-40 lies above the tie and rounds up
    assert float(R.bf16_rne(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64))) == 1.0 + 2.0 ** -7
    assert float(R.bf16_trunc(torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -20]))) == 1.0
    # a bf16-stored operand has no lo part
    assert not R.parts(x, blk16=True)[1].any()


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("M,P", MP)
def test_honest_fp32_implementation_is_inside_the_bound(M, P, precision):
    d = _data(M, P)
    worst = {}
    for first in (False, True):
        z, b = R.forward_stage(d["r"], d["wA"], d["tau"], None if first else d["zin"], 1.0 if first else -1.0, precision)
        got = _honest_forward(d, precision, first)
        bad, worst["first" if first else "fwd"] = R.violations_fp32(got, z, b)
        assert bad == 0
        bad, _ = R.violations_bf16(got.bfloat16(), z, b)                       # the same output stored as bf16
        assert bad == 0
    on = d["gate"] != 0
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], precision)
    got = _honest_reverse(d, precision, on)
    bad, worst["bwd"] = R.violations_fp32(got, du, b)
    assert bad == 0 and R.zeros_off_support(got, on) == 0
    dt, bt = R.dtau_sums(got, on, d["gate"] < 0, d["c"])
    t32 = torch.where(d["gate"] < 0, got, -got)
    dt32 = torch.stack([t32.sum(dim=(0, 2, 3)), (d["c"][:, None] * t32.sum(dim=(2, 3))).sum(0)])
    bad, worst["dtau"] = R.violations_fp32(dt32, dt, bt)
    assert bad == 0
    for blk16 in (False, True):
        z = d["zin"].bfloat16().float() if blk16 else d["zin"]
        val, b = R.synth_assemble(z, d["wB"], precision, blk16, d["mask"], d["sub"], -1.0)
        got = d["mask"] * -R.honest_product(R.synthesis, z, d["wB"], precision, blk16_a=blk16) - d["sub"]
        bad, worst["synth16" if blk16 else "synth"] = R.violations_fp32(got, val, b)
        assert bad == 0
    val, b = R.wgrad(d["gate"], d["r2"], -1.0, P, precision)
    got = -R.honest_product(lambda a, c: R.filter_grad(a, c, P), d["gate"], d["r2"], precision)
    bad, worst["wgrad"] = R.violations_fp32(got, val, b)
    assert bad == 0
    print(f"M{M}P{P} {precision}: worst |err|/b " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    # round-to-nearest adds err by at most 2^-24 each, half of what the bound allows per term: the honest version can
    # never pass 0.5, and being a sum of random roundings it sits far below (the cap is not a fit to it)
    assert max(worst.values()) < 0.5


@pytest.mark.parametrize("precision", R.PRECISIONS)
def test_a_zeroed_tap_violates_the_bound(precision):
    """One tap of one channel zeroed changes every in-image element of that channel's analysis by w r[.]: far above b
    (about n 2^-23 S ~ 1e-5) unless r is tiny there.  Reverse stage with the whole map on: at least half the channel's
    N H W = 12000 elements must violate; forward stage: only elements that pass the threshold move, still many."""
    M, P = 64, 7
    d = _data(M, P)
    w = d["wA"].clone()
    w[17, 0, 2, 5] = 0.0
    on = torch.ones_like(d["gate"], dtype=torch.bool)
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], precision)
    err = (_honest_reverse(d, precision, on, w1=w).double() - du).abs() > b
    assert int(err.sum()) >= N * H * W // 2 and int(err[:, 17].sum()) == int(err.sum())
    z, b = R.forward_stage(d["r"], d["wA"], d["tau"], d["zin"], -1.0, precision)
    bad, _ = R.violations_fp32(_honest_forward(d, precision, False, wA=w), z, b)
    assert bad >= N * H * W // 8


def test_split3_without_lo_hi_violates_the_bound():
    """The dropped term is of relative size 2^-9 per product against a bound of about 49 * 3 * 2^-23: almost every element
    of the reverse stage (no threshold) must violate."""
    M, P = 64, 7
    d = _data(M, P)
    on = torch.ones_like(d["gate"], dtype=torch.bool)
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], "split3")
    bad, _ = R.violations_fp32(_honest_reverse(d, "split3", on, kept=((0, 0), (0, 1))), du, b)
    assert bad > 0.9 * du.numel()


def test_a_truncated_bf16_output_violates_the_bound():
    """Truncation differs from round-to-nearest in about half of the non-zero elements, by one bf16 step (2^-8 relative)
    against b of 2^-17 relative: at least a quarter of the non-zero elements must fall outside."""
    M, P = 32, 5
    d = _data(M, P)
    z, b = R.forward_stage(d["r"], d["wA"], d["tau"], d["zin"], -1.0, "split3")
    got = _honest_forward(d, "split3", False)
    assert R.violations_bf16(got.bfloat16(), z, b)[0] == 0
    bad, _ = R.violations_bf16(R.bf16_trunc(got), z, b)
    assert bad > 0.25 * int((got != 0).sum())


def test_an_ignored_map_bit_violates_the_zero_predicate():
    M, P = 32, 5
    d = _data(M, P)
    on = d["gate"] != 0
    ignored = on.clone()
    idx = tuple((~on).nonzero()[-7].tolist())                 # an off element near the end of the last image
    assert not on[idx]
    ignored[idx] = True
    got = _honest_reverse(d, "split3", ignored)
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], "split3")
    assert R.zeros_off_support(got, on) == 1
    assert R.violations_fp32(got, du, b)[0] == 1
    assert R.zeros_off_support(_honest_reverse(d, "split3", on), on) == 0


def test_a_nan_or_infinite_element_violates_every_predicate():
    """Comparisons with NaN are false: the predicates count what does NOT satisfy them, so one NaN (an unwritten slot of a
    NaN-filled buffer, a NaN on the support) or one infinity in an otherwise correct output is one violation -- on the
    support and off it, in the fp32 and the bf16 form, and when it reaches a model as the device's own code."""
    M, P = 32, 5
    d = _data(M, P)
    on = d["gate"] != 0
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], "split3")
    good = _honest_reverse(d, "split3", on)
    i_on, i_off = tuple(on.nonzero()[5].tolist()), tuple((~on).nonzero()[5].tolist())
    for idx in (i_on, i_off):
        for poison in (float("nan"), float("inf"), -float("inf")):
            got = good.clone()
            got[idx] = poison
            bad, worst = R.violations_fp32(got, du, b)
            assert bad == 1 and (worst == float("inf") or idx == i_off), (idx, poison, bad, worst)
            assert R.violations_bf16(got.bfloat16(), du, b)[0] == 1
            assert R.zeros_off_support(got, on) == (1 if idx == i_off else 0)
    # a NaN code fed to the models of the other half: every element it reaches is a violation, whatever the device wrote there
    got = good.clone()
    got[i_on] = float("nan")
    thin, bt = R.synth_assemble(got, d["wB"], "split3")
    clean = R.synth_assemble(good, d["wB"], "split3")[0]
    assert R.violations_fp32(clean.float(), thin, bt)[0] == int(thin.isnan().sum()) > 0
    dt, bdt = R.dtau_sums(got, on, d["gate"] < 0, d["c"])
    assert R.violations_fp32(torch.zeros(2, M), dt, bdt)[0] >= 2
    # a NaN where the model is an exact zero with b == 0 (first stage below the threshold) is counted too
    z, bz = R.forward_stage(d["r"], 0 * d["wA"], d["tau"], None, 1.0, "split3")
    assert not z.any() and not bz.any()
    got = torch.zeros_like(z, dtype=torch.float32)
    got[0, 3, 7, 11] = float("nan")
    assert R.violations_fp32(got, z, bz)[0] == 1 and R.violations_bf16(got, z, bz)[0] == 1


@pytest.mark.parametrize("M,P", [(64, 7), (32, 5)])
def test_crafted_inputs_tell_split4_from_split3(M, P):
    """Random data cannot: there lo . lo lies below the bound.  On the crafted inputs an honest split4 passes the split4
    model and fails the split3 model at (nearly) every non-zero element, and an honest split3 fails the split4 model."""
    r, w = R.crafted_split4_inputs(N, M, P, H, W, seed=40 + M)
    hi, lo = R.parts(r)
    assert torch.equal(lo, hi * 2.0 ** -9)
    on = torch.ones(N, M, H, W, dtype=torch.bool)
    m4, b4 = R.reverse_stage(r, w, on, None, "split4")
    m3, b3 = R.reverse_stage(r, w, on, None, "split3")
    nz = int((m4 != 0).sum())
    assert nz > 0.9 * N * M * (H - P) * (W - P)
    h4 = R.honest_product(R.analysis, r, w, "split4")
    h3 = R.honest_product(R.analysis, r, w, "split3")
    assert R.violations_fp32(h4, m4, b4)[0] == 0 and R.violations_fp32(h3, m3, b3)[0] == 0
    assert R.violations_fp32(h4, m3, b3)[0] == nz
    assert R.violations_fp32(h3, m4, b4)[0] == nz
    # random data: the split3 implementation is inside the split4 bound (why the crafted case is needed)
    d = _data(M, P)
    on = d["gate"] != 0
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], "split4")
    assert R.violations_fp32(_honest_reverse(d, "split3", on), du, b)[0] == 0


# ------------------------------------------------------------------------------------------------ exactly-summable stages
# DESIGN.md section 41.  An honest fp32 evaluation of a stage on the exact operands of a recipe, each half fed the half before
# it, as the device does.
import generic_arith_restate as G  # noqa: E402


def _h_code(mode, e, prec, acc=None):
    if mode in ("first", "fwd"):
        acc = R.honest_product(R.analysis, e["r"], e["wA"], prec) if acc is None else acc
        return _shrink32(acc if mode == "first" else e["zin"] - acc, e["tau"])
    acc = R.honest_product(R.analysis, e["thin"], e["wA"], prec) if acc is None else acc
    return (e["base"] + acc) * (e["gate"] != 0)


def _h_thin(fwd, e, prec, z, kept=None, flip=False):
    z, w = (torch.flip(z, (1,)), torch.flip(e["wB"], (0,))) if flip else (z, e["wB"])
    acc = R.honest_product(R.synthesis, z, w, prec, kept)
    return e["mask"] * acc - e["sub"] if fwd else -(e["mask"] * acc)


def _h_dt(e, du, perm=None):
    t = (torch.where(e["gate"] < 0, du, -du) * (e["gate"] != 0)).reshape(N, du.shape[1], -1)
    per = (t if perm is None else t[:, :, perm]).sum(-1)
    return torch.stack([per.sum(0), (e["c"][:, None] * per).sum(0)])


def _h_dA(e, du, prec, P, kept=None):
    return -R.honest_product(lambda a, c: R.filter_grad(a, c, P), du, e["r2"], prec, kept)


def _by_hand(a_img, w, prec, perm_seed):
    """A a_img with the taps in a random order, as one matrix product per kept product over an im2col written out."""
    M, P = w.shape[0], w.shape[-1]
    col = G.im2col(a_img, (P, P), 1)                                         # (N, 1, T, Z)
    perm = torch.randperm(P * P, generator=torch.Generator().manual_seed(perm_seed))
    colk, wk = col[:, 0, perm].contiguous(), w.reshape(M, -1)[:, perm].contiguous()
    acc = None
    for (i, j) in R._KEPT[prec]:
        t = R.parts(wk)[j].float() @ R.parts(colk)[i].float()
        acc = t if acc is None else acc + t
    return acc.reshape(N, M, H, W)


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("M,P", [(64, 7), (32, 5)])
def test_exact_stage_inputs_are_what_the_recipe_says_and_fp32_reproduces_the_model_in_two_orders(M, P, recipe, precision):
    held = R.EXACT_HELD[recipe]
    for mode in ("first", "fwd", "bwd"):
        e = R.exact_stage_inputs(recipe, precision, N, M, P, H, W, seed=31 + M + P, first=mode == "first")
        # -- the operands are what the recipe says
        ints = {0.0, 1.0, -1.0, 2.0, -2.0}
        for k in ("r", "thin", "r2", "wA", "wB", "zin", "base", "sub"):
            hi, lo = R.parts(e[k])
            assert set(hi.unique().tolist()) <= (ints if recipe == "int" else {0.0, 1.0, -1.0}), k
            assert set(lo.unique().tolist()) <= ({0.0} if recipe == "int" else {0.0, 2.0 ** -9, -2.0 ** -9}), k
        assert bool((e["tau"] == 0).any()) and bool((e["tau"] * 2 ** 9 == torch.round(e["tau"] * 2 ** 9)).all())
        assert bool((torch.log2(e["c"]) == torch.round(torch.log2(e["c"]))).all())
        if recipe != "int" and precision == "split4":                         # lo parts on one operand only
            assert not any(R.parts(e[k])[1].any() for k in ("wA", "wB", "r2")) and bool(R.parts(e["r"])[1].any())
        if recipe == "hilo-p":
            assert (int((e["wA"] != 0).sum()) == M) if mode == "first" else not e["wA"].any()
            assert set(e["tau"].unique().tolist()) <= {0.0, 2.0} and bool(((e["base"] != 0).sum(1) == 1).all())
        model = R.exact_stage_model(mode, e, precision, ride=mode == "bwd", wgrad_P=P)
        for k in held:
            if k in model:
                val, S, q = model[k]
                assert G.exact_cap_ok(S, q), (mode, k, R.cap_quanta(S, q))
                assert bool((val / q == torch.round(val / q)).all()), (mode, k)
        code = model["code"][0].float()
        if recipe == "int":
            assert not R.parts(code)[1].any() and float(code.abs().max()) < 2 ** 8
            assert mode == "bwd" or not code[:, M // 3].any()                 # the silenced channel
        elif recipe == "hilo-a":
            assert float(code.abs().max()) < 2 ** 6
        elif precision != "bf16":
            assert bool(R.parts(code)[1].any())                              # hi + lo operands reach the second half
        # -- order 1: torch's own float32 operators; order 2: the summed axes permuted / reversed, by hand
        fwd = mode != "bwd"
        for order in (1, 2):
            acc = None if order == 1 else _by_hand(e["r"] if fwd else e["thin"], e["wA"], precision, 2)
            got = _h_code(mode, e, precision, acc)
            assert R.violations_exact(got, model["code"][0])[0] == 0, (mode, order, "code")
            if "thin" in held:
                assert R.violations_exact(_h_thin(fwd, e, precision, got, flip=order == 2), model["thin"][0])[0] == 0, (mode, order)
            if not fwd and "dt" in held:
                perm = None if order == 1 else torch.randperm(H * W, generator=torch.Generator().manual_seed(1))
                assert R.violations_exact(_h_dt(e, got, perm), model["dt"][0])[0] == 0, (mode, order, "dt")
                # order 2: images and pixels reversed (which reverses the taps: flipped back)
                dA = _h_dA(e, got, precision, P) if order == 1 else -torch.flip(R.honest_product(
                    lambda a, c: R.filter_grad(a, c, P), torch.flip(got, (0, 2, 3)), torch.flip(e["r2"], (0, 2, 3)), precision), (2, 3))
                assert R.violations_exact(dA, model["dA"][0])[0] == 0, (mode, order, "dA")


def test_bf16_stored_outputs_of_the_exact_recipes_are_bf16_rne_of_the_model():
    M, P = 32, 5
    for recipe in R.RECIPES:
        e = R.exact_stage_inputs(recipe, "split3", N, M, P, H, W, seed=31 + M + P)
        plain = R.exact_stage_model("fwd", e, "split3")
        stored = R.exact_stage_model("fwd", e, "split3", blk16_in=True, blk16_out=True)
        u16 = R.shrink(R.bf16_rne(e["zin"]) - R._value_and_abs(R.analysis, R.parts(e["r"]), R.parts(e["wA"]), "split3")[0], e["tau"])
        assert torch.equal(stored["code"][0], R.bf16_rne(u16)) and not R.parts(stored["code"][0].float())[1].any()
        assert recipe == "int" or R.violations_exact(stored["code"][0], plain["code"][0])[0] > 0
        got = _h_code("fwd", dict(e, zin=e["zin"].bfloat16().float()), "split3").bfloat16()
        assert R.violations_exact(got, stored["code"][0])[0] == 0
        assert R.violations_exact(R.bf16_trunc(_h_code("fwd", dict(e, zin=e["zin"].bfloat16().float()), "split3")), stored["code"][0])[0] > (0 if recipe == "hilo-a" else -1)


def test_the_threshold_sums_of_a_bf16_stored_du_take_it_before_its_rounding():
    """k_stage adds du_k to the threshold partials in its epilogue, in front of the rounding for a bf16-stored buffer.  On the
    pass-through recipe with an fp32 input layout the two readings differ at nearly every channel (on the seeded data the bound
    admits both); with a bf16-stored input du_k has no lo part and they coincide."""
    M, P = 32, 5
    e = R.exact_stage_inputs("hilo-p", "split3", N, M, P, H, W, seed=31 + M + P)
    on, neg = e["gate"] != 0, e["gate"] < 0
    m = R.exact_stage_model("bwd", e, "split3", blk16_in=False, blk16_out=True)
    du16, du = m["code"][0].float(), R.exact_stage_model("bwd", e, "split3")["code"][0].float()
    assert torch.equal(du16, du.bfloat16().float()) and not torch.equal(du16, du)
    assert R.violations_exact(_h_dt(e, du), m["dt"][0])[0] == 0
    assert R.violations_exact(_h_dt(e, du16), m["dt"][0])[0] > M
    assert R.violations_exact(_h_thin(False, e, "split3", du16), m["thin"][0])[0] == 0       # the synthesis takes the stored value
    both = R.exact_stage_model("bwd", e, "split3", blk16_in=True, blk16_out=True)
    assert R.violations_exact(_h_dt(e, both["code"][0].float()), both["dt"][0])[0] == 0
    d = _data(M, P)
    got = _honest_reverse(d, "split3", d["gate"] != 0)
    assert R.violations_fp32(_h_dt(d, got), *R.dtau_sums(got.bfloat16().float(), d["gate"] != 0, d["gate"] < 0, d["c"]))[0] == 0


def test_the_exact_predicate_counts_what_is_not_equal():
    m = torch.tensor([0.0, 1.5, -2.0, 3.0], dtype=torch.float64)
    assert R.violations_exact(torch.tensor([-0.0, 1.5, -2.0, 3.0]), m) == (0, 0.0)
    assert R.violations_exact(torch.tensor([0.0, 1.5 + 2.0 ** -9, -2.0, 3.0]), m, 2.0 ** -9) == (1, 1.0)
    bad, worst = R.violations_exact(torch.tensor([0.0, float("nan"), -2.0, float("inf")]), m)
    assert bad == 2 and worst == float("inf")
    assert R.product_quantum("bf16", torch.tensor([1 + 2.0 ** -9]), torch.tensor([1 - 2.0 ** -9])) == 1.0
    assert R.product_quantum("split3", torch.tensor([1 + 2.0 ** -9]), torch.tensor([1.0])) == 2.0 ** -9
    assert R.product_quantum("split3", torch.tensor([1 + 2.0 ** -9]), torch.tensor([1 - 2.0 ** -9])) == 2.0 ** -9
    assert R.product_quantum("split4", torch.tensor([1 + 2.0 ** -9]), torch.tensor([1 - 2.0 ** -9])) == 2.0 ** -18
    assert R.product_quantum("split4", torch.tensor([1 + 2.0 ** -9]), torch.tensor([2.0])) == 2.0 ** -9
    # split4 with lo on both sides of a stage's long sums: the cap would ask for S_e < 8
    assert G.CAP_QUANTA * 2.0 ** -18 == 8.0


@pytest.mark.parametrize("part", range(8))
def test_the_cap_holds_for_every_exact_input_of_the_gpu_cells(part):
    """test_gpu_fused_cells.exact_inputs_of_this_file: for every exact input a GPU test feeds a kernel and every output it
    holds to equality, the model's own S_e / quantum < CAP_QUANTA (in eight parts).  A condition on the recipes' densities,
    not a measurement: no case is skipped for failing it."""
    import test_gpu_fused_cells as T
    every = T.exact_inputs_of_this_file()
    stages = [c for c in every if c[0] == "stage"]
    assert len(stages) >= 3 * len(T.ROWS) * sum(len({(a == T.B16 and m != "first", b == T.B16) for a, b in T.PAIRS[m]}) for m in T.PAIRS)
    assert len(every) - len(stages) == 4 * len(T.ROWS)
    for case in every[part::8]:
        if case[0] == "stage":
            _, mode, M, P, prec, recipe, b_in, b_out = case
            model = T.exact_model(mode, M, P, prec, recipe, b_in, b_out)
            for k in R.EXACT_HELD[recipe]:
                if k in model:
                    assert R.cap_quanta(model[k][1], model[k][2]) < G.CAP_QUANTA, (case, k)
                    assert bool((model[k][0] / model[k][2] == torch.round(model[k][0] / model[k][2])).all()), (case, k)
            assert (mode == "ride") == ("dA" in model)
        else:
            _, M, P, prec, variant, blk16 = case
            d = T.exact_wgrad_data(M, P, prec, variant)
            assert all(bool(((d[k] != 0).sum(1) == 1).all()) for k in ("F", "F2"))
            for val, S, q in T.exact_wgrad_model(M, P, prec, variant, blk16):
                assert R.cap_quanta(S, q) < G.CAP_QUANTA and q == (1.0 if variant == "integer" or prec == "bf16" or blk16 and prec == "split4" else 2.0 ** -9), case
                assert bool((val / q == torch.round(val / q)).all())


# ---- the mutant table.  Each mutant is evaluated twice at a GPU cell's shape in split3: on the cell's seeded data against b, and
# on exact operands against equality.  x: the operands, with "z" the code the synthesis half is fed and "du" a reverse stage's
# output.  Returns (got, (model value, b)).
def _trunc_parts(x):
    hi = R.bf16_trunc(x)
    return hi.float(), R.bf16_trunc(x - hi.float()).float()


def _m_syn(x, P, minus):
    full = R.honest_product(R.synthesis, x["z"], x["wB"], "split3")
    return x["mask"] * (full - minus) - x["sub"], R.synth_assemble(x["z"], x["wB"], "split3", False, x["mask"], x["sub"], 1.0)


def _m_syn_lo_hi_one_tap(x, P):
    w = torch.zeros_like(x["wB"])
    w[:, :, P // 2 - 1, P // 2 + 1] = x["wB"][:, :, P // 2 - 1, P // 2 + 1]
    return _m_syn(x, P, R.synthesis(R.parts(x["z"])[1].float(), R.parts(w)[0].float()))


def _m_syn_lo_hi_one_channel(x, P):
    m = x["z"].shape[1] // 2 + 1
    return _m_syn(x, P, R.synthesis(R.parts(x["z"][:, m:m + 1])[1].float(), R.parts(x["wB"][m:m + 1])[0].float()))


def _m_syn_hi_lo_last_quad(x, P):
    return _m_syn(x, P, R.synthesis(R.parts(x["z"][:, -4:])[0].float(), R.parts(x["wB"][-4:])[1].float()))


def _m_dA_lo_hi(x, P):
    return _h_dA(x, x["du"], "split3", P, kept=((0, 0), (0, 1))), R.wgrad(x["du"], x["r2"], -1.0, P, "split3")


def _m_dt_one_pixel(x, P):
    du = x["du"].clone()
    y, xx = x["du"][1].abs().sum(0).nonzero()[1234 % int((x["du"][1].abs().sum(0) != 0).sum())].tolist()
    du[1, :, y, xx] = 0.0
    return _h_dt(x, du), R.dtau_sums(x["du"], x["gate"] != 0, x["gate"] < 0, x["c"])


def _m_zeroed_tap(x, P):
    w = x["wA"].clone()
    idx = tuple(w[3].nonzero()[len(w[3].nonzero()) // 2].tolist())           # a tap that is there (the exact banks are sparse)
    w[(3,) + idx] = 0.0
    on = x["gate"] != 0
    return (x["base"] + R.honest_product(R.analysis, x["thin"], w, "split3")) * on, R.reverse_stage(x["thin"], x["wA"], on, x["base"], "split3")


def _m_ignored_map_bit(x, P):
    on = x["gate"] != 0
    ignored = on.clone()
    ignored[tuple((~on).nonzero()[-7].tolist())] = True
    return (x["base"] + R.honest_product(R.analysis, x["thin"], x["wA"], "split3")) * ignored, R.reverse_stage(x["thin"], x["wA"], on, x["base"], "split3")


def _m_truncating_split(x, P):
    a, b = _trunc_parts(x["thin"]), _trunc_parts(x["wA"])
    acc = sum(R.analysis(a[i], b[j]) for (i, j) in R._KEPT["split3"])
    on = x["gate"] != 0
    return (x["base"] + acc) * on, R.reverse_stage(x["thin"], x["wA"], on, x["base"], "split3")


# mutant: (function, exact recipe it is shown on, {(M, P): does the bound b catch it on the seeded data})
MUTANTS = {
    "synthesis: lo.hi dropped at one tap of every filter": (_m_syn_lo_hi_one_tap, "hilo-p", {(64, 7): False, (32, 5): True}),
    "synthesis: lo.hi dropped for one channel": (_m_syn_lo_hi_one_channel, "hilo-p", {(64, 7): False, (32, 5): True}),
    "synthesis: hi.lo dropped for the last channel quad": (_m_syn_hi_lo_last_quad, "hilo-p", {(64, 7): False, (32, 5): True}),
    "dA / dB: lo.hi dropped at every term": (_m_dA_lo_hi, "hilo-p", {(64, 7): False, (32, 5): False}),
    "dt: one code pixel of one image missing from the sum": (_m_dt_one_pixel, "hilo-p", {(64, 7): True, (32, 5): True}),
    "analysis: a zeroed tap": (_m_zeroed_tap, "hilo-a", {(64, 7): True, (32, 5): True}),
    "an ignored map bit": (_m_ignored_map_bit, "hilo-a", {(64, 7): True, (32, 5): True}),
    "lo = bf16_trunc instead of round-to-nearest-even": (_m_truncating_split, "hilo-a", {(64, 7): True, (32, 5): True}),
}


@functools.lru_cache(maxsize=None)
def _mutant_operands(M, P, recipe):
    """The operands of a mutant: the cell's seeded data (recipe None) or the exact operands of a recipe, with the code the
    synthesis half is fed ("z") and a reverse stage's output ("du")."""
    if recipe is None:
        d = _data(M, P)
        return dict(d, z=d["zin"], du=_honest_reverse(d, "split3", d["gate"] != 0))
    e = R.exact_stage_inputs(recipe, "split3", N, M, P, H, W, seed=31 + M + P)
    return dict(e, z=R.exact_stage_model("fwd", e, "split3")["code"][0].float(), du=R.exact_stage_model("bwd", e, "split3")["code"][0].float())


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_leaves_the_exact_predicate_and_the_bound_only_where_the_table_says(mutant):
    """Every mutant leaves the exact predicate.  The ones the bound lets through on the seeded data (the long sums at the flagship
    shape) are why the exact inputs exist: that they pass b is asserted too, so that a later tightening of b shows up."""
    fn, recipe, table = MUTANTS[mutant]
    for (M, P), caught in table.items():
        got, model = fn(_mutant_operands(M, P, None), P)
        bad, worst = R.violations_fp32(got, *model)
        got_e, model_e = fn(_mutant_operands(M, P, recipe), P)
        off = R.violations_exact(got_e, model_e[0])[0]
        print(f"{mutant} [M{M}P{P}]: worst |err|/b {worst:.3g}, {bad} outside b; exact ({recipe}): {off} of {got_e.numel()} differ")
        assert off > 0, (mutant, M, P)
        assert (bad > 0) == caught, (mutant, M, P, bad, worst)
