"""The float64 model of the fused 2-D arithmetics (fused2d_arith_restate.py) and its bound, on the CPU: an honest fp32
implementation of the definition (the kept products one by one through torch's float32 conv2d, summed in float32) stays
inside the bound in every mode and operation at the shapes of test_gpu_fused_cells.py; implementations that are subtly
wrong leave it.  Thresholds of the mutation counts are reasoned in the tests, not measured."""
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
