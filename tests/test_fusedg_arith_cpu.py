"""The float64 model of the fused generic tier (fusedg_arith_restate.py) and its bound, on the CPU: at C = 1, stride 1, 2-D it
is the fused 2-D model bit for bit; an honest fp32 implementation of the definition (the kept products one by one through
torch's float32 conv*, summed in float32) stays inside the bound at a 3-D, a C = 3 masked and a stride-2 shape;
implementations that are subtly wrong in the ways this tier can be (a tap, a depth plane, the order of the groups, the
geometry of the stride-2 col2im, a dropped product, a map bit) leave it.  The mutation counts are reasoned in the tests."""
import functools

import pytest
import torch

import fused2d_arith_restate as R2
import fusedg_arith_restate as R

N = 2
# name: C, M, P, image extents, stride, Bayer mask
SHAPES = {
    "3d": (1, 24, (3, 5, 5), (3, 20, 70), 1, False),           # depth taps, a tile kernel cell's shape
    "c3": (3, 24, (5, 5), (20, 70), 1, True),                  # JDD: three image channels under the mosaic
    "s2": (1, 25, (7, 7), (22, 74), 2, False),                 # a strip kernel cell: code plane 11 x 37
}


@functools.lru_cache(maxsize=None)
def _data(name):
    C, M, P, sp, s, bayer = SHAPES[name]
    return R.stage_inputs(N, C, M, P, sp, s, seed=11 + M + len(sp) + s, bayer=bayer)


def _shrink32(u, tau):
    t = tau.reshape(tau.shape + (1,) * (u.dim() - 2))
    return u - torch.minimum(torch.maximum(u, -t), t)


def _honest_analysis(x, w, s, precision, kept=None):
    return R.honest_product(lambda a, b: R.analysis(a, b, s), x, w, precision, kept)


def _honest_reverse(d, s, precision, on, kept=None, w1=None):
    return (d["base"] + _honest_analysis(d["thin"], d["wA"] if w1 is None else w1, s, precision, kept)) * on


def _all_on(d):
    return torch.ones_like(d["gate"], dtype=torch.bool)


# ------------------------------------------------------------------------------------------------ the 2-D module
@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("M,P", [(32, 5), (24, 7)])
def test_at_one_channel_unit_stride_the_model_is_the_2d_model_bit_for_bit(M, P, precision):
    H, W = 20, 70
    d = R2.stage_inputs(N, M, P, H, W, seed=3 + M)
    on, neg = d["gate"] != 0, d["gate"] < 0
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for base, sgn in ((None, 1.0), (d["zin"], -1.0)):
        assert same(R.forward_stage(d["r"], d["wA"], d["tau"], base, sgn, precision),
                    R2.forward_stage(d["r"], d["wA"], d["tau"], base, sgn, precision))
    for base in (None, d["base"]):
        assert same(R.reverse_stage(d["thin"], d["wA"], on, base, precision), R2.reverse_stage(d["thin"], d["wA"], on, base, precision))
    for mask, sub, alpha in ((None, None, 1.0), (d["mask"], d["sub"], 1.0), (d["mask"], None, -1.0)):
        assert same(R.synth_assemble(d["zin"], d["wB"], precision, False, mask, sub, alpha),
                    R2.synth_assemble(d["zin"], d["wB"], precision, False, mask, sub, alpha))
    assert same(R.dtau_sums(d["gate"], on, neg, d["c"]), R2.dtau_sums(d["gate"], on, neg, d["c"]))
    a, b = R.crafted_split4_inputs(N, 1, M, (P, P), (H, W), seed=9), R2.crafted_split4_inputs(N, M, P, H, W, seed=9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_operators_are_the_definitions():
    """The strided pair against the oracle's own two lines, and as an adjoint pair: <A r, z> = <r, B z> in float64."""
    for name in SHAPES:
        C, M, P, sp, s, _ = SHAPES[name]
        d = _data(name)
        r, z, w = d["r"].double(), d["zin"].double(), d["wA"].double()
        Ar, Bz = R.analysis(r, w, s), R.synthesis(z, w, s)
        assert Ar.shape == z.shape and Bz.shape == r.shape
        assert abs(float((Ar * z).sum() - (r * Bz).sum())) < 1e-9 * float(Ar.abs().sum())
        # out[m, y, x] = sum_{c, i, j} w[m, c, i, j] r[c, s y - P/2 + i, s x - P/2 + j] at one interior element, by hand
        if len(sp) == 2:
            y, x, p = 4, 9, P[-1] // 2
            win = r[1, :, s * y - p:s * y + p + 1, s * x - p:s * x + p + 1]
            assert abs(float((win * w[5]).sum() - Ar[1, 5, y, x])) < 1e-12


# ------------------------------------------------------------------------------------------------ a correct implementation
@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_honest_fp32_implementation_is_inside_the_bound(name, precision):
    C, M, P, sp, s, _ = SHAPES[name]
    d = _data(name)
    worst = {}
    for first in (False, True):
        z, b = R.forward_stage(d["r"], d["wA"], d["tau"], None if first else d["zin"], 1.0 if first else -1.0, precision, s=s)
        acc = _honest_analysis(d["r"], d["wA"], s, precision)
        got = _shrink32(acc if first else d["zin"] - acc, d["tau"])
        bad, worst["first" if first else "fwd"] = R.violations_fp32(got, z, b)
        assert bad == 0
    on, neg = d["gate"] != 0, d["gate"] < 0
    for base in (d["base"], None):
        du, b = R.reverse_stage(d["thin"], d["wA"], on, base, precision, s=s)
        got = _honest_reverse(d, s, precision, on) if base is not None else _honest_analysis(d["thin"], d["wA"], s, precision) * on
        bad, worst["bwd" if base is not None else "bwd0"] = R.violations_fp32(got, du, b)
        assert bad == 0 and R.zeros_off_support(got, on) == 0
    got = _honest_reverse(d, s, precision, on)
    dt, bt = R.dtau_sums(got, on, neg, d["c"])
    t32 = torch.where(neg, got, -got).reshape(N, M, -1).sum(-1)
    bad, worst["dtau"] = R.violations_fp32(torch.stack([t32.sum(0), (d["c"][:, None] * t32).sum(0)]), dt, bt)
    assert bad == 0
    for mask, sub, alpha in ((d["mask"], d["sub"], 1.0), (d["mask"], None, -1.0), (None, None, 1.0)):
        val, b = R.synth_assemble(d["zin"], d["wB"], precision, False, mask, sub, alpha, s=s)
        got = alpha * R.honest_product(lambda a, c: R.synthesis(a, c, s), d["zin"], d["wB"], precision)
        got = got if mask is None else mask * got
        got = got if sub is None else got - sub
        bad, worst[f"synth{alpha:+.0f}"] = R.violations_fp32(got, val, b)
        assert bad == 0
    print(f"{name} {precision}: worst |err|/b " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    # round-to-nearest adds err by at most 2^-24 each, half of what the bound allows per term: an honest version cannot pass 0.5
    assert max(worst.values()) < 0.5


# ------------------------------------------------------------------------------------------------ mutations
def test_a_zeroed_tap_violates_the_bound():
    """One tap of one channel zeroed moves every element of that channel whose tap lies inside the clip by w r[.] ~ 0.1,
    against b ~ 1e-5: with the whole map on, at least half of the channel's elements, and no element of another channel."""
    C, M, P, sp, s, _ = SHAPES["3d"]
    d = _data("3d")
    w = d["wA"].clone()
    w[17, 0, 1, 2, 4] = 0.0                                         # the centre depth plane: present at every depth
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), d["base"], "split3", s=s)
    err = ~((_honest_reverse(d, s, "split3", _all_on(d), w1=w).double() - du).abs() <= b)
    assert int(err.sum()) >= du[:, 17].numel() // 2 and int(err[:, 17].sum()) == int(err.sum())


def test_a_zeroed_depth_plane_of_one_group_violates_the_bound():
    """Depth tap 0 reads frame d - 1: zeroing it changes nothing at d = 0 (the plane is absent there) and 25 taps' worth at
    the other 2 of 3 depths.  C = 3: one image channel's filters zeroed changes every element."""
    C, M, P, sp, s, _ = SHAPES["3d"]
    d = _data("3d")
    w = d["wA"].clone()
    w[:, 0, 0] = 0.0
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), d["base"], "split3", s=s)
    err = ~((_honest_reverse(d, s, "split3", _all_on(d), w1=w).double() - du).abs() <= b)
    assert int(err[:, :, 0].sum()) == 0 and int(err[:, :, 1:].sum()) > 0.9 * du[:, :, 1:].numel()
    d = _data("c3")
    w = d["wA"].clone()
    w[:, 2] = 0.0
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), d["base"], "split3")
    assert R.violations_fp32(_honest_reverse(d, 1, "split3", _all_on(d), w1=w), du, b)[0] > 0.9 * du.numel()


@pytest.mark.parametrize("name", ["3d", "c3"])
def test_two_groups_swapped_violate_the_bound(name):
    """Groups are (image channel, depth tap) pairs: two depth planes, or two image channels, of the bank exchanged."""
    C, M, P, sp, s, _ = SHAPES[name]
    d = _data(name)
    w = d["wA"].clone()
    if name == "3d":
        w[:, :, [0, 1]] = d["wA"][:, :, [1, 0]]
    else:
        w[:, [0, 2]] = d["wA"][:, [2, 0]]
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), d["base"], "split3", s=s)
    assert R.violations_fp32(_honest_reverse(d, s, "split3", _all_on(d), w1=w), du, b)[0] > 0.9 * du.numel()
    # the synthesis side: the col2im of group g added into image plane g'
    val, b = R.synth_assemble(d["zin"], d["wB"], "split3", s=s)
    wb = d["wB"].clone()
    if name == "3d":
        wb[:, :, [0, 2]] = d["wB"][:, :, [2, 0]]
    else:
        wb[:, [0, 1]] = d["wB"][:, [1, 0]]
    got = R.honest_product(lambda a, c: R.synthesis(a, c, s), d["zin"], wb, "split3")
    assert R.violations_fp32(got, val, b)[0] > 0.5 * val.numel()


def test_the_stride_2_col2im_geometry_violates_the_bound_when_wrong():
    """output_padding = 0 computes the same image without its last row and column (2 Hz - 1 by 2 Wz - 1): exactly those
    pixels are wrong.  A one-pixel shift puts every parity class on its neighbour's pixels: nearly every pixel is."""
    import torch.nn.functional as F
    C, M, P, sp, s, _ = SHAPES["s2"]
    d = _data("s2")
    H, W = sp
    val, b = R.synth_assemble(d["zin"], d["wB"], "split3", s=s)
    good = R.honest_product(lambda a, c: R.synthesis(a, c, s), d["zin"], d["wB"], "split3")
    assert R.violations_fp32(good, val, b)[0] == 0
    short = R.honest_product(lambda a, c: F.conv_transpose2d(a, c, stride=s, padding=P[-1] // 2), d["zin"], d["wB"], "split3")
    assert short.shape[-2:] == (H - 1, W - 1)
    got = torch.zeros_like(good)
    got[..., :H - 1, :W - 1] = short
    err = ~((got.double() - val).abs() <= b)
    assert int(err[..., :H - 1, :W - 1].sum()) == 0 and int(err.sum()) > 0.9 * N * (H + W - 1)
    for dims in (-1, -2):
        assert R.violations_fp32(torch.roll(good, 1, dims=dims), val, b)[0] > 0.9 * val.numel()
    # the analysis side: the strided correlation started one pixel late
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), None, "split3", s=s)
    late = _honest_analysis(torch.roll(d["thin"], -1, dims=-1), d["wA"], s, "split3")
    assert R.violations_fp32(late, du, b)[0] > 0.9 * du.numel()


@pytest.mark.parametrize("name", list(SHAPES))
def test_split3_without_lo_hi_violates_the_bound(name):
    """The dropped term is 2^-9 relative per product against a bound of about n 3 2^-23 with n <= 175 taps."""
    C, M, P, sp, s, _ = SHAPES[name]
    d = _data(name)
    du, b = R.reverse_stage(d["thin"], d["wA"], _all_on(d), d["base"], "split3", s=s)
    bad, _ = R.violations_fp32(_honest_reverse(d, s, "split3", _all_on(d), kept=((0, 0), (0, 1))), du, b)
    assert bad > 0.9 * du.numel()


@pytest.mark.parametrize("name", list(SHAPES))
def test_an_ignored_map_bit_violates_the_zero_predicate(name):
    C, M, P, sp, s, _ = SHAPES[name]
    d = _data(name)
    on = d["gate"] != 0
    ignored = on.clone()
    idx = tuple((~on).nonzero()[-7].tolist())                 # an off element near the end of the last sample
    ignored[idx] = True
    got = _honest_reverse(d, s, "split3", ignored)
    du, b = R.reverse_stage(d["thin"], d["wA"], on, d["base"], "split3", s=s)
    assert R.zeros_off_support(got, on) == 1 and R.violations_fp32(got, du, b)[0] == 1
    assert R.zeros_off_support(_honest_reverse(d, s, "split3", on), on) == 0


# ------------------------------------------------------------------------------------------------ the lo . lo products
@pytest.mark.parametrize("name", list(SHAPES))
def test_crafted_inputs_tell_split4_from_split3(name):
    C, M, P, sp, s, _ = SHAPES[name]
    r, w = R.crafted_split4_inputs(N, C, M, P, sp, seed=40 + M)
    hi, lo = R.parts(r)
    assert torch.equal(lo, hi * 2.0 ** -9)
    assert int((w != 0).reshape(M, -1).sum(1).max()) == 1 and len({tuple(i[1:]) for i in w.nonzero().tolist()}) > M // 2
    on = torch.ones((N, M) + tuple(sp[:-2]) + (sp[-2] // s, sp[-1] // s), dtype=torch.bool)
    m4, b4 = R.reverse_stage(r, w, on, None, "split4", s=s)
    m3, b3 = R.reverse_stage(r, w, on, None, "split3", s=s)
    nz = int((m4 != 0).sum())
    assert nz > 0.6 * m4.numel()                              # a tap outside the clip (border, absent frame) gives a zero
    h4, h3 = _honest_analysis(r, w, s, "split4"), _honest_analysis(r, w, s, "split3")
    assert R.violations_fp32(h4, m4, b4)[0] == 0 and R.violations_fp32(h3, m3, b3)[0] == 0
    assert R.violations_fp32(h4, m3, b3)[0] == nz and R.violations_fp32(h3, m4, b4)[0] == nz
    ratio = ((m4 - m3).abs()[m4 != 0] / b4[m4 != 0]).min()
    assert 7.5 < float(ratio) < 8.5                           # lo . lo = 2^-18 |x w| against b = 4 * 2^-23 |x w| (1 + 2^-9)^2
