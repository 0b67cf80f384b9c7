"""The float64 model of the fused generic tier (fusedg_arith_restate.py) and its bound, on the CPU: at C = 1, stride 1, 2-D it
is the fused 2-D model bit for bit; an honest fp32 implementation of the definition (the kept products one by one through
torch's float32 conv*, summed in float32) stays inside the bound at a 3-D, a C = 3 masked and a stride-2 shape;
implementations that are subtly wrong in the ways this tier can be (a tap, a depth plane, the order of the groups, the
geometry of the stride-2 col2im, a dropped product, a map bit) leave it.  The mutation counts are reasoned in the tests.
Second part: the exactly-summable stage inputs at this tier's geometries -- the cap for every input of
the GPU cells, an honest fp32 evaluation equal to the model in two summation orders, and the mutant table."""
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


# ------------------------------------------------------------------------------------------------ exactly-summable stages
# the three recipes at a 3-D, a C = 3 Bayer and a stride-2 shape of the GPU cells.
def _ops(s):
    return (lambda a, b: R.analysis(a, b, s)), (lambda a, b: R.synthesis(a, b, s))


def _h_code(mode, e, s, prec, w=None):
    w = e["wA"] if w is None else w
    if mode in ("first", "fwd"):
        acc = _honest_analysis(e["r"], w, s, prec)
        return _shrink32(acc if mode == "first" else e["zin"] - acc, e["tau"])
    acc = _honest_analysis(e["thin"], w, s, prec)
    return (acc + e["base"] if mode == "bwd" else acc) * (e["gate"] != 0)


def _h_thin(fwd, e, s, prec, z, masked=True, flip=False, w=None):
    w = e["wB"] if w is None else w
    z, w = (torch.flip(z, (1,)), torch.flip(w, (0,))) if flip else (z, w)
    acc = R.honest_product(_ops(s)[1], z, w, prec)
    acc = e["mask"] * acc if masked else acc
    return acc - e["sub"] if fwd else -acc


def _by_hand(x, w, P, s, prec):
    """A x over an im2col written out (generic_arith_restate.im2col: its depth stride is s, and the strided shapes here have no
    depth), the C * taps axis in a random order."""
    import generic_arith_restate as G
    col = G.im2col(x, tuple(P), s)                                            # (N, C, T, Z)
    M, K = w.shape[0], col.shape[1] * col.shape[2]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(2))
    colk, wk = col.reshape(N, K, -1)[:, perm].contiguous(), w.reshape(M, K)[:, perm].contiguous()
    acc = None
    for (i, j) in R._KEPT[prec]:
        t = R.parts(wk)[j].float() @ R.parts(colk)[i].float()
        acc = t if acc is None else acc + t
    return acc


def _h_dt(e, du, perm=None):
    t = (torch.where(e["gate"] < 0, du, -du) * (e["gate"] != 0)).reshape(N, du.shape[1], -1)
    per = (t if perm is None else t[:, :, perm]).sum(-1)
    return torch.stack([per.sum(0), (e["c"][:, None] * per).sum(0)])


@pytest.mark.parametrize("precision", R.PRECISIONS)
@pytest.mark.parametrize("recipe", R.RECIPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_stage_inputs_are_summable_and_fp32_reproduces_the_model_in_two_orders(name, recipe, precision):
    C, M, P, sp, s, bayer = SHAPES[name]
    held = R.EXACT_HELD[recipe]
    for mode in ("first", "fwd", "bwd", "bwd0"):
        e = R.exact_stage_inputs(recipe, precision, N, C, M, P, sp, s, seed=5 + M, first=mode == "first", bayer=bayer)
        assert not bayer or torch.equal(e["mask"], R.bayer_mask(N, *sp))
        model = R.exact_stage_model(mode, e, precision, s)
        for k in (k for k in held if k in model):
            val, S, q = model[k]
            assert R.exact_cap_ok(S, q), (mode, k, R.cap_quanta(S, q))
            assert bool((val / q == torch.round(val / q)).all()), (mode, k)
        code = model["code"][0].float()
        if recipe == "int":
            assert not R.parts(code)[1].any()
        elif recipe == "hilo-p" and mode in ("fwd", "bwd"):
            assert bool(R.parts(code)[1].any())
        fwd = mode in ("first", "fwd")
        for order in (1, 2):
            if order == 1:
                got = _h_code(mode, e, s, precision)
            else:                                             # by hand: one matrix product per kept product, channels x taps permuted
                acc = _by_hand(e["r"] if fwd else e["thin"], e["wA"], P, s, precision).reshape(code.shape)
                got = (_shrink32(acc if mode == "first" else e["zin"] - acc, e["tau"]) if fwd
                       else (acc + e["base"] if mode == "bwd" else acc) * (e["gate"] != 0))
            assert R.violations_exact(got, model["code"][0])[0] == 0, (mode, order, "code")
            if "thin" in held:
                assert R.violations_exact(_h_thin(fwd, e, s, precision, got, flip=order == 2), model["thin"][0])[0] == 0, (mode, order)
            if not fwd and "dt" in held:
                perm = None if order == 1 else torch.randperm(got[0, 0].numel(), generator=torch.Generator().manual_seed(1))
                assert R.violations_exact(_h_dt(e, got, perm), model["dt"][0])[0] == 0, (mode, order, "dt")


@pytest.mark.parametrize("part", range(8))
def test_the_cap_holds_for_every_exact_input_of_the_gpu_cells(part):
    """test_gpu_fusedg_cells.exact_inputs_of_this_file: for every exact input a GPU test feeds a kernel and every output it holds
    to equality, the model's own S_e / quantum < CAP_QUANTA (in eight parts); the integer chain's codes have no lo part.  A
    condition on the recipes' densities, not a measurement: no case is skipped for failing it."""
    import test_gpu_fusedg_cells as T
    every = T.exact_inputs_of_this_file()
    n_int = 2 * len(T.TILE_CELLS) + len(T.STRIP_CELLS)         # cells x arithmetics of the integer chain
    assert len(every) >= 4 * n_int and len(T.TILE_CELLS) == 27 and len(T.STRIP_CELLS) == 36
    assert {(c.want["P"], c.want["G"]) for c in T.HILO_TILE} == {(c.want["P"], c.want["G"]) for c in T.TILE_CELLS}
    assert {(c.want["P"], c.s) for c in T.HILO_STRIP} == {(c.want["P"], c.s) for c in T.STRIP_CELLS}
    assert {T.BY_ID[cid].want["P"] for k, cid in T.RSC_CASES if k == "strip"} == {3, 5, 7} == {T.BY_ID[cid].want["P"] for k, cid in T.RSC_CASES if k == "stripg"}
    for (cid, prec, recipe, mode) in every[part::8]:
        model = T.exact_model(cid, prec, recipe, mode)
        for k in R.EXACT_HELD[recipe]:
            if k in model:
                assert R.cap_quanta(model[k][1], model[k][2]) < R.CAP_QUANTA, (cid, prec, recipe, mode, k)
        if recipe == "int":
            assert not R.parts(model["code"][0].float())[1].any(), (cid, mode)


# ---- the mutant table of this tier (split3): each mutant on the seeded data of a shape against b and on exact operands
# against equality.  x: the operands with "z" (the code the synthesis half is fed), "du" (a reverse stage's output), "s".
def _m_syn(x, minus=None, got=None):
    s = x["s"]
    got = R.honest_product(_ops(s)[1], x["z"], x["wB"], "split3") - minus if got is None else got
    return x["mask"] * got - x["sub"], R.synth_assemble(x["z"], x["wB"], "split3", False, x["mask"], x["sub"], 1.0, s=s)


def _center(w):
    return (slice(None), slice(None)) + tuple(p // 2 for p in w.shape[2:-1]) + (w.shape[-1] // 2 + 1,)


def _m_syn_lo_hi_one_tap(x):
    w = torch.zeros_like(x["wB"])
    w[_center(w)] = x["wB"][_center(w)]
    return _m_syn(x, _ops(x["s"])[1](R.parts(x["z"])[1].float(), R.parts(w)[0].float()))


def _m_syn_lo_hi_one_channel(x):
    m = x["z"].shape[1] // 2 + 1
    return _m_syn(x, _ops(x["s"])[1](R.parts(x["z"][:, m:m + 1])[1].float(), R.parts(x["wB"][m:m + 1])[0].float()))


def _m_syn_hi_lo_last_quad(x):
    return _m_syn(x, _ops(x["s"])[1](R.parts(x["z"][:, -4:])[0].float(), R.parts(x["wB"][-4:])[1].float()))


def _m_parity_class(x):
    """One of the four parity classes of the stride-2 col2im never added: output rows 1 mod 2, columns 0 mod 2."""
    got = R.honest_product(_ops(x["s"])[1], x["z"], x["wB"], "split3")
    got[..., 1::2, 0::2] = 0.0
    return _m_syn(x, got=got)


def _m_channel_leak(x):
    """A channel >= M in the last tile: the code and filter of channel 0 once more."""
    got = R.honest_product(_ops(x["s"])[1], torch.cat([x["z"], x["z"][:, :1]], 1), torch.cat([x["wB"], x["wB"][:1]], 0), "split3")
    return _m_syn(x, got=got)


def _m_dt_one_pixel(x):
    du = x["du"].clone()
    hit = du[1].abs().sum(0).nonzero()
    du[(1, slice(None)) + tuple(hit[len(hit) // 3].tolist())] = 0.0
    return _h_dt(x, du), R.dtau_sums(x["du"], x["gate"] != 0, x["gate"] < 0, x["c"])


def _m_rev(x, w=None, on=None, parts_of=None):
    on_true = x["gate"] != 0
    if parts_of is None:
        acc = _honest_analysis(x["thin"], x["wA"] if w is None else w, x["s"], "split3")
    else:
        a, b = parts_of(x["thin"]), parts_of(x["wA"])
        acc = sum(R.analysis(a[i], b[j], x["s"]) for (i, j) in R._KEPT["split3"])
    return (x["base"] + acc) * (on_true if on is None else on), R.reverse_stage(x["thin"], x["wA"], on_true, x["base"], "split3", s=x["s"])


def _m_zeroed_tap(x):
    w = x["wA"].clone()
    idx = tuple(w[3].nonzero()[len(w[3].nonzero()) // 2].tolist())
    w[(3,) + idx] = 0.0
    return _m_rev(x, w=w)


def _m_depth_plane(x):
    w = x["wA"].clone()
    w[:, :, w.shape[2] // 2 + 1] = 0.0
    return _m_rev(x, w=w)


def _m_ignored_map_bit(x):
    on = x["gate"] != 0
    on[tuple((~on).nonzero()[-7].tolist())] = True
    return _m_rev(x, on=on)


def _m_truncating_split(x):
    def trunc_parts(t):
        hi = R2.bf16_trunc(t).float()
        return hi, R2.bf16_trunc(t - hi).float()
    return _m_rev(x, parts_of=trunc_parts)


# mutant: (function, exact recipe, {shape: does the bound b catch it on the seeded data})
MUTANTS = {
    "synthesis: lo.hi dropped at one tap of every filter": (_m_syn_lo_hi_one_tap, "hilo-p", {"c3": True, "s2": True, "s2long": False}),
    "synthesis: lo.hi dropped for one channel": (_m_syn_lo_hi_one_channel, "hilo-p", {"c3": True, "s2": True, "s2long": False}),
    "synthesis: hi.lo dropped for the last channel quad": (_m_syn_hi_lo_last_quad, "hilo-p", {"c3": True, "s2": True, "s2long": False}),
    "dt: one code pixel of one sample missing from the sum": (_m_dt_one_pixel, "hilo-p", {"3d": True, "s2": True}),
    "stride-2 col2im: one parity class dropped": (_m_parity_class, "hilo-p", {"s2": True, "s2long": True}),
    "a channel >= M leaking into the last tile": (_m_channel_leak, "int", {"c3": True, "s2": True}),
    "analysis: a zeroed tap": (_m_zeroed_tap, "hilo-a", {"3d": True, "c3": True, "s2": True}),
    "analysis: a dropped depth plane": (_m_depth_plane, "hilo-a", {"3d": True}),
    "an ignored map bit": (_m_ignored_map_bit, "hilo-a", {"s2": True}),
    "lo = bf16_trunc instead of round-to-nearest-even": (_m_truncating_split, "hilo-a", {"3d": True, "c3": True}),
}
LONG = {"s2long": (1, 185, (7, 7), (22, 74), 2, False)}       # the strip kernel's longest synthesis sum: P7S2MT6M185


@functools.lru_cache(maxsize=None)
def _mutant_operands(name, recipe):
    C, M, P, sp, s, bayer = {**SHAPES, **LONG}[name]
    if recipe is None:
        d = _data(name) if name in SHAPES else R.stage_inputs(N, C, M, P, sp, s, seed=11 + M + len(sp) + s, bayer=bayer)
        return dict(d, s=s, z=d["zin"], du=_honest_reverse(d, s, "split3", d["gate"] != 0))
    e = R.exact_stage_inputs(recipe, "split3", N, C, M, P, sp, s, seed=5 + M, bayer=bayer)
    return dict(e, s=s, z=R.exact_stage_model("fwd", e, "split3", s)["code"][0].float(),
                du=R.exact_stage_model("bwd", e, "split3", s)["code"][0].float())


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_leaves_the_exact_predicate_and_the_bound_only_where_the_table_says(mutant):
    """Every mutant leaves the exact predicate.  Where the bound lets one through on the seeded data, that it passes b is asserted
    too, so that a later tightening of b shows up."""
    fn, recipe, table = MUTANTS[mutant]
    for name, caught in table.items():
        got, model = fn(_mutant_operands(name, None))
        bad, worst = R.violations_fp32(got, *model)
        got_e, model_e = fn(_mutant_operands(name, recipe))
        off = R.violations_exact(got_e, model_e[0])[0]
        print(f"{mutant} [{name}]: worst |err|/b {worst:.3g}, {bad} outside b; exact ({recipe}): {off} of {got_e.numel()} differ")
        assert off > 0, (mutant, name)
        assert (bad > 0) == caught, (mutant, name, bad, worst)
