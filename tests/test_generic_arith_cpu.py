"""The float64 model of the sparse matrix-core tier (generic_arith_restate.py), its bound and its exactly-summable inputs, on the
CPU: at C = 1, stride 1, 2-D the operators are the fused 2-D model's bit for bit and an adjoint pair; an honest fp32
implementation of the definition stays inside the bound at a 9 x 9 x 5 stride-2 shape, a C = 3 shape and a 3 x 3 stride-2
shape, and on the exact inputs reproduces the model bit for bit in two summation orders; implementations that are subtly
wrong in the ways this tier can be leave the bound or the exact predicate (MUTANTS says which).  The summability cap is
asserted here for every exact input the GPU cells use."""
import functools

import pytest
import torch
import torch.nn.functional as F

import fused2d_arith_restate as R2
import generic_arith_restate as R

N = 2
# name: C, M, P, image extents, stride
SHAPES = {
    "d952": (1, 8, (9, 9, 5), (4, 12, 20), 2),       # the shipped 3-D bank: 9 depth taps of 9 x 5 planes, stride 2 in depth too
    "c3": (3, 24, (5, 5), (20, 38), 1),              # three image channels
    "s2": (1, 25, (3, 3), (22, 74), 2),              # 3 x 3 at stride 2, code plane 11 x 37
}
# the filter gradient at the length of a GPU cell's sums (16 x 40 x 70 code pixels per element): where the bound is loose
LONG = {"wlong": (1, 8, (3, 3), (40, 70), 1)}
N_OF = {"wlong": 16}


@functools.lru_cache(maxsize=None)
def _data(name, kind="random"):
    C, M, P, sp, s = {**SHAPES, **LONG}[name]
    n = N_OF.get(name, N)
    if kind == "random":
        d = R.stage_inputs(n, C, M, P, sp, s, seed=5 + M + len(sp) + s)
        d["F"] = d["z"]
        return d
    d = R.exact_inputs(n, C, M, P, sp, s, seed=6 + M, integer=kind == "integer")
    d["mask"] = (d["x2"] != 0).float()
    d["sub"] = d["x2"]
    return d


def _ana(s):
    return lambda a, b: R.analysis(a, b, s)


def _syn(s):
    return lambda a, b: R.synthesis(a, b, s)


def _wg(P, s):
    return lambda a, b: R.filter_grad(a, b, P, s)


def _gated(t, gate):
    return t * (gate != 0)


# honest fp32 versions of the three forms the mutants are measured on
def _h_analysis(d, s, x=None, w=None, gate=True, kept=None, op=None):
    acc = R.honest_product(op or _ana(s), d["x"] if x is None else x, d["w"] if w is None else w, "split3", kept)
    return (_gated(d["u"], d["gate"]) if gate else d["u"]) + acc


def _m_analysis(d, s):
    return R.analysis_form(d["x"], d["w"], s, 1.0, zin=d["u"], gate=d["gate"])


def _h_synth(d, s, z=None, w=None, kept=None, op=None):
    z = _gated(d["z"], d["gate"]) if z is None else z
    return d["mask"] * R.honest_product(op or _syn(s), z, d["w"] if w is None else w, "split3", kept) - d["sub"]


def _m_synth(d, s):
    return R.synth_form(d["z"], d["w"], s, gate=d["gate"], mask=d["mask"], sub=d["sub"])


def _h_wgrad(d, P, s, Fc=None, kept=None):
    return -1.0 * R.honest_product(_wg(P, s), d["F"] if Fc is None else Fc, d["x"], "split3", kept)


def _m_wgrad(d, P, s):
    return R.wgrad_form(d["F"], d["x"], P, s, -1.0)


# ------------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize("M,P", [(32, 5), (24, 7)])
def test_at_one_channel_unit_stride_the_operators_are_the_2d_models_bit_for_bit(M, P):
    H, W = 20, 70
    d = R2.stage_inputs(N, M, P, H, W, seed=3 + M)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for base, sgn in ((None, 1.0), (d["zin"], -1.0)):
        assert same(R.analysis_form(d["r"], d["wA"], 1, sgn, zin=base, tau=d["tau"]),
                    R2.forward_stage(d["r"], d["wA"], d["tau"], base, sgn, "split3"))
    on = d["gate"] != 0
    assert same(R.analysis_form(d["thin"], d["wA"], 1, 1.0, zin=d["base"], zsup=d["gate"]),
                R2.reverse_stage(d["thin"], d["wA"], on, d["base"], "split3"))
    for mask, sub, alpha in ((None, None, 1.0), (d["mask"], d["sub"], 1.0), (d["mask"], None, -1.0)):
        assert same(R.synth_form(d["zin"], d["wB"], 1, None, mask, sub, alpha),
                    R2.synth_assemble(d["zin"], d["wB"], "split3", False, mask, sub, alpha))
    assert same(R.wgrad_form(d["zin"], d["r"], (P, P), 1, -1.0), R2.wgrad(d["zin"], d["r"], -1.0, P, "split3"))
    assert same(R.dtau_sums(d["gate"], on, d["gate"] < 0, d["c"]), R2.dtau_sums(d["gate"], on, d["gate"] < 0, d["c"]))
    # (the im2col product and the 2-D module's convolution add in different orders: equal to float64 rounding, and the
    # float64 values above round to the same model all the same)
    ga, gb = R.filter_grad(d["zin"].double(), d["r"].double(), (P, P)), R2.filter_grad(d["zin"].double(), d["r"].double(), P)
    assert float((ga - gb).abs().max()) < 1e-10


def test_the_operators_are_the_definitions_and_an_adjoint_pair():
    """<A x, z> = <x, B z> and <A x, z> = <w, z (x) x> in float64; one interior element of A x by hand."""
    for name, (C, M, P, sp, s) in SHAPES.items():
        d = _data(name)
        x, z, w = d["x"].double(), d["z"].double(), d["w"].double()
        Ax, Bz, G = R.analysis(x, w, s), R.synthesis(z, w, s), R.filter_grad(z, x, P, s)
        assert Ax.shape == z.shape and Bz.shape == x.shape and G.shape == w.shape
        scale = float(Ax.abs().sum())
        assert abs(float((Ax * z).sum() - (x * Bz).sum())) < 1e-9 * scale
        assert abs(float((Ax * z).sum() - (w * G).sum())) < 1e-9 * scale
        if len(sp) == 2:
            y, xx, p = 4, 9, P[-1] // 2
            win = x[1, :, s * y - p:s * y + p + 1, s * xx - p:s * xx + p + 1]
            assert abs(float((win * w[5]).sum() - Ax[1, 5, y, xx])) < 1e-12
        else:                                       # depth stride follows s: code plane 1 reads frames 2 - 4 .. 2 + 4
            zd, y, xx = 1, 3, 5
            pd, ph, pw = (q // 2 for q in P)
            xp = F.pad(x, (pw, pw, ph, ph, pd, pd))
            win = xp[1, :, s * zd:s * zd + P[0], s * y:s * y + P[1], s * xx:s * xx + P[2]]
            assert abs(float((win * w[5]).sum() - Ax[1, 5, zd, y, xx])) < 1e-12


def test_the_csr_epilogue_and_thresholds_are_the_definitions():
    """prox_csr32 against the oracle's prox_CSR / prox_CSR_f2 in float32; the map thresholds t0 + c * t1 with a rounded product."""
    from oracle import cdl_oracle as O
    d = _data("s2")
    lam, g1, g2 = R.prox_thresholds32(d["lam"], d["g1"], d["g2"], d["u"])
    assert torch.equal(R.prox_csr32(d["u"], d["zp"], lam, g1), O.prox_csr(d["u"], d["zp"], lam, g1))
    assert torch.equal(R.prox_csr32(d["u"], d["zp"], lam, g1, d["za"], g2), O.prox_csr_f2(d["u"], d["zp"], d["za"], lam, g1, g2))
    t = R.thresholds(d["tau"], d["u"], d["cmap"], d["tslope"])
    want = d["tau"][:, :, None, None] + d["cmap"] * d["tslope"][None, :, None, None]
    assert t.shape == d["u"].shape and torch.equal(t, want.double())
    tm = R.prox_thresholds32(d["lam"], d["g1"], None, d["u"], d["cmap"], d["tslope3"])
    assert tm[2] is None and torch.equal(tm[1], d["g1"][:, :, None, None] + d["cmap"] * d["tslope3"][1][None, :, None, None])
    u = torch.tensor([-1.0, -0.05, 0.0, 0.05, 1.0]).double()
    assert torch.allclose(R.shrink(u, torch.tensor(0.1).double()), torch.tensor([-0.9, 0.0, 0.0, 0.0, 0.9]).double())
    assert torch.allclose(R.shrink(u, torch.tensor(-0.1).double()), torch.tensor([-1.1, -0.15, 0.0, 0.15, 1.1]).double())


# ------------------------------------------------------------------------------------------------ a correct implementation
@pytest.mark.parametrize("name", list(SHAPES))
def test_honest_fp32_implementation_is_inside_the_bound(name):
    C, M, P, sp, s = SHAPES[name]
    d = _data(name)
    worst = {}
    acc = R.honest_product(_ana(s), d["x"], d["w"], "split3")
    t4 = lambda t: R._rows(t, acc)
    forms = {
        "plain": (acc, R.analysis_form(d["x"], d["w"], s)),
        "first": (R._st32(acc, t4(d["tau"])), R.analysis_form(d["x"], d["w"], s, tau=d["tau"])),
        "iter": (R._st32(d["z"] - acc, t4(d["tau"])), R.analysis_form(d["x"], d["w"], s, -1.0, zin=d["z"], tau=d["tau"])),
        "gated": (_h_analysis(d, s), _m_analysis(d, s)),
        "map": (R._st32(d["z"] - acc, R.thresholds(d["tau"], acc, d["cmap"], d["tslope"]).float()),
                R.analysis_form(d["x"], d["w"], s, -1.0, zin=d["z"], tau=d["tau"], cmap=d["cmap"], tslope=d["tslope"])),
        "rev": ((d["u"] + 0.5 * acc) * (d["z"] != 0), R.analysis_form(d["x"], d["w"], s, 0.5, zin=d["u"], zsup=d["z"])),
        "synth": (_h_synth(d, s), _m_synth(d, s)),
        "wgrad": (_h_wgrad(d, P, s), _m_wgrad(d, P, s)),
        "wgrad gated": (0.5 * R.honest_product(_wg(P, s), _gated(d["u"], d["gate"]), d["x"], "split3"),
                        R.wgrad_form(d["u"], d["x"], P, s, 0.5, gate=d["gate"])),
    }
    for k, (got, (val, b)) in forms.items():
        bad, worst[k] = R.violations_fp32(got, val, b)
        assert bad == 0, (k, bad, worst[k])
    rev = forms["rev"][0]
    on, neg = d["z"] != 0, d["z"] < 0
    assert R.zeros_off_support(rev, on) == 0
    t32 = torch.where(neg, rev, -rev) * on
    dt, bt = R.dtau_sums(rev, on, neg, d["c"])
    per = t32.reshape(N, M, -1).sum(-1)
    bad, worst["dt"] = R.violations_fp32(torch.stack([per.sum(0), (d["c"][:, None] * per).sum(0)]), dt, bt)
    assert bad == 0
    dtm, btm = R.dtau_sums_map(rev, on, neg, d["cmap"])
    dims = (0,) + tuple(range(2, rev.dim()))
    bad, worst["dt map"] = R.violations_fp32(torch.stack([t32.sum(dims), (d["cmap"] * t32).sum(dims)]), dtm, btm)
    assert bad == 0
    print(f"{name}: worst |err|/b " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) < 0.5              # round-to-nearest adds err by at most 2^-24 each: half of what b allows


# ------------------------------------------------------------------------------------------------ the exact inputs
def _exact_forms(d, P, s):
    """{form: (model value, S_e)} of the forms the GPU cells compare bit for bit."""
    a = lambda t: t.abs()
    S_ana = R.abs_sum(_ana(s), d["x"], d["w"]) + a(d["u"])
    S_syn = R.abs_sum(_syn(s), _gated(d["z"], d["gate"]), d["w"]) + a(d["sub"])
    S_wg = R.abs_sum(_wg(P, s), d["F"], d["x"])
    return {"analysis": (_m_analysis(d, s)[0], S_ana), "synth": (_m_synth(d, s)[0], S_syn), "wgrad": (_m_wgrad(d, P, s)[0], S_wg)}


@pytest.mark.parametrize("kind", ["hilo", "integer"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_inputs_are_summable_and_fp32_reproduces_the_model_in_two_orders(name, kind):
    C, M, P, sp, s = SHAPES[name]
    d = _data(name, kind)
    q = d["quantum"]
    for k in ("x", "w", "z", "u", "F"):                        # the parts are what the recipe says
        hi, lo = R.parts(d[k])
        assert set(hi.unique().tolist()) <= ({0.0, 1.0, -1.0, 2.0, -2.0} if kind == "integer" else {0.0, 1.0, -1.0})
        assert set(lo.unique().tolist()) <= ({0.0} if kind == "integer" else {0.0, q, -q})
        assert kind == "integer" or bool((lo != 0).any())
    assert bool(((d["F"] != 0).sum(1) == 1).all())             # every code pixel is hit in exactly one channel
    forms = _exact_forms(d, P, s)
    for k, (val, S) in forms.items():
        assert R.exact_cap_ok(S, q), (k, float(S.max()) / q)
        assert bool((val / q == torch.round(val / q)).all())
    flip = lambda t, dims: torch.flip(t, dims)
    sdims = tuple(range(2, 2 + len(sp)))
    # order 1: torch's own; order 2: the operands reversed along the summed axes (taps / channels / pixels)
    got1 = _h_analysis(d, s)
    col = R.im2col(d["x"], P, s)                               # (N, C, T, Z): the same sums by hand, taps in a random order
    permk = torch.randperm(col.shape[1] * col.shape[2], generator=torch.Generator().manual_seed(2))
    colk = col.reshape(N, -1, col.shape[-1])[:, permk].contiguous()
    wk = d["w"].reshape(M, -1)[:, permk].contiguous()
    acc = None
    for (i, j) in R._KEPT["split3"]:
        t = R.parts(wk)[j].float() @ R.parts(colk)[i].float()
        acc = t if acc is None else acc + t
    got2 = acc.reshape(got1.shape) + _gated(d["u"], d["gate"])
    assert R.mismatches(got1, forms["analysis"][0]) == 0 and R.mismatches(got2, forms["analysis"][0]) == 0
    got1 = _h_synth(d, s)
    got2 = _h_synth(d, s, z=flip(_gated(d["z"], d["gate"]), (1,)), w=flip(d["w"], (0,)))
    assert R.mismatches(got1, forms["synth"][0]) == 0 and R.mismatches(got2, forms["synth"][0]) == 0
    got1 = _h_wgrad(d, P, s)
    perm = torch.randperm(N * d["F"][0, 0].numel(), generator=torch.Generator().manual_seed(1))
    col = R.im2col(d["x"], P, s)                               # the same sum with its pixels in a random order, by hand
    Z = col.shape[-1]
    Fm = d["F"].reshape(N, M, Z).transpose(0, 1).reshape(M, N * Z)[:, perm]
    cm = col.permute(0, 3, 1, 2).reshape(N * Z, -1)[perm]
    got2 = None
    for (i, j) in R._KEPT["split3"]:
        t = R.parts(Fm.contiguous())[i].float() @ R.parts(cm.contiguous())[j].float()
        got2 = t if got2 is None else got2 + t
    got2 = -got2.reshape(got1.shape)
    assert R.mismatches(got1, forms["wgrad"][0]) == 0 and R.mismatches(got2, forms["wgrad"][0]) == 0


@pytest.mark.parametrize("part", range(8))
def test_the_cap_holds_for_every_exact_input_of_the_gpu_cells(part):
    """test_gpu_generic_cells.exact_inputs_of_this_file: the summability condition of every exact input a GPU test feeds a
    kernel (in eight parts), and every code pixel of the filter-gradient operands hit in exactly one channel."""
    import test_gpu_generic_cells as G
    every = G.exact_inputs_of_this_file()
    assert len(every) >= 6 + 2 * (len(G.SYN_CELLS) + len(G.WGM_CELLS))
    for kind, cid, variant, aligned in every[part::8]:
        d = G.exact_data(kind, cid, variant, aligned)
        c = G._sized(G.BY_ID[cid], kind, aligned)
        for k, quanta in G.exact_cap_quanta(kind, c, d, variant).items():
            assert quanta < R.CAP_QUANTA, (kind, cid, variant, aligned, k, quanta)
        if kind == "wgm":
            for k in ("F", "F2"):
                assert bool(((d[k] != 0).sum(1) == 1).all()), (cid, k)


def test_the_sign_mixed_thresholds_leave_out_under_one_percent_on_the_model():
    """test_gpu_generic_cells.SIGN_MIXED: with thresholds of both signs the shrinkage jumps at u = 0, so the cell compares where
    |u| > b only; the seeds are chosen so that the model alone leaves out less than 1 % of the elements."""
    import test_gpu_generic_cells as G
    for cell in G.SIGN_MIXED:
        d = G.cell_data(cell.id)
        assert bool((d["tau"] < 0).any()) and bool((d["tau"] > 0).any())
        _, b, u = R.analysis_form(d["x"], d["w"], cell.s, -1.0, zin=d["z"], tau=d["tau"], with_u=True)
        out = int((u.abs() <= b).sum())
        assert out <= 0.01 * u.numel(), (cell.id, out, u.numel())


# ------------------------------------------------------------------------------------------------ mutations
def _w_without_a_tap(d):
    w = d["w"].clone()
    idx = tuple(w[3].nonzero()[len(w[3].nonzero()) // 2].tolist())       # a tap that is there (the exact banks are sparse)
    w[(3,) + idx] = 0.0
    return w


def _m_zeroed_tap(d, P, s):
    return "analysis", _h_analysis(d, s, w=_w_without_a_tap(d))


def _m_dropped_depth_plane(d, P, s):
    w = d["w"].clone()
    w[:, :, P[0] // 2 + 1] = 0.0
    return "analysis", _h_analysis(d, s, w=w)


def _m_depth_stride_ignored(d, P, s):
    """Code plane zd reads frames zd - pd .. instead of s zd - pd ..: stride 1 in depth, the first D / s planes kept."""
    pad = tuple(p // 2 for p in P)
    op = lambda a, b: F.conv3d(a, b, stride=(1, s, s), padding=pad)[:, :, :a.shape[2] // s]
    return "analysis", _h_analysis(d, s, op=op)


def _m_plane_transposed(d, P, s):
    """The 9 x 5 plane's 45 values read as 5 rows of 9."""
    w = d["w"]
    wt = w.reshape(w.shape[:3] + (P[2], P[1]))
    return "analysis", _h_analysis(d, s, w=wt)


def _m_gate_ignored(d, P, s):
    return "analysis", _h_analysis(d, s, gate=False)


def _m_shift_at_stride_2(d, P, s):
    return "analysis", _h_analysis(d, s, x=torch.roll(d["x"], -1, dims=-1))


def _m_channel_leak(d, P, s):
    """A 26th channel in the last 32-channel tile: the code and filter of channel 0 once more."""
    z = _gated(d["z"], d["gate"])
    return "synth", _h_synth(d, s, z=torch.cat([z, z[:, :1]], 1), w=torch.cat([d["w"], d["w"][:1]], 0))


def _m_output_padding_0(d, P, s):
    pad = tuple(p // 2 for p in P)
    ct = F.conv_transpose2d if len(P) == 2 else F.conv_transpose3d
    short = d["mask"] * 0
    got = R.honest_product(lambda a, b: ct(a, b, stride=s, padding=pad), _gated(d["z"], d["gate"]), d["w"], "split3")
    short[tuple(slice(0, n) for n in got.shape)] = got
    return "synth", d["mask"] * short - d["sub"]


def _m_synth_shift(d, P, s):
    z = _gated(d["z"], d["gate"])
    return "synth", d["mask"] * torch.roll(R.honest_product(_syn(s), z, d["w"], "split3"), 1, dims=-1) - d["sub"]


def _m_no_lo_hi_analysis(d, P, s):
    return "analysis", _h_analysis(d, s, kept=((0, 0), (0, 1)))


def _m_no_lo_hi_synth(d, P, s):
    return "synth", _h_synth(d, s, kept=((0, 0), (0, 1)))


def _m_no_lo_hi_wgrad(d, P, s):
    return "wgrad", _h_wgrad(d, P, s, kept=((0, 0), (0, 1)))


def _m_missing_k_step(d, P, s):
    """16 consecutive code pixels of one row of one sample never multiplied."""
    Fc = d["F"].clone()
    Fc[(1, slice(None)) + (0,) * (Fc.dim() - 4) + (3, slice(16, 32))] = 0.0
    return "wgrad", _h_wgrad(d, P, s, Fc=Fc)


def _m_missing_row_part(d, P, s):
    """The lower half of the code rows of one sample never multiplied (one of two row parts of a tile)."""
    Fc = d["F"].clone()
    Fc[0, ..., Fc.shape[-2] // 2:, :] = 0.0
    return "wgrad", _h_wgrad(d, P, s, Fc=Fc)


# mutant: (function, shapes it applies to, what catches it: "both", or "exact" = ONLY the exact inputs do)
MUTANTS = {
    "zeroed tap": (_m_zeroed_tap, ("d952", "c3", "s2"), "both"),
    "dropped depth plane": (_m_dropped_depth_plane, ("d952",), "both"),
    "depth stride ignored": (_m_depth_stride_ignored, ("d952",), "both"),
    "9 x 5 plane read as 5 x 9": (_m_plane_transposed, ("d952",), "both"),
    "gate ignored": (_m_gate_ignored, ("d952", "c3", "s2"), "both"),
    "channel >= M leaking into the last tile": (_m_channel_leak, ("c3", "s2"), "both"),
    "output_padding = 0": (_m_output_padding_0, ("d952", "s2"), "both"),
    "one-pixel shift at stride 2 (analysis)": (_m_shift_at_stride_2, ("d952", "s2"), "both"),
    "one-pixel shift at stride 2 (col2im)": (_m_synth_shift, ("s2",), "both"),
    "split3 without lo.hi (analysis)": (_m_no_lo_hi_analysis, ("d952", "c3", "s2"), "both"),
    "split3 without lo.hi (synthesis)": (_m_no_lo_hi_synth, ("c3", "s2"), "both"),
    "split3 without lo.hi (filter gradient)": (_m_no_lo_hi_wgrad, ("wlong",), "exact"),
    "filter gradient: a missing 16-pixel k-step": (_m_missing_k_step, ("wlong",), "exact"),
    "filter gradient: a missing row part": (_m_missing_row_part, ("c3", "s2"), "both"),
}
_MODEL = {"analysis": lambda d, P, s: _m_analysis(d, s), "synth": lambda d, P, s: _m_synth(d, s), "wgrad": _m_wgrad}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_leaves_the_bound_or_the_exact_predicate(mutant):
    """Every mutant is run on the seeded random data against the bound and on the exact inputs against bit equality.  "both":
    each instrument catches it; "exact": the bound, loose by the length of the sum, lets it through and ONLY the exact inputs
    catch it."""
    fn, names, caught_by = MUTANTS[mutant]
    for name in names:
        C, M, P, sp, s = {**SHAPES, **LONG}[name]
        d, e = _data(name), _data(name, "hilo")
        form, got = fn(d, P, s)
        bad, worst = R.violations_fp32(got, *_MODEL[form](d, P, s))
        _, got_e = fn(e, P, s)
        off = R.mismatches(got_e, _MODEL[form](e, P, s)[0])
        print(f"{mutant} [{name}]: {bad} outside b (worst {worst:.3g}), {off} exact mismatches")
        assert off > 0, (mutant, name)
        assert (bad > 0) == (caught_by == "both"), (mutant, name, bad, worst)
