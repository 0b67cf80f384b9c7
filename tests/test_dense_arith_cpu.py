"""The float64 model of the dense matrix-core tier (dense_arith_restate.py), its bound and its exactly-summable inputs, on the
CPU: at C = 1 every form is generic_arith_restate's bit for bit; the two roles and the filter gradient are an adjoint triple at
3 x 5 x 3 and 5 x 3 banks; an honest fp32 implementation of the definitions stays inside the bound in every form and on the
exact inputs reproduces the model bit for bit in two summation orders; the filter-gradient plan restated gives each
filter-gradient cell the property it is there for; implementations that are subtly wrong in the ways this tier can be leave
the bound or the exact predicate (MUTANTS says which).  The summability cap and the 1 % cap of the sign-mixed case are
asserted here for every input the GPU cells use."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dense_arith_restate as R
import generic_arith_restate as G

N = 2
# name: C, M, P, image extents
SHAPES = {
    "t353": (20, 24, (3, 5, 3), (2, 10, 14)),        # Pd = 3 over D = 2: a depth plane absent at both ends; plane 5 x 3
    "p35": (24, 40, (3, 5), (12, 18)),               # plane 3 x 5
    "sq": (24, 24, (3, 3, 3), (2, 9, 12)),           # C == M, the residual block's geometry
    "w3": (24, 40, (3, 3, 3), (2, 9, 40)),           # the filter gradient: two tile columns of 32
    "w3d1": (24, 24, (3, 3, 3), (1, 9, 40)),         # D = 1 under Pd = 3: the banks kd = 0 and kd = 2 are empty
}
# the filter gradient at the length of the longest sums of a GPU cell (2 x 2 x 20 x 72 pixels per element): the bound still
# sees a missing k-step, halo element or tile there (the sparse tier's cells sum 16 x 40 x 70 pixels and it does not), but
# not a dropped lo.hi product
LONG = {"wlong": (16, 16, (3, 3, 3), (2, 20, 72))}


@functools.lru_cache(maxsize=None)
def _data(name, kind="random"):
    C, M, P, sp = {**SHAPES, **LONG}[name]
    if kind == "random":
        d = R.stage_inputs(N, C, M, P, sp, seed=5 + M + len(sp) + C)
        d["F"] = d["z"]
        return d
    d = R.exact_inputs(N, C, M, P, sp, 1, seed=6 + M + C, integer=kind == "integer")
    d["mask"], d["sub"] = (d["x2"] != 0).float(), d["x2"]
    return d


def _conv(transpose):
    return lambda a, b: R.conv(a, b, transpose)


def _wg(P):
    return lambda a, b: R.filter_grad(a, b, P, 1)


def _gated(t, gate):
    return t * (gate != 0)


def _rows(t, like):
    return t.reshape(t.shape + (1,) * (like.dim() - t.dim()))


def _epi(acc, alpha=1.0, mask=None, add=None, add_gate=None, sub=None, tau=None, relu=False, out_gate=None):
    """k_dense's epilogue in float32, one operation after the other (no fma)."""
    v = alpha * acc
    if mask is not None:
        v = v * mask
    if add is not None:
        v = v + (add if add_gate is None else _gated(add, add_gate))
    if sub is not None:
        v = v - sub
    if tau is not None:
        v = G._st32(v, _rows(tau, v))
    if relu:
        v = v.clamp_min(0.0)
    if out_gate is not None:
        v = torch.where(out_gate != 0, v, torch.zeros_like(v))
    return v


# honest fp32 versions of the three forms the mutants are measured on
def _h_analysis(d, x=None, w=None, kept=None, op=None, add_gate=True):
    acc = R.honest_product(op or _conv(False), d["x"] if x is None else x, d["w"] if w is None else w, "split3", kept)
    return _epi(acc, add=d["u"], add_gate=d["gate"] if add_gate else None)


def _m_analysis(d):
    return R.dense_form(d["x"], d["w"], add=d["u"], add_gate=d["gate"])


def _h_synth(d, z=None, w=None, kept=None, op=None):
    z = _gated(d["z"], d["gate"]) if z is None else z
    return _epi(R.honest_product(op or _conv(True), z, d["w"] if w is None else w, "split3", kept), mask=d["mask"], sub=d["sub"])


def _m_synth(d):
    return R.dense_form(d["z"], d["w"], True, in_gate=d["gate"], mask=d["mask"], sub=d["sub"])


def _h_wgrad(d, P, Fc=None, x=None, kept=None):
    return -1.0 * R.honest_product(_wg(P), d["F"] if Fc is None else Fc, d["x"] if x is None else x, "split3", kept)


def _m_wgrad(d, P):
    return R.wgrad_form(d["F"], d["x"], P, -1.0)


# ------------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize("M,P,sp", [(24, (5, 5), (20, 38)), (8, (3, 9, 5), (2, 12, 20)), (25, (3, 3), (11, 37))])
def test_at_one_channel_every_form_is_the_sparse_tiers_bit_for_bit(M, P, sp):
    d = G.stage_inputs(N, 1, M, P, sp, 1, seed=3 + M)
    same = lambda a, b: all(torch.equal(p, q) for p, q in zip(a, b))
    for alpha, zin, gate, tau in ((1.0, None, None, None), (1.0, None, None, d["tau"]), (-1.0, d["z"], None, d["tau"]),
                                  (1.0, d["u"], d["z"], None), (0.5, d["u"], None, None)):
        assert same(R.dense_form(d["x"], d["w"], alpha=alpha, add=zin, add_gate=gate, tau=tau, with_u=True),
                    G.analysis_form(d["x"], d["w"], 1, alpha, zin=zin, gate=gate, tau=tau, with_u=True))
    assert same(R.dense_form(d["x"], d["w"], alpha=0.5, add=d["u"], out_gate=d["z"]),
                G.analysis_form(d["x"], d["w"], 1, 0.5, zin=d["u"], zsup=d["z"]))
    for gate, mask, sub, alpha in ((None, None, None, 1.0), (d["gate"], None, None, -1.0), (None, d["mask"], None, 1.0),
                                   (d["gate"], None, d["sub"], 1.0), (None, d["mask"], d["sub"], -1.0)):
        assert same(R.dense_form(d["z"], d["w"], True, alpha, in_gate=gate, mask=mask, sub=sub), G.synth_form(d["z"], d["w"], 1, gate, mask, sub, alpha))
    assert same(R.wgrad_form(d["u"], d["x"], P, 0.5, gate=d["gate"]), G.wgrad_form(d["u"], d["x"], P, 1, 0.5, gate=d["gate"]))


@pytest.mark.parametrize("name", ["t353", "p35"])
def test_the_two_roles_and_the_filter_gradient_are_an_adjoint_triple(name):
    """<A x, z> = <x, B z> = <w, z (x) x> in float64 at a 3 x 5 x 3 and a 3 x 5 bank and its 5 x 3 transpose; the transposed role is
    the correlation with the bank flipped on every axis and its channel axes swapped."""
    C, M, P, sp = SHAPES[name]
    d = _data(name)
    for swap in (False, True):
        x, z, w = d["x"].double(), d["z"].double(), d["w"].double()
        if swap and len(P) == 2:                               # the 5 x 3 bank
            x, z, w, P = x.transpose(-1, -2), z.transpose(-1, -2), w.transpose(-1, -2), P[::-1]
        Ax, Bz, Gw = R.conv(x, w), R.conv(z, w, True), R.filter_grad(z, x, P, 1)
        assert Ax.shape == z.shape and Bz.shape == x.shape and Gw.shape == w.shape
        scale = float(Ax.abs().sum())
        assert abs(float((Ax * z).sum() - (x * Bz).sum())) < 1e-9 * scale
        assert abs(float((Ax * z).sum() - (w * Gw).sum())) < 1e-9 * scale
        flipped = torch.flip(w.transpose(0, 1), tuple(range(2, w.dim())))
        assert float((R.conv(z, flipped) - Bz).abs().max()) < 1e-10


def test_the_pool_the_diff_and_the_unpool_are_the_definitions():
    g = torch.Generator().manual_seed(4)
    h = torch.randn((2, 3, 7, 9), generator=g).double()
    pooled, codes = R.pool_first_max(h)
    ref, idx = F.max_pool2d(h, 2, 2, return_indices=True)       # floor mode; torch takes the first maximum too
    assert torch.equal(pooled, ref) and pooled.shape[-2:] == (3, 4)
    assert torch.equal(codes.long(), ((idx // 9) % 2) * 2 + (idx % 9) % 2)
    tied = torch.tensor([[1.0, 2.0, 0.0, 5.0], [2.0, 2.0, 5.0, 5.0]]).reshape(1, 1, 2, 4)
    assert R.pool_first_max(tied)[1].flatten().tolist() == [1, 1]
    placed = R.unpool_place(pooled, codes, 7, 9)
    assert torch.equal(placed, F.max_unpool2d(ref, idx, 2, 2, output_size=(7, 9)))
    assert float(placed[..., 6, :].abs().sum()) == 0 and float(placed[..., 8].abs().sum()) == 0
    fx, fy = torch.relu(h), torch.relu(h.flip(0))
    dd, sx, sy, s = R.vgg_diff(fx, fy)
    assert torch.equal(sx, (fx - fy) * (fx > 0)) and torch.equal(sy, (fx - fy) * (fy > 0)) and abs(s - float(((fx - fy) ** 2).sum())) < 1e-12
    assert torch.equal(torch.where(sx != 0, sx, sy), dd)        # d from the seeds alone, as the GPU test rebuilds it


# ------------------------------------------------------------------------------------------------ a correct implementation
@pytest.mark.parametrize("name", ["t353", "p35", "sq"])
def test_honest_fp32_implementation_is_inside_the_bound(name):
    C, M, P, sp = SHAPES[name]
    d = _data(name)
    acc = R.honest_product(_conv(False), d["x"], d["w"], "split3")
    syn = R.honest_product(_conv(True), d["z"], d["w"], "split3")
    syg = R.honest_product(_conv(True), _gated(d["z"], d["gate"]), d["w"], "split3")
    A = lambda **kw: R.dense_form(d["x"], d["w"], **kw)
    S = lambda **kw: R.dense_form(d["z"], d["w"], True, **kw)
    bias = 0.1 * d["tau"][0]
    forms = {
        "plain": (acc, A()),
        "first": (_epi(acc, tau=d["tau"]), A(tau=d["tau"])),
        "iter": (_epi(acc, -1.0, add=d["z"], tau=d["tau"]), A(alpha=-1.0, add=d["z"], tau=d["tau"])),
        "gated": (_h_analysis(d), _m_analysis(d)),
        "alpha": (_epi(acc, 0.75, add=d["u"]), A(alpha=0.75, add=d["u"])),
        "alpha fma": ((0.75 * acc.double() + d["u"].double()).float(), A(alpha=0.75, add=d["u"])),
        "rev": (_epi(acc, 0.5, add=d["u"], out_gate=d["z"]), A(alpha=0.5, add=d["u"], out_gate=d["z"])),
        "relu": (_epi(acc, relu=True), A(relu=True)),
        "bias": (_epi(acc, add=R._bias_like(bias, acc), relu=True), R.vgg_bias(d["x"], d["w"], bias)),
        "synth": (syn, S()),
        "synth gated": (_epi(syg, -1.0), S(alpha=-1.0, in_gate=d["gate"])),
        "synth mask": (_epi(syn, mask=d["mask"]), S(mask=d["mask"])),
        "synth sub": (_epi(syg, sub=d["sub"]), S(in_gate=d["gate"], sub=d["sub"])),
        "synth mask sub": (_h_synth(d), _m_synth(d)),
        "synth out_gate": (_epi(syn, out_gate=d["igate"]), S(out_gate=d["igate"])),
        "synth add": (_epi(syn, add=d["x2"]), S(add=d["x2"])),
        "wgrad": (_h_wgrad(d, P), _m_wgrad(d, P)),
        "wgrad gated": (0.5 * R.honest_product(_wg(P), _gated(d["u"], d["gate"]), d["x"], "split3"),
                        R.wgrad_form(d["u"], d["x"], P, 0.5, gate=d["gate"])),
    }
    if name == "sq":
        forms["relu add"] = (_epi(acc, add=d["x2"], relu=True), A(add=d["x2"], relu=True))
    if len(sp) == 2:                                           # the pooled forms are 2-D
        act = _epi(acc, add=R._bias_like(bias, acc), relu=True)
        pooled, codes = R.pool_first_max(act)
        val, b, _ = R.vgg_pool(d["x"], d["w"], bias)
        forms["pool"] = (pooled, (val, b))
        gp = d["u"][..., :sp[0] // 2, :sp[1] // 2].contiguous()
        og = d["igate"]
        placed = R.unpool_place(gp, codes, *sp)
        forms["unpool"] = (_epi(R.honest_product(_conv(True), placed, d["w"], "split3"), out_gate=og),
                           R.vgg_unpool(gp, codes, d["w"], *sp, out_gate=og))
    worst = {}
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
    print(f"{name}: worst |err|/b " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) < 0.5              # round-to-nearest adds err by at most 2^-24 each: half of what b allows


# ------------------------------------------------------------------------------------------------ the exact inputs
def _exact_forms(d, P):
    """{form: (model value, S_e)} of the forms the GPU cells compare for equality."""
    S_ana = R.abs_sum(_conv(False), d["x"], d["w"]) + d["u"].abs()
    S_syn = R.abs_sum(_conv(True), _gated(d["z"], d["gate"]), d["w"]) + d["sub"].abs()
    S_wg = R.abs_sum(_wg(P), d["F"], d["x"])
    return {"analysis": (_m_analysis(d)[0], S_ana), "synth": (_m_synth(d)[0], S_syn), "wgrad": (_m_wgrad(d, P)[0], S_wg)}


@pytest.mark.parametrize("kind", ["hilo", "integer"])
@pytest.mark.parametrize("name", ["t353", "p35", "w3"])
def test_exact_inputs_are_summable_and_fp32_reproduces_the_model_in_two_orders(name, kind):
    C, M, P, sp = SHAPES[name]
    d = _data(name, kind)
    q = d["quantum"]
    for k in ("x", "w", "z", "u", "F"):                        # the parts are what the recipe says
        hi, lo = R.parts(d[k])
        assert set(hi.unique().tolist()) <= ({0.0, 1.0, -1.0, 2.0, -2.0} if kind == "integer" else {0.0, 1.0, -1.0})
        assert set(lo.unique().tolist()) <= ({0.0} if kind == "integer" else {0.0, q, -q})
    assert bool(((d["F"] != 0).sum(1) == 1).all())             # every pixel is hit in exactly one channel
    forms = _exact_forms(d, P)
    for k, (val, S) in forms.items():
        assert R.exact_cap_ok(S, q), (k, float(S.max()) / q)
        assert bool((val / q == torch.round(val / q)).all())
    # order 1: torch's own; order 2: the summed axes (channels and taps, or pixels) permuted, by hand
    got1 = _h_analysis(d)
    col = R.im2col(d["x"], P, 1)                               # (N, C, T, Z)
    permk = torch.randperm(col.shape[1] * col.shape[2], generator=torch.Generator().manual_seed(2))
    colk = col.reshape(N, -1, col.shape[-1])[:, permk].contiguous()
    wk = d["w"].reshape(M, -1)[:, permk].contiguous()
    acc = None
    for (i, j) in R._KEPT["split3"]:
        t = R.parts(wk)[j].float() @ R.parts(colk)[i].float()
        acc = t if acc is None else acc + t
    got2 = acc.reshape(got1.shape) + _gated(d["u"], d["gate"])
    assert R.mismatches(got1, forms["analysis"][0]) == 0 and R.mismatches(got2, forms["analysis"][0]) == 0
    got1 = _h_synth(d)
    got2 = _h_synth(d, z=torch.flip(_gated(d["z"], d["gate"]), (1,)), w=torch.flip(d["w"], (0,)))
    assert R.mismatches(got1, forms["synth"][0]) == 0 and R.mismatches(got2, forms["synth"][0]) == 0
    got1 = _h_wgrad(d, P)
    Z = col.shape[-1]
    perm = torch.randperm(N * Z, generator=torch.Generator().manual_seed(1))
    Fm = d["F"].reshape(N, M, Z).transpose(0, 1).reshape(M, N * Z)[:, perm]
    cm = col.permute(0, 3, 1, 2).reshape(N * Z, -1)[perm]
    got2 = None
    for (i, j) in R._KEPT["split3"]:
        t = R.parts(Fm.contiguous())[i].float() @ R.parts(cm.contiguous())[j].float()
        got2 = t if got2 is None else got2 + t
    got2 = -got2.reshape(got1.shape)
    assert R.mismatches(got1, forms["wgrad"][0]) == 0 and R.mismatches(got2, forms["wgrad"][0]) == 0


@pytest.mark.parametrize("part", range(4))
def test_the_cap_holds_for_every_exact_input_of_the_gpu_cells(part):
    """The summability condition, on the model's own S_e, of every exact input test_gpu_dense_cells feeds a kernel (in four
    parts): the dense cells of both roles, the residual block's ReLU form, the filter-gradient cells at every width."""
    import test_gpu_dense_cells as D
    dense = D.exact_inputs_of_the_dense_cells()
    assert len(dense) == 2 * len(D.DENSE_CELLS) == 56
    for cid, variant in dense[part::4]:
        c, d = D.BY_ID[cid], D.exact_data(cid, variant)
        for k, (val, S) in D.exact_models(c, d).items():
            assert R.exact_cap_ok(S, d["quantum"]), (cid, variant, k, float(S.max()) / d["quantum"])
            assert bool((val / d["quantum"] == torch.round(val / d["quantum"])).all())
    wg = D.exact_inputs_of_the_wgrad_cells()
    assert len(wg) == 2 * (2 * len(D.WGRAD_CELLS) + 1)
    for cid, W, variant in wg[part::4]:
        e = D.wgrad_data(cid, W, variant)
        assert bool(((e["F"] != 0).sum(1) == 1).all()), cid
        pix = (e["F"] != 0).sum(dim=(0,) + tuple(range(2, e["F"].dim()))).max()
        assert float(pix) * R.exact_term_quanta(variant == "integer") < R.CAP_QUANTA, (cid, W, variant)
    if part == 0:
        for M in (24, 40):
            for variant in ("hilo", "integer"):
                e = D.residual_data(M, variant)
                assert R.exact_cap_ok(R.abs_sum(_conv(False), e["x"], e["w1"]), e["quantum"]), (M, variant)


def test_the_sign_mixed_thresholds_leave_out_under_one_percent_on_the_model():
    """test_gpu_dense_cells.SIGN_MIXED: with thresholds of both signs the shrinkage jumps at u = 0, so the cell compares where
    |u| > b only; on the model alone that leaves out less than 1 % of the elements."""
    import test_gpu_dense_cells as D
    for cell in D.SIGN_MIXED:
        d = D.cell_data(cell.id)
        assert bool((d["tau"] < 0).any()) and bool((d["tau"] > 0).any())
        for alpha, zin in ((1.0, None), (-1.0, d["z"])):
            _, b, u = R.dense_form(d["x"], d["w"], alpha=alpha, add=zin, tau=d["tau"], with_u=True)
            out = int((u.abs() <= b).sum())
            assert out <= 0.01 * u.numel(), (cell.id, out, u.numel())


# ------------------------------------------------------------------------------------------------ the filter-gradient plan
def test_the_filter_gradient_plan_gives_each_cell_its_property():
    import test_gpu_dense_cells as D
    seen = set()
    for c in D.WGRAD_CELLS + [D.NARROW_IMAGE]:
        for W in D.wgrad_widths(c):
            p = R.wgrad_plan(c.N, c.C, c.M, c.D, c.H, W, c.Pd)
            assert p is not None and p["ntiles"] >= 8 and p["vec"] == (W % 4 == 0), (c.id, W)
            seen.add(p["vec"])
            if c.why == "nwg == ntiles":
                assert p["nwg"] == p["ntiles"] and max(p["walked"]) == 1
            elif c.why == "ntiles > nwg":
                assert (p["ntiles"], p["nwg"]) == (60, 40) and max(p["walked"]) == 2
                # next_tile skips: some workgroup's first tile is depth-invalid for kd = 0
                assert p["valid"][0] < p["ntiles"] and p["valid"][1] == p["ntiles"]
            elif c.why == "empty kd":
                empty = [kd for kd in range(c.Pd) if p["valid"][kd] == 0]
                assert empty == ([0, 4] if c.Pd == 5 else [0, 2]), (c.id, p["valid"])
                if c.Pd == 5:
                    assert (p["ntiles"], p["nwg"]) == (36, 24) and max(p["walked"]) == 2
            elif c.why == "a single ragged tile column":
                assert p["tilesX"] == 1 and W < R.WTX and c.H % R.WTY
            else:                                              # the channel cells
                want = {"wg-C24M24": [True], "wg-C24M40": [False], "wg-C24M72": [False, True], "wg-C40M72": [False, False],
                        "wg-C64M64": [False]}[c.id]
                assert p["narrow"] == want, (c.id, p["narrow"])
                assert c.H % R.WTY and (W % R.WTX) and all(0 < v < p["ntiles"] for v in (p["valid"][0], p["valid"][2]))
    assert seen == {True, False}
    assert R.wgrad_plan(1, 24, 24, 1, 9, 40, 1) is None        # fewer than 8 tiles: the tier refuses
    assert R.wgrad_plan(2, 72, 72, 2, 9, 72, 3) is None        # C > 64


# ------------------------------------------------------------------------------------------------ mutations
# Each mutant returns (got, (model value, b)) on the data it is given; it is run on the seeded random data against b and on
# the exact inputs against equality.
def _flip_w(w, dims):
    return torch.flip(w.transpose(0, 1), dims).contiguous()


def _m_no_flip(d, P):
    """The transposed role as a correlation with the channel-swapped bank, not flipped."""
    return _h_synth(d, w=_flip_w(d["w"], ()), op=_conv(False)), _m_synth(d)


def _m_flip_plane_only(d, P):
    return _h_synth(d, w=_flip_w(d["w"], (3, 4)), op=_conv(False)), _m_synth(d)


def _m_plane_transposed(d, P):
    """The 5 x 3 plane's 15 values read as 3 rows of 5 (t353), the 3 x 5 plane's as 5 rows of 3 (p35)."""
    w = d["w"]
    return _h_synth(d, w=w.reshape(w.shape[:-2] + (P[-1], P[-2]))), _m_synth(d)


def _m_dropped_depth_plane(d, P):
    """The depth plane absent at the low end handled, the one at the high end read as if kd = Pd - 1 did not exist."""
    w = d["w"].clone()
    w[:, :, 0] = 0.0
    return _h_synth(d, w=w), _m_synth(d)


def _m_channel_leak_in(d, P):
    """A channel >= I of the ragged 16-chunk not zeroed: channel 0 and its filters once more."""
    return _h_analysis(d, x=torch.cat([d["x"], d["x"][:, :1]], 1), w=torch.cat([d["w"], d["w"][:, :1]], 1)), _m_analysis(d)


def _m_padded_channel_written(d, P):
    """Channel O of the padded tile (zero filters: the epilogue of a zero accumulator) written over channel O - 1."""
    got = _h_analysis(d)
    got[:, -1] = _gated(d["u"], d["gate"])[:, -1]
    return got, _m_analysis(d)


def _m_add_gate_ignored(d, P):
    return _h_analysis(d, add_gate=False), _m_analysis(d)


def _m_in_gate_on_output(d, P):
    """C == M: the gate multiplies the output of the ungated product."""
    on = d["gate"] != 0
    got = _epi(R.honest_product(_conv(True), d["z"], d["w"], "split3") * on, mask=d["mask"], sub=d["sub"])
    return got, _m_synth(d)


def _m_no_lo_hi_analysis(d, P):
    return _h_analysis(d, kept=((0, 0), (0, 1))), _m_analysis(d)


def _m_no_lo_hi_synth(d, P):
    return _h_synth(d, kept=((0, 0), (0, 1))), _m_synth(d)


def _m_no_lo_hi_wgrad(d, P):
    return _h_wgrad(d, P, kept=((0, 0), (0, 1))), _m_wgrad(d, P)


def _m_missing_k_step(d, P):
    """8 consecutive pixels of one row of one sample never multiplied."""
    Fc = d["F"].clone()
    Fc[1, :, 0, 3, 8:16] = 0.0
    return _h_wgrad(d, P, Fc=Fc), _m_wgrad(d, P)


def _m_missing_halo(d, P):
    """The halo element left of a tile row missing: the taps kj = 0 lose x[.., 31] at the pixels of column 32 only."""
    Fb, xb = torch.zeros_like(d["F"]), torch.zeros_like(d["x"])
    Fb[..., 32], xb[..., 31] = d["F"][..., 32], d["x"][..., 31]
    return _h_wgrad(d, P) - _h_wgrad(d, P, Fc=Fb, x=xb), _m_wgrad(d, P)


def _m_missing_second_tile(d, P):
    """One 4 x 32 tile of one (sample, depth) never accumulated."""
    Fc = d["F"].clone()
    Fc[1, :, 1, 4:8, 0:32] = 0.0
    return _h_wgrad(d, P, Fc=Fc), _m_wgrad(d, P)


def _m_empty_kd_not_zero(d, P):
    """D = 1 under Pd = 3: the bank of kd = 0, which no depth plane feeds, left holding the bank of kd = 1."""
    got = _h_wgrad(d, P)
    got[:, :, 0] = got[:, :, 1]
    return got, _m_wgrad(d, P)


# mutant: (function, shapes it applies to, what catches it: "both", or "exact" = ONLY the exact inputs do)
MUTANTS = {
    "transposed role: no flip": (_m_no_flip, ("t353", "p35"), "both"),
    "transposed role: flipped in the plane, not in depth": (_m_flip_plane_only, ("t353",), "both"),
    "transposed role: a 3 x 5 plane read as 5 x 3": (_m_plane_transposed, ("t353", "p35"), "both"),
    "transposed role: a dropped depth plane at one end only": (_m_dropped_depth_plane, ("t353",), "both"),
    "a channel >= I of a ragged 16-chunk leaking in": (_m_channel_leak_in, ("t353", "p35"), "both"),
    "a channel >= O of the padded tile written over channel O - 1": (_m_padded_channel_written, ("t353", "p35"), "both"),
    "add_gate ignored": (_m_add_gate_ignored, ("t353", "p35"), "both"),
    "in_gate applied to the output": (_m_in_gate_on_output, ("sq",), "both"),
    "split3 without lo.hi (analysis role)": (_m_no_lo_hi_analysis, ("t353", "p35"), "both"),
    "split3 without lo.hi (transposed role)": (_m_no_lo_hi_synth, ("t353", "p35"), "both"),
    "split3 without lo.hi (filter gradient)": (_m_no_lo_hi_wgrad, ("wlong",), "exact"),
    "filter gradient: one 8-pixel k-step missing": (_m_missing_k_step, ("wlong",), "both"),
    "filter gradient: the halo element of one side missing": (_m_missing_halo, ("wlong",), "both"),
    "filter gradient: the second tile of a workgroup missing": (_m_missing_second_tile, ("wlong",), "both"),
    "filter gradient: a kd bank not zero where no depth plane is valid": (_m_empty_kd_not_zero, ("w3d1",), "both"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_leaves_the_bound_or_the_exact_predicate(mutant):
    """Every mutant is run on the seeded random data against the bound and on the exact inputs against equality.  "both": each
    instrument catches it; "exact": the bound, loose by the length of the sum, lets it through and ONLY the exact inputs
    catch it."""
    fn, names, caught_by = MUTANTS[mutant]
    for name in names:
        C, M, P, sp = {**SHAPES, **LONG}[name]
        got, (val, b) = fn(_data(name), P)
        bad, worst = R.violations_fp32(got, val, b)
        got_e, (val_e, _) = fn(_data(name, "hilo"), P)
        off = R.mismatches(got_e, val_e)
        print(f"{mutant} [{name}]: {bad} outside b (worst {worst:.3g}), {off} exact mismatches")
        assert off > 0, (mutant, name)
        assert (bad > 0) == (caught_by == "both"), (mutant, name, bad, worst)


# the pool and the unpool are compared through their codes and their values: mutants of the two
def _pool_last_max(h):
    v, (Hp, Wp) = h, (h.shape[-2] // 2, h.shape[-1] // 2)
    w = v[..., :2 * Hp, :2 * Wp].reshape(v.shape[:-2] + (Hp, 2, Wp, 2)).transpose(-3, -2).reshape(v.shape[:-2] + (Hp, Wp, 4))
    mx = w.max(-1).values
    return mx, (3 - (w.flip(-1) == mx[..., None]).to(torch.uint8).argmax(-1)).to(torch.uint8)


def _pool_swapped_bits(h):
    mx, code = R.pool_first_max(h.transpose(-1, -2))           # the window walked column-major: (xx & 1) << 1 | (yy & 1)
    return mx.transpose(-1, -2), code.transpose(-1, -2)


def _pool_ceil(h):
    return R.pool_first_max(F.pad(h, (0, h.shape[-1] % 2, 0, h.shape[-2] % 2), value=float("-inf")))


POOL_MUTANTS = {"pool: the last maximum instead of the first": (_pool_last_max, "both"),
                "pool: the code's bit order swapped": (_pool_swapped_bits, "both"),
                "pool: ceil instead of floor at an odd extent": (_pool_ceil, "both")}


def _pool_inputs(kind):
    """relu(conv + bias) at an odd 11 x 13 plane: seeded random values (no ties), or exact inputs (integers: many ties)."""
    C, M, P, sp = 16, 24, (3, 3), (11, 13)
    if kind == "random":
        d = R.stage_inputs(N, C, M, P, sp, seed=9)
        bias = 0.1 * d["tau"][0]
    else:
        d = R.exact_inputs(N, C, M, P, sp, 1, seed=10, integer=True, only=("x", "w"))
        bias = torch.ones(M)
    acc = R.honest_product(_conv(False), d["x"], d["w"], "split3")
    return d, bias, _epi(acc, add=R._bias_like(bias, acc), relu=True)


@pytest.mark.parametrize("mutant", list(POOL_MUTANTS))
def test_pool_mutant_is_caught_by_the_values_or_the_codes(mutant):
    """The pooled values against b (or equality) and the codes against the first-maximum codes of the same values.  On seeded
    random data the only tied windows are those the ReLU zeroed altogether (enough to tell the last maximum from the first);
    the exact (integer) inputs tie at positive values too, which is asserted."""
    fn, caught_by = POOL_MUTANTS[mutant]
    for kind in ("random", "exact"):
        d, bias, act = _pool_inputs(kind)
        val, b, _ = R.vgg_pool(d["x"], d["w"], bias)
        want, codes = R.pool_first_max(act)
        assert R.violations_fp32(want, val, b)[0] == 0
        got, gcodes = fn(act)
        caught = got.shape != want.shape or R.violations_fp32(got, val, b)[0] > 0 or int((gcodes != codes).sum()) > 0
        if kind == "exact":
            ties = int((((act[..., :10, :12].reshape(N, 24, 5, 2, 6, 2) == want[:, :, :, None, :, None]).sum(dim=(3, 5)) > 1) & (want > 0)).sum())
            assert ties > 0 and caught, (mutant, ties)
        else:
            assert caught == (caught_by == "both"), (mutant, kind)


def test_unpool_writing_into_the_dropped_row_is_caught():
    for kind in ("random", "exact"):
        d, bias, act = _pool_inputs(kind)
        _, codes = R.pool_first_max(act)
        gp = R.pool_first_max(act)[0]                           # a pooled gradient: the pooled values themselves
        val, b = R.vgg_unpool(gp, codes, d["w"], 11, 13)
        placed = R.unpool_place(gp, codes, 11, 13)
        assert R.violations_fp32(R.honest_product(_conv(True), placed, d["w"], "split3"), val, b)[0] == 0
        wrong = placed.clone()
        wrong[..., 10, 0:12:2] = gp[..., -1, :]                 # the dropped eleventh row written
        got = R.honest_product(_conv(True), wrong, d["w"], "split3")
        assert R.violations_fp32(got, val, b)[0] > 0 and R.mismatches(got, val) > 0, kind
