"""Every instance the step-wise entry points of the fused 2-D tier can launch -- arithmetic x layout pair x mode x M, with
and without the dA_k ride -- against the float64 model of its arithmetic (fused2d_arith_restate.py):
|got - model| <= b at every element, exact zeros off the support, the written map that of the output, every output bit
for bit the same in a second call.  Geometry of test_gpu_stage_tile_phase.py: N = 2, 40 x 150, masked, 18 tiles, ragged in
both axes, padding pixels in the blocked layouts; at the default grid (one tile per workgroup) and under CDL_FUSED_GRID=4
(5, 5, 4, 4 tiles: the next tile's thin inputs are loaded across an image boundary and past the last tile).  The same cells on
exactly-summable inputs, where the outputs must EQUAL the model: the second half of the file."""
import functools

import pytest
import torch

import fused2d_arith_restate as R
from gpu_util import launch_sites, log

pytestmark = pytest.mark.gpu

N, H, W = 2, 40, 150
NC, BL, B16 = "nchw", "blocked", "blocked_bf16"
LAYS = (NC, BL, B16)
ALL_PAIRS = [(a, b) for a in LAYS for b in LAYS]
# the dispatcher's table (launch_stage_lay / launch_stage_one, 64 x 16 tiles)
PAIRS = {
    "first": [(NC, NC), (BL, BL), (B16, B16)],
    "fwd": [(NC, NC), (BL, BL), (B16, B16), (BL, NC), (B16, NC)],
    "bwd": [(NC, NC), (BL, BL), (B16, B16), (NC, BL), (BL, NC), (NC, B16)],
    "ride": [(NC, NC), (BL, BL), (B16, B16), (NC, BL), (NC, B16)],
}
MODE_ID = {"fwd": 0, "first": 1, "bwd": 2, "ride": 2}
LAY_ID = {NC: 0, BL: 1, B16: 2}
ROWS = [(M, P, prec) for (M, P) in ((64, 7), (32, 5)) for prec in R.PRECISIONS] + [(64, 3, "split3")]
STAGE = "cdl_fused2d.hip:k_stage<"


@functools.lru_cache(maxsize=None)
def _data(M, P):
    return R.stage_inputs(N, M, P, H, W, seed=5 + M + P)


@functools.lru_cache(maxsize=None)
def _dev(M, P):
    return {k: v.cuda() for k, v in _data(M, P).items()}


def _as_stored(x, blk16):
    """An fp32 code tensor as a buffer of the layout holds it."""
    return x.bfloat16().float() if blk16 else x


@functools.lru_cache(maxsize=None)
def _model(mode, M, P, prec, blk16_in):
    """(value, b) of the analysis half, once per (mode, M, P, arithmetic, rounding of the fat input)."""
    d = _data(M, P)
    if mode == "first":
        return R.forward_stage(d["r"], d["wA"], d["tau"], None, 1.0, prec)
    if mode == "fwd":
        return R.forward_stage(d["r"], d["wA"], d["tau"], _as_stored(d["zin"], blk16_in), -1.0, prec)
    return R.reverse_stage(d["thin"], d["wA"], d["gate"] != 0, _as_stored(d["base"], blk16_in), prec)


def _geom(o, M, P):
    g = o.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1)
    assert o.fused_supported(g) and o.fused_tiles(g) == 18
    return g


def _fresh(o, g, lay):
    """An output code buffer of `lay` with a recognisable fill (padding pixels of a blocked buffer are never written)."""
    return o.fused_code_buffer(g, lay, "cuda")[0].fill_(-7.0)


def _pad_untouched(g, buf, lay):
    if lay == NC or W % 32 == 0:
        return True
    v = buf.reshape(g.N, H, (W + 31) // 32, g.M // 4, 32, 4)[:, :, -1, :, W % 32:, :]
    return bool((v.float() == -7.0).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _run_cell(o, g, mode, lin, lout, prec, d, frags):
    """One launch of the cell [and its assemble / reductions]: dict of outputs (device tensors) and the trace."""
    M = g.M
    patches = o.fused_patches(g, "cuda").fill_(float("nan"))
    out = _fresh(o, g, lout)
    res = {}
    with o.trace() as t:
        if mode in ("first", "fwd"):
            bits = torch.full((N, 4, H, W), -1, dtype=torch.int32, device="cuda")
            zin = None if mode == "first" else o.fused_from_nchw(g, d["zin"], lin)
            o.fused_iter(g, d["r"], zin, d["tau"], frags, 1.0 if mode == "first" else -1.0, patches, prec, out=out,
                         map_out=bits, lay_in=lin, lay_out=lout)
            res["map"] = bits
            res["thin"] = o.fused_assemble(g, patches, d["mask"], d["sub"], 1.0)
        else:
            dtp = torch.full((o.fused_tiles(g), M), float("nan"), device="cuda")
            rider = dict(r2=d["r2"], alpha=-1.0, workspace=o.fused_wgrad_workspace(g, "cuda")) if mode == "ride" else {}
            got = o.fused_stage_bwd(g, d["thin"], o.fused_from_nchw(g, d["base"], lin), d["bits"], frags, patches, dtp, True,
                                    prec, out=out, lay_in=lin, lay_out=lout, **rider)
            if mode == "ride":
                res["dA"] = got[1]
            res["dtp"] = dtp
            res["dt"] = torch.zeros(2, M, device="cuda")
            o.fused_dtau_reduce(g, dtp, d["c"], res["dt"])
            res["thin"] = o.fused_assemble(g, patches, d["mask"], None, -1.0)
        torch.cuda.synchronize()
    res["code"], res["patches"] = out, patches
    return res, t


@pytest.mark.parametrize("grid", ["gdef", "g4"])
@pytest.mark.parametrize("M,P,prec", ROWS)
@pytest.mark.parametrize("mode", ["first", "fwd", "bwd", "ride"])
def test_cell_against_the_float64_model(mode, M, P, prec, grid, hip_env):
    import cdlnet_video_amd as cva
    o = cva.ops
    if grid == "g4":
        hip_env("CDL_FUSED_GRID", "4")
    g = _geom(o, M, P)
    d, dc = _dev(M, P), _data(M, P)
    if "bits" not in d:
        d["bits"] = o.fused_support_map(g, d["gate"])
    frags = o.fused_prep(d["wA"], d["wB"])
    on, neg = dc["gate"] != 0, dc["gate"] < 0
    failures = []
    for (lin, lout) in PAIRS[mode]:
        tag = f"cell {mode} M{M}P{P} {prec} {lin}->{lout} {grid}"
        res, t = _run_cell(o, g, mode, lin, lout, prec, d, frags)
        # -- the instance asked for
        sites = launch_sites(t)
        keys = [k for k in sites if k.startswith(STAGE)]
        assert len(keys) == 1 and len(sites[keys[0]]) == 1, sites.keys()
        tpl = sites[keys[0]][0].template()
        want = dict(WY=2, MT=M // 32, PREC=o.PRECISION[prec], MODE=MODE_ID[mode], LIN=LAY_ID[lout if mode == "first" else lin],
                    LOUT=LAY_ID[lout])
        assert {k: tpl[k] for k in want} == want and keys[0].split(",")[-2] == ("true" if mode == "ride" else "false"), (tpl, keys)
        # -- a second identical call: bit for bit, patches and partial sums included
        res2, _ = _run_cell(o, g, mode, lin, lout, prec, d, frags)
        differ = [k for k in res if not _same([res[k]], [res2[k]])]
        assert _pad_untouched(g, res["code"], lout), tag
        # -- analysis half against the model
        val, b = _model("bwd" if mode == "ride" else mode, M, P, prec, lin == B16 and mode != "first")
        code = o.fused_to_nchw(g, res["code"], lout).cpu()
        bad, worst = (R.violations_bf16 if lout == B16 else R.violations_fp32)(code, val, b)
        ratios = {"code": worst}
        counts = {"code": bad}
        if mode in ("first", "fwd"):
            assert torch.equal(res["map"], o.fused_support_map(g, code.cuda())), f"{tag}: support / sign map"
            thin_model = R.synth_assemble(code, dc["wB"], prec, lout == B16, dc["mask"], dc["sub"], 1.0)
        else:
            counts["off-support"] = R.zeros_off_support(code, on)
            thin_model = R.synth_assemble(code, dc["wB"], prec, lout == B16, dc["mask"], None, -1.0)
            counts["dt"], ratios["dt"] = R.violations_fp32(res["dt"].cpu(), *R.dtau_sums(code, on, neg, dc["c"]))
            if mode == "ride":
                counts["dA"], ratios["dA"] = R.violations_fp32(res["dA"].cpu(), *R.wgrad(code, dc["r2"], -1.0, P, prec, lout == B16))
        # -- synthesis half: the model is fed the device's own z' / du
        counts["thin"], ratios["thin"] = R.violations_fp32(res["thin"].cpu(), *thin_model)
        log(f"{tag:64s} {tpl} worst|err|/b " + " ".join(f"{k}={v:.2e}" for k, v in ratios.items())
            + f" violations={counts} not-reproduced={differ}")
        if differ or any(counts.values()):
            failures.append((tag, counts, differ, ratios))
    assert not failures, failures


@pytest.mark.parametrize("mode", ["fwd", "bwd", "ride"])
def test_pairs_outside_the_table_are_refused(mode):
    import cdlnet_video_amd as cva
    o = cva.ops
    M, P = 32, 5
    g = _geom(o, M, P)
    d = _dev(M, P)
    if "bits" not in d:
        d["bits"] = o.fused_support_map(g, d["gate"])
    frags = o.fused_prep(d["wA"], d["wB"])
    refused = [p for p in ALL_PAIRS if p not in PAIRS[mode]]
    assert len(refused) == 9 - len(PAIRS[mode])
    for prec in R.PRECISIONS:
        for (lin, lout) in refused:
            with pytest.raises(cva._lib.HipKernelError, match="CDL_EUNSUPPORTED"):
                _run_cell(o, g, mode, lin, lout, prec, d, frags)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ k_wgrad2d
@functools.lru_cache(maxsize=None)
def _wgrad_model(M, P, prec, blk16, which):
    d = _data(M, P)
    X, T, al = ((d["gate"], d["r2"], -1.0), (d["base"], d["thin"], 1.0))[which]
    return R.wgrad(_as_stored(X, blk16), T, al, P, prec, blk16)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("M,P,prec", ROWS)
def test_filter_gradient_against_the_float64_model(M, P, prec, lay):
    import cdlnet_video_amd as cva
    o = cva.ops
    g = _geom(o, M, P)
    d = _dev(M, P)
    ws = o.fused_wgrad_workspace(g, "cuda")
    X0, X1 = o.fused_from_nchw(g, d["gate"], lay), o.fused_from_nchw(g, d["base"], lay)
    with o.trace() as t:
        pair = o.fused_wgrad(g, ws, X0, d["r2"], -1.0, X1, d["thin"], 1.0, precision=prec, layout=lay)
        single = o.fused_wgrad(g, ws, X1, d["thin"], 1.0, precision=prec, layout=lay, tiles_reversed=True)
        torch.cuda.synchronize()
    recs = [r for k, v in launch_sites(t).items() if k.startswith("cdl_fused2d.hip:k_wgrad2d<") for r in v]
    assert len(recs) == 2
    for r in recs:
        tpl = r.template()
        assert (tpl["MT"], tpl["PREC"], tpl["LAY"]) == (M // 32, o.PRECISION[prec], LAY_ID[lay]), tpl
    assert single[1] is None
    again = o.fused_wgrad(g, ws, X0, d["r2"], -1.0, X1, d["thin"], 1.0, precision=prec, layout=lay)
    assert _same(pair, again)
    counts, ratios = {}, {}
    for name, got, which in (("pair0", pair[0], 0), ("pair1", pair[1], 1), ("single", single[0], 1)):
        counts[name], ratios[name] = R.violations_fp32(got.cpu(), *_wgrad_model(M, P, prec, lay == B16, which))
    log(f"cell wgrad M{M}P{P} {prec} {lay}".ljust(64) + f" {tpl} worst|err|/b "
        + " ".join(f"{k}={v:.2e}" for k, v in ratios.items()))
    assert not any(counts.values()), (counts, ratios)


# ------------------------------------------------------------------------------------------------ the lo . lo products
@pytest.mark.parametrize("mode", ["first", "fwd", "bwd"])
@pytest.mark.parametrize("M,P", [(64, 7), (32, 5)])
def test_crafted_inputs_show_the_lo_lo_products_of_split4(M, P, mode):
    """On the crafted inputs (fused2d_arith_restate.crafted_split4_inputs) the four-product arithmetic passes the split4 model
    and fails the split3 model at every non-zero element; the three-product arithmetic the other way round."""
    import cdlnet_video_amd as cva
    o = cva.ops
    g = _geom(o, M, P)
    r, w = R.crafted_split4_inputs(N, M, P, H, W, seed=40 + M)
    frags = o.fused_prep(w.cuda(), _dev(M, P)["wB"])
    patches = o.fused_patches(g, "cuda")
    tau = torch.zeros(N, M)
    ones = torch.ones(N, M, H, W)
    model = {}
    for prec in ("split3", "split4"):
        if mode == "bwd":
            model[prec] = R.reverse_stage(r, w, ones.bool(), None, prec)
        else:
            model[prec] = R.forward_stage(r, w, tau, None if mode == "first" else 0 * ones, 1.0 if mode == "first" else -1.0, prec)
    nz = int((model["split4"][0] != 0).sum())
    assert nz > 0.9 * N * M * (H - P) * (W - P)
    for prec, other in (("split4", "split3"), ("split3", "split4")):
        if mode == "bwd":
            got = o.fused_stage_bwd(g, r.cuda(), None, o.fused_support_map(g, ones.cuda()), frags, patches,
                                    torch.empty(o.fused_tiles(g), M, device="cuda"), True, prec)
        else:
            got = o.fused_iter(g, r.cuda(), None if mode == "first" else (0 * ones).cuda(), tau.cuda(), frags,
                               1.0 if mode == "first" else -1.0, patches, prec)
        own, worst = R.violations_fp32(got.cpu(), *model[prec])
        impostor, _ = R.violations_fp32(got.cpu(), *model[other])
        log(f"cell crafted {mode} M{M}P{P} {prec}".ljust(64) + f" worst|err|/b={worst:.2e} violations of the {other} model: "
            f"{impostor} of {nz}")
        assert own == 0 and impostor == nz, (prec, own, impostor, nz)


# ------------------------------------------------------------------------------------------------ the forward sweep
@functools.lru_cache(maxsize=None)
def _sweep_data(M, P, K):
    gen = torch.Generator().manual_seed(17 + M)
    rnd = lambda *s: torch.randn(s, generator=gen)
    return dict(yp=rnd(N, 1, H, W), A=[0.1 * rnd(M, 1, P, P) for _ in range(K)], B=[0.1 * rnd(M, 1, P, P) for _ in range(K)],
                tau=0.3 * torch.rand(K, N, M, generator=gen), mask=(torch.rand(N, 1, H, W, generator=gen) < 0.5).float())


@pytest.mark.parametrize("M,P", [(64, 7), (32, 5)])
@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("lay", LAYS)
def test_forward_sweep_launch_by_launch_against_the_float64_model(lay, prec, M, P, hip_env):
    """cdl_fused2d_forward (K = 3, every code and residual kept) teacher-forced: each launch's own inputs (z_k, r_k) as the
    device produced them go to the model, the predicate is applied to its z_{k+1} and r_{k+1}.  With bf16 code storage these
    are the 64 x 32-tile kernels (WY = 4), which no step-wise entry point reaches."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    K = 3
    hip_env("CDL_FUSED_GRID", "4")
    g = _geom(o, M, P)
    dc = _sweep_data(M, P, K)
    A, B = [w.cuda() for w in dc["A"]], [w.cuda() for w in dc["B"]]
    with loop.precision_scope(prec), o.trace() as t:
        xp, zK, codes, resid, maps = loop._forward_fused(g, dc["yp"].cuda(), dc["mask"].cuda(), dc["tau"].cuda(), A, B, True, True,
                                                         layout=lay)
        torch.cuda.synchronize()
    stages = [r.template() for sid, recs in launch_sites(t).items() if sid.startswith(STAGE) for r in recs]
    WY = 4 if lay == B16 else 2
    want = [(WY, M // 32, o.PRECISION[prec], 1 if k == 0 else 0, LAY_ID[lay], LAY_ID[lay if k < K - 1 else NC]) for k in range(K)]
    assert [(tp["WY"], tp["MT"], tp["PREC"], tp["MODE"], tp["LIN"], tp["LOUT"]) for tp in stages] == want, stages
    assert len(codes) == K and len(resid) == K - 1 and len(maps) == K
    r_in, z_in = dc["yp"], None
    counts, ratios = {}, {}
    for k in range(K):
        lout = lay if k < K - 1 else NC
        val, b = R.forward_stage(r_in, dc["A"][k], dc["tau"][k], z_in, 1.0 if k == 0 else -1.0, prec)
        z_out = o.fused_to_nchw(g, codes[k], lout).cpu()
        counts[f"z{k + 1}"], ratios[f"z{k + 1}"] = (R.violations_bf16 if lout == B16 else R.violations_fp32)(z_out, val, b)
        assert torch.equal(maps[k], o.fused_support_map(g, z_out.cuda())), f"map of launch {k}"
        if k < K - 1:
            thin, model = resid[k].cpu(), R.synth_assemble(z_out, dc["B"][k + 1], prec, lout == B16, dc["mask"], dc["yp"], 1.0)
        else:
            thin, model = xp.cpu(), R.synth_assemble(z_out, dc["B"][0], prec)
        counts[f"r{k + 1}"], ratios[f"r{k + 1}"] = R.violations_fp32(thin, *model)
        r_in, z_in = thin, z_out
    assert torch.equal(zK, codes[-1])
    log(f"cell forward-sweep M{M}P{P} {prec} {lay} g4".ljust(64) + f" (WY, MT, PREC, MODE, LIN, LOUT)={want} worst|err|/b "
        + " ".join(f"{k}={v:.2e}" for k, v in ratios.items()))
    assert not any(counts.values()), (counts, ratios)


# ------------------------------------------------------------------------------------------------ exactly-summable inputs
# operands on which every partial sum in every order is an fp32 number (the cap is asserted on the CPU,
# test_fused2d_arith_cpu.py, for every input enumerated by exact_inputs_of_this_file), so the device must EQUAL the model at
# every element.  Three recipes per cell (fused2d_arith_restate.RECIPES); EXACT_HELD names the outputs a recipe holds to
# equality, the others stay with the bound.
EXACT_G4 = [(64, 7, "split3"), (64, 7, "bf16")]               # CDL_FUSED_GRID=4: the thin prefetch across an image boundary
EXACT_CASES = [(mode, M, P, prec, recipe, grid)
               for grid, rows in (("gdef", ROWS), ("g4", EXACT_G4)) for (M, P, prec) in rows
               for mode in ("first", "fwd", "bwd", "ride") for recipe in R.RECIPES]


@functools.lru_cache(maxsize=4)
def _exact_operands(recipe, M, P, no_bank_lo, first):
    return R.exact_stage_inputs(recipe, "split4" if no_bank_lo else "split3", N, M, P, H, W, seed=31 + M + P, first=first)


_EXACT_SECONDS = [0.0]                                        # the time the exact cases of this file have added, for the parity log


def _added(t0):
    import time
    _EXACT_SECONDS[0] += time.perf_counter() - t0
    return f"{time.perf_counter() - t0:.2f} s (exact cases of this file so far: {_EXACT_SECONDS[0]:.1f} s)"


def exact_data(mode, M, P, prec, recipe):
    """The operands of an exact case; they depend on the arithmetic only through split4's rule (no lo part in the banks) and
    on the mode only through the pass-through bank of a first stage."""
    return _exact_operands(recipe, M, P, prec == "split4" and recipe != "int", mode == "first" and recipe == "hilo-p")


@functools.lru_cache(maxsize=8)
def exact_model(mode, M, P, prec, recipe, blk16_in, blk16_out):
    """{output: (value, S_e, quantum)} of an exact case, once per rounding of the fat input and output."""
    return R.exact_stage_model("bwd" if mode == "ride" else mode, exact_data(mode, M, P, prec, recipe), prec, blk16_in, blk16_out,
                               ride=mode == "ride", wgrad_P=P)


@functools.lru_cache(maxsize=2)
def exact_wgrad_data(M, P, prec, variant):
    """k_wgrad2d's operands: F, F2 with one non-zero channel per code pixel (generic_arith_restate.exact_inputs), x, x2 the thin
    operands -- without lo parts under split4."""
    import generic_arith_restate as G
    d = G.exact_inputs(N, 1, M, (P, P), (H, W), 1, seed=57 + M + P, integer=variant == "integer", only=("x", "x2", "F", "F2"))
    if prec == "split4":
        d["x"], d["x2"] = R.hi_only(d["x"]), R.hi_only(d["x2"])
    return d


def exact_wgrad_model(M, P, prec, variant, blk16):
    d = exact_wgrad_data(M, P, prec, variant)
    return [R.exact_wgrad_model(d["F"], d["x2"], -1.0, P, prec, blk16), R.exact_wgrad_model(d["F2"], d["x"], 1.0, P, prec, blk16)]


def exact_inputs_of_this_file():
    """Every exact input a test below feeds a kernel, with the model that is compared: ("stage", mode, M, P, prec, recipe,
    blk16_in, blk16_out) and ("wgrad", M, P, prec, variant, blk16).  The grid does not change the operands."""
    out = set()
    for (mode, M, P, prec, recipe, _) in EXACT_CASES:
        for (lin, lout) in PAIRS[mode]:
            out.add(("stage", mode, M, P, prec, recipe, lin == B16 and mode != "first", lout == B16))
    for (M, P, prec) in ROWS:
        for variant in ("hilo", "integer"):
            for blk16 in (False, True):
                out.add(("wgrad", M, P, prec, variant, blk16))
    return sorted(out)


def _pin_stage(o, t, mode, M, prec, lin, lout):
    """The one k_stage launch of the trace, with the template arguments asked for."""
    sites = launch_sites(t)
    keys = [k for k in sites if k.startswith(STAGE)]
    assert len(keys) == 1 and len(sites[keys[0]]) == 1, sites.keys()
    tpl = sites[keys[0]][0].template()
    want = dict(WY=2, MT=M // 32, PREC=o.PRECISION[prec], MODE=MODE_ID[mode], LIN=LAY_ID[lout if mode == "first" else lin],
                LOUT=LAY_ID[lout])
    assert {k: tpl[k] for k in want} == want and keys[0].split(",")[-2] == ("true" if mode == "ride" else "false"), (tpl, keys)
    return tpl


@pytest.mark.parametrize("mode,M,P,prec,recipe,grid", EXACT_CASES)
def test_exact_inputs_hold_the_stage_to_equality(mode, M, P, prec, recipe, grid, hip_env):
    """Every (mode, layout pair) of PAIRS on exactly-summable operands: the outputs the recipe holds (EXACT_HELD) equal the
    model in value at every element, a bf16-stored code equals bf16_rne(model), the written map is that of the code; the outputs
    it does not hold stay inside the bound of the model fed the device's own z' / du."""
    import time
    import generic_arith_restate as G
    import cdlnet_video_amd as cva
    o = cva.ops
    t0 = time.perf_counter()
    if grid == "g4":
        hip_env("CDL_FUSED_GRID", "4")
    g = _geom(o, M, P)
    e = exact_data(mode, M, P, prec, recipe)
    ev = {k: v.cuda() for k, v in e.items() if torch.is_tensor(v)}
    ev["bits"] = o.fused_support_map(g, ev["gate"])
    frags = o.fused_prep(ev["wA"], ev["wB"])
    on, neg = e["gate"] != 0, e["gate"] < 0
    held = R.EXACT_HELD[recipe]
    failures = []
    for (lin, lout) in PAIRS[mode]:
        tag = f"cell exact {recipe} {mode} M{M}P{P} {prec} {lin}->{lout} {grid}"
        res, t = _run_cell(o, g, mode, lin, lout, prec, ev, frags)
        tpl = _pin_stage(o, t, mode, M, prec, lin, lout)
        assert _pad_untouched(g, res["code"], lout), tag
        model = exact_model(mode, M, P, prec, recipe, lin == B16 and mode != "first", lout == B16)
        code = o.fused_to_nchw(g, res["code"], lout).cpu()
        counts, quanta = {}, {}
        for name in ("code", "thin", "dt", "dA"):
            if name in model and name in held:
                val, S, q = model[name]
                counts[name], _ = R.violations_exact(code if name == "code" else res[name].cpu(), val, q)
                quanta[name] = R.cap_quanta(S, q)
                assert quanta[name] < G.CAP_QUANTA, (tag, name)
        fwd = mode in ("first", "fwd")
        if fwd:
            # the written map is that of the output, which equals the model (the sign bit of a zero is not the model's to say)
            counts["map"] = int((res["map"] != o.fused_support_map(g, code.cuda())).sum())
        else:
            counts["off-support"] = R.zeros_off_support(code, on)
        if "thin" not in held:                                # the synthesis half of the analysis recipe: the bound, as today
            counts["thin<=b"], _ = R.violations_fp32(res["thin"].cpu(), *R.synth_assemble(
                code, e["wB"], prec, lout == B16, e["mask"], e["sub"] if fwd else None, 1.0 if fwd else -1.0))
            if not fwd:
                counts["dt<=b"], _ = R.violations_fp32(res["dt"].cpu(), *R.dtau_sums(code, on, neg, e["c"]))
            if mode == "ride":
                counts["dA<=b"], _ = R.violations_fp32(res["dA"].cpu(), *R.wgrad(code, e["r2"], -1.0, P, prec, lout == B16))
        log(f"{tag:72s} {tpl} violations={counts} largest S_e in quanta "
            + " ".join(f"{k}={v:.0f}" for k, v in quanta.items()) + f" cap={G.CAP_QUANTA:.0f}")
        if any(counts.values()):
            failures.append((tag, counts))
    log(f"cell exact {recipe} {mode} M{M}P{P} {prec} {grid}: {len(PAIRS[mode])} pairs in {_added(t0)}")
    assert not failures, failures


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("M,P,prec", ROWS)
def test_exact_inputs_hold_the_filter_gradient_to_equality(M, P, prec, lay):
    """k_wgrad2d, pair and single, on the one-channel-per-pixel code operands: equality at every filter tap."""
    import time
    import generic_arith_restate as G
    import cdlnet_video_amd as cva
    o = cva.ops
    t0 = time.perf_counter()
    g = _geom(o, M, P)
    ws = o.fused_wgrad_workspace(g, "cuda")
    for variant in ("hilo", "integer"):
        d = exact_wgrad_data(M, P, prec, variant)
        dv = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
        X0, X1 = o.fused_from_nchw(g, dv["F"], lay), o.fused_from_nchw(g, dv["F2"], lay)
        with o.trace() as t:
            pair = o.fused_wgrad(g, ws, X0, dv["x2"], -1.0, X1, dv["x"], 1.0, precision=prec, layout=lay)
            single = o.fused_wgrad(g, ws, X1, dv["x"], 1.0, precision=prec, layout=lay, tiles_reversed=True)
            torch.cuda.synchronize()
        recs = [r for k, v in launch_sites(t).items() if k.startswith("cdl_fused2d.hip:k_wgrad2d<") for r in v]
        assert len(recs) == 2
        for r in recs:
            tpl = r.template()
            assert (tpl["MT"], tpl["PREC"], tpl["LAY"]) == (M // 32, o.PRECISION[prec], LAY_ID[lay]), tpl
        m0, m1 = exact_wgrad_model(M, P, prec, variant, lay == B16)
        counts = {name: R.violations_exact(got.cpu(), m[0], m[2])[0]
                  for name, got, m in (("pair0", pair[0], m0), ("pair1", pair[1], m1), ("single", single[0], m1))}
        quanta = max(R.cap_quanta(m[1], m[2]) for m in (m0, m1))
        assert quanta < G.CAP_QUANTA
        log(f"cell exact wgrad {variant} M{M}P{P} {prec} {lay}".ljust(72) + f" {tpl} violations={counts} largest S_e in quanta "
            f"{quanta:.0f} cap={G.CAP_QUANTA:.0f}")
        assert not any(counts.values()), (variant, counts)
    log(f"cell exact wgrad M{M}P{P} {prec} {lay}: {_added(t0)}")
