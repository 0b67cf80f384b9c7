"""Every instance of the three stage kernels of the fused generic tier that the plan accepts -- k_stage_g<P,G,MT,MODE,FOUR>
(cdl_fusedg.hip) in both arithmetics, k_stripg<P,G,MT,MODE,MAPPED> (cdl_stripg.hip, CDL_FUSEDG_STRIP=1) and
k_strip<P,S,MTP,MODE,MAPPED> (cdl_strip.hip) -- against the float64 model of its arithmetic (fusedg_arith_restate.py;
DESIGN.md section 33): |got - model| <= b at every element of z' / du, exact zeros off the map, the written map that of the
output, the assembled r_next / q (NaN-filled patches) and the threshold sums inside the bound of the model fed the device's
own z' / du, every output bit for bit the same in a second call, with and without map_out, with do_synth on and off, and
(strip kernels) in the row-strip layout.  Each cell pins its template arguments from the launch trace.  The same cells on
exactly-summable inputs, where the outputs must EQUAL the model: the last part of the file.

Shapes: the smallest with every kind of boundary.  Tile kernels (64 x 16 tiles): N = 2, plane 20 x 70 = 2 x 2 ragged tiles,
D = 3 for Pd = 3 and D = 4 for Pd = 5, 7 (fewer frames than depth taps: absent planes); M = 24 (MT = 1) and 56 (MT = 2),
multiples of 8 that are not whole 16- or 32-channel tiles.  Strip kernel: code plane 11 x 37 (19 x 37 where SEG = 8) = three
segments with a ragged last one, two strips of which the last has 5 columns; M = 32 MT - 7 (a 25-channel last tile)."""
import collections
import functools

import pytest
import torch

import fusedg_arith_restate as R
from gpu_util import launch_sites, log

pytestmark = pytest.mark.gpu

N = 2
PLANE = (20, 70)
SITE = {"tile": "cdl_fusedg.hip:k_stage_g<P,G,MT,MODE,FOUR>", "stripg": "cdl_stripg.hip:k_stripg<P,G,MT,MODE,MAPPED>",
        "strip": "cdl_strip.hip:k_strip<P,S,MTP,MODE,MAPPED>"}
STAGES = tuple(s.split("<")[0] + "<" for s in SITE.values())
MODE_ID = {"fwd": 0, "first": 1, "bwd": 2}

# ---- the (P, G, MT) table of k_stage_g / k_stripg.  M of a cell: 24 (MT = 1) / 56 (MT = 2) unless listed.
# Refused by the plan at EVERY M of the MT (cdl_fusedg_supported is asked about all of them below):
REFUSED = {
    (7, 7, 1): "cdl_grouped_plan_base: P = 7 with G = 7 is 49 ring registers on top of the tiles (spills to scratch)",
    (7, 7, 2): "cdl_grouped_plan_base: P = 7 with G = 7 is 49 ring registers on top of the tiles (spills to scratch)",
    (5, 7, 2): "tile_plan_for: LDS carve above 160 KB from M = 40 on (175 taps = 11 k-steps x 2 channel tiles of A fragments)",
    (7, 5, 2): "tile_plan_for: LDS carve above 160 KB from M = 24 on (245 taps = 16 k-steps, 2 tap tiles per group of B fragments)",
}
# Accepted at some M only: the cell runs at those instead of 24 / 56.
PARTIAL = {
    (7, 5, 1): ((8, 16), "tile_plan_for: LDS carve above 160 KB from M = 24 on; the instance serves M = 8 and 16"),
}
# form of the G groups: "c1" one channel 2-D; "c3" three image channels 2-D under the Bayer mosaic (JDD); "d" C = 1 with Pd = G
FORMS = {1: ("c1",), 3: ("c3", "d"), 5: ("d",), 7: ("d",)}

Cell = collections.namedtuple("Cell", "id C M P sp s masked bayer want")


def _tile_cells():
    out = []
    for P in (3, 5, 7):
        for G in (1, 3, 5, 7):
            for MT in (1, 2):
                if (P, G, MT) in REFUSED:
                    continue
                for M in PARTIAL.get((P, G, MT), ((24 if MT == 1 else 56,), ""))[0]:
                    for form in FORMS[G]:
                        D = () if form != "d" else ((3,) if G == 3 else (4,))
                        Pt = ((G,) if form == "d" else ()) + (P, P)
                        out.append(Cell(f"P{P}G{G}{form}MT{MT}M{M}", 3 if form == "c3" else 1, M, Pt, D + PLANE, 1,
                                        form == "c3" or MT == 2, form == "c3", dict(P=P, G=G, MT=MT)))
    return out


def _strip_cells():
    out = []
    for P in (3, 5, 7):
        for S in (1, 2):
            for MT in range(1, 7):
                hz = 19 if (P == 7 and S == 1) else 11                        # SEG = 8 there, 4 elsewhere: three segments
                out.append(Cell(f"P{P}S{S}MT{MT}M{32 * MT - 7}", 1, 32 * MT - 7, (P, P), (hz * S, 37 * S), S, (MT + S) % 2 == 0,
                                False, dict(P=P, S=S, MTP=(MT + 1) // 2)))
    return out


TILE_CELLS, STRIP_CELLS = _tile_cells(), _strip_cells()
BY_ID = {c.id: c for c in TILE_CELLS + STRIP_CELLS}


def _geom(o, cell):
    return o.Geometry.make(N, cell.C, cell.M, cell.sp, cell.P, tuple(p // 2 for p in cell.P), cell.s)


def _items(cell, kind):
    """Work items of the plan, from the decomposition written down: 64 x 16 tiles; 32-column strips of SEG-row segments."""
    D = cell.sp[0] if len(cell.sp) == 3 else 1
    H, W = cell.sp[-2] // cell.s, cell.sp[-1] // cell.s
    if kind == "tile":
        return N * D * -(-H // 16) * -(-W // 64)
    seg = (4 if cell.P[-1] <= 5 else 8) if kind == "stripg" else (8 if (cell.P[-1] == 7 and cell.s == 1) else 4)
    return N * D * -(-H // seg) * -(-W // 32)


@functools.lru_cache(maxsize=None)
def _data(cid):
    c = BY_ID[cid]
    return R.stage_inputs(N, c.C, c.M, c.P, c.sp, c.s, seed=7 + sum(c.P) + c.M + len(c.sp) + c.s, bayer=c.bayer)


@functools.lru_cache(maxsize=None)
def _model(cid, mode, prec):
    """(value, b) of the analysis half: once per (cell, mode, arithmetic), shared by the tile and the grouped strip kernel."""
    c, d = BY_ID[cid], _data(cid)
    if mode == "first":
        return R.forward_stage(d["r"], d["wA"], d["tau"], None, 1.0, prec, s=c.s)
    if mode == "fwd":
        return R.forward_stage(d["r"], d["wA"], d["tau"], d["zin"], -1.0, prec, s=c.s)
    return R.reverse_stage(d["thin"], d["wA"], d["gate"] != 0, d["base"] if mode == "bwd" else None, prec, s=c.s)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _pin(t, kind, want):
    """The one stage launch of the trace: the kernel asked for, with the template arguments asked for."""
    sites = launch_sites(t)
    stages = [k for k in sites if k.startswith(STAGES)]
    assert stages == [SITE[kind]] and len(sites[SITE[kind]]) == 1, (kind, list(sites))
    tpl = sites[SITE[kind]][0].template()
    assert tpl == want, (tpl, want)
    return tpl


def _forward(o, g, kind, cell, dv, frags, mode, prec, mapped, lay=("nchw", "nchw")):
    patches = o.fusedg_patches(g, "cuda").fill_(float("nan"))
    bits = o.fusedg_map(g, "cuda").fill_(-1) if mapped else None
    zin = None if mode == "first" else (o.fusedg_to_rsc(g, dv["zin"]) if lay[0] == "rsc" else dv["zin"])
    with o.trace() as t:
        z = o.fusedg_iter(g, dv["r"], zin, dv["tau"], frags, 1.0 if mode == "first" else -1.0, patches, map_out=bits,
                          lay_in=lay[0], lay_out=lay[1], precision=prec)
        thin = o.fusedg_assemble(g, patches, dv["mask"] if cell.masked else None, dv["sub"], 1.0)
        torch.cuda.synchronize()
    last = {"FOUR": prec == "split4"} if kind == "tile" else {"MAPPED": mapped}
    tpl = _pin(t, kind, dict(cell.want, MODE=MODE_ID[mode], **last))
    res = dict(code=z if lay[1] == "nchw" else o.fusedg_from_rsc(g, z), thin=thin, patches=patches)
    return res, bits, tpl


def _reverse(o, g, kind, cell, dv, frags, with_base, do_synth, prec, lay=("nchw", "nchw")):
    patches = o.fusedg_patches(g, "cuda").fill_(float("nan"))
    dtp = torch.full((o._fusedg_sizes(g)[2], cell.M), float("nan"), device="cuda")
    base = None if not with_base else (o.fusedg_to_rsc(g, dv["base"]) if lay[0] == "rsc" else dv["base"])
    with o.trace() as t:
        du = o.fusedg_stage_bwd(g, dv["thin"], base, dv["bits"], frags, patches if do_synth else None, dtp, do_synth,
                                lay_in=lay[0], lay_out=lay[1], precision=prec)
        dt = torch.zeros(2, cell.M, device="cuda")
        o.fusedg_dtau_reduce(g, dtp, dv["c"], dt)
        q = o.fusedg_assemble(g, patches, dv["mask"] if cell.masked else None, None, -1.0) if do_synth else None
        torch.cuda.synchronize()
    last = {"FOUR": prec == "split4"} if kind == "tile" else {"MAPPED": True}
    tpl = _pin(t, kind, dict(cell.want, MODE=2, **last))
    res = dict(code=du if lay[1] == "nchw" else o.fusedg_from_rsc(g, du), dtp=dtp, dt=dt)
    if do_synth:
        res.update(thin=q, patches=patches)
    return res, tpl


def _check_cell(o, kind, cell, prec):
    g = _geom(o, cell)
    assert o.fusedg_supported(g) and o._fusedg_sizes(g)[2] == _items(cell, kind), (cell, o._fusedg_sizes(g))
    dc = _data(cell.id)
    dv = {k: v.cuda() for k, v in dc.items()}
    dv["bits"] = o.fusedg_support_map(g, dv["gate"])
    frags = o.fusedg_prep(g, dv["wA"], dv["wB"])
    mask = dc["mask"] if cell.masked else None
    on, neg = dc["gate"] != 0, dc["gate"] < 0
    rsc = kind != "tile"
    counts, ratios, notes, tpls = {}, {}, [], []

    def viol(name, got, model):
        counts[name], ratios[name] = R.violations_fp32(got.cpu(), *model)

    for mode in ("first", "fwd"):
        res, bits, tpl = _forward(o, g, kind, cell, dv, frags, mode, prec, True)
        tpls.append(tpl)
        code = res["code"].cpu()
        viol(f"{mode}.z", code, _model(cell.id, mode, prec))
        counts[f"{mode}.map"] = int((bits != o.fusedg_support_map(g, res["code"])).sum())
        counts[f"{mode}.nan"] = int((~torch.isfinite(res["thin"])).sum())
        viol(f"{mode}.r", res["thin"], R.synth_assemble(code, dc["wB"], prec, False, mask, dc["sub"], 1.0, s=cell.s))
        if not _same(res, _forward(o, g, kind, cell, dv, frags, mode, prec, True)[0]):
            notes.append(f"{mode}: second call differs")
        plain, _, tpl = _forward(o, g, kind, cell, dv, frags, mode, prec, False)
        tpls.append(tpl)
        if not _same(res, plain):
            notes.append(f"{mode}: differs without map_out")
        for lay in ((("rsc", "rsc"), ("rsc", "nchw"), ("nchw", "rsc")) if rsc and mode == "fwd" else ()):
            if not _same(res, _forward(o, g, kind, cell, dv, frags, mode, prec, True, lay)[0]):
                notes.append(f"{mode}: layouts {lay} differ")
    for with_base in (True, False):
        mode = "bwd" if with_base else "bwd0"
        res, tpl = _reverse(o, g, kind, cell, dv, frags, with_base, True, prec)
        tpls.append(tpl)
        code = res["code"].cpu()
        viol(f"{mode}.du", code, _model(cell.id, mode, prec))
        counts[f"{mode}.off"] = R.zeros_off_support(code, on)
        counts[f"{mode}.nan"] = int((~torch.isfinite(res["thin"])).sum())
        viol(f"{mode}.q", res["thin"], R.synth_assemble(code, dc["wB"], prec, False, mask, None, -1.0, s=cell.s))
        viol(f"{mode}.dt", res["dt"], R.dtau_sums(code, on, neg, dc["c"]))
        if not _same(res, _reverse(o, g, kind, cell, dv, frags, with_base, True, prec)[0]):
            notes.append(f"{mode}: second call differs")
        dry = _reverse(o, g, kind, cell, dv, frags, with_base, False, prec)[0]
        if not _same(dry, {k: res[k] for k in dry}):
            notes.append(f"{mode}: differs without do_synth")
        for lay in ((("rsc", "rsc"), ("nchw", "rsc")) if rsc and with_base else ()):
            if not _same(res, _reverse(o, g, kind, cell, dv, frags, with_base, True, prec, lay)[0]):
                notes.append(f"{mode}: layouts {lay} differ")
    log(f"gcell {kind} {cell.id} {prec} C{cell.C} {cell.sp}".ljust(56) + f" {tpls[0]} modes {[t['MODE'] for t in tpls]} worst|err|/b "
        + " ".join(f"{k}={v:.2e}" for k, v in ratios.items()) + f" violations={ {k: v for k, v in counts.items() if v} } {notes}")
    assert not any(counts.values()) and not notes, (counts, ratios, notes)


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("cid", [c.id for c in TILE_CELLS])
def test_tile_kernel_cell_against_the_float64_model(cid, prec):
    import cdlnet_video_amd as cva
    _check_cell(cva.ops, "tile", BY_ID[cid], prec)


@pytest.mark.parametrize("cid", [c.id for c in TILE_CELLS])
def test_grouped_strip_kernel_cell_against_the_float64_model(cid, hip_env):
    import cdlnet_video_amd as cva
    hip_env("CDL_FUSEDG_STRIP", "1")
    _check_cell(cva.ops, "stripg", BY_ID[cid], "split3")


@pytest.mark.parametrize("cid", [c.id for c in STRIP_CELLS])
def test_strip_kernel_cell_against_the_float64_model(cid):
    import cdlnet_video_amd as cva
    _check_cell(cva.ops, "strip", BY_ID[cid], "split3")


# ------------------------------------------------------------------------------------------------ the table itself
@pytest.mark.parametrize("strip", ["0", "1"])
def test_the_refused_cells_are_the_listed_ones(strip, hip_env):
    """cdl_fusedg_supported at every M of every (P, G, MT), both forms of G = 3: a cell is refused at every M (REFUSED),
    accepted at the listed ones (PARTIAL) or accepted at all of them -- and then it is in TILE_CELLS.  The grouped strip
    kernel stands behind the tile plan (route_for), so its table is the same."""
    import cdlnet_video_amd as cva
    o = cva.ops
    hip_env("CDL_FUSEDG_STRIP", strip)
    got_refused, got_partial = set(), {}
    for P in (3, 5, 7):
        for G in (1, 3, 5, 7):
            for MT in (1, 2):
                Ms = range(8, 33, 8) if MT == 1 else range(40, 65, 8)
                for form in FORMS[G]:
                    D = () if form != "d" else ((3,) if G == 3 else (4,))
                    Pt = ((G,) if form == "d" else ()) + (P, P)
                    ok = tuple(M for M in Ms if o.fusedg_supported(
                        o.Geometry.make(N, 3 if form == "c3" else 1, M, D + PLANE, Pt, tuple(p // 2 for p in Pt), 1)))
                    if not ok:
                        got_refused.add((P, G, MT))
                    elif len(ok) < len(Ms):
                        got_partial[(P, G, MT)] = ok
                    if ok:
                        assert all(f"P{P}G{G}{form}MT{MT}M{M}" in BY_ID for M in PARTIAL.get((P, G, MT), ((24 if MT == 1 else 56,),))[0])
    assert got_refused == set(REFUSED) and got_partial == {k: v[0] for k, v in PARTIAL.items()}
    assert len({(c.want["P"], c.want["G"], c.want["MT"]) for c in TILE_CELLS}) == 24 - len(REFUSED) == 20
    assert len(STRIP_CELLS) == 36 and all(o.fusedg_supported(_geom(o, c)) for c in STRIP_CELLS)


@pytest.mark.parametrize("kind,cid", [("tile", "P5G3dMT1M24"), ("stripg", "P5G3dMT1M24"), ("strip", "P5S2MT3M89")])
def test_arithmetics_outside_the_table_are_refused(kind, cid, hip_env):
    """Plain bf16 (arithmetic 1) on the tile kernel, any arithmetic but split3 on the strip kernels: CDL_EUNSUPPORTED."""
    import cdlnet_video_amd as cva
    o = cva.ops
    if kind == "stripg":
        hip_env("CDL_FUSEDG_STRIP", "1")
    cell = BY_ID[cid]
    g = _geom(o, cell)
    dv = {k: v.cuda() for k, v in _data(cid).items()}
    dv["bits"] = o.fusedg_support_map(g, dv["gate"])
    frags = o.fusedg_prep(g, dv["wA"], dv["wB"])
    patches = o.fusedg_patches(g, "cuda")
    dtp = torch.empty(o._fusedg_sizes(g)[2], cell.M, device="cuda")
    for prec in (("bf16",) if kind == "tile" else ("bf16", "split4")):
        for zin in (None, dv["zin"]):
            with pytest.raises(cva._lib.HipKernelError, match="CDL_EUNSUPPORTED"):
                o.fusedg_iter(g, dv["r"], zin, dv["tau"], frags, 1.0 if zin is None else -1.0, patches, precision=prec)
        with pytest.raises(cva._lib.HipKernelError, match="CDL_EUNSUPPORTED"):
            o.fusedg_stage_bwd(g, dv["thin"], dv["base"], dv["bits"], frags, patches, dtp, True, precision=prec)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the lo . lo products
@pytest.mark.parametrize("mode", ["first", "fwd", "bwd"])
@pytest.mark.parametrize("cid", ["P3G3dMT1M24", "P5G3c3MT2M56", "P7G1c1MT1M24"])
def test_crafted_inputs_show_the_lo_lo_products_of_the_four_product_kernel(cid, mode):
    """On the crafted inputs (fusedg_arith_restate.crafted_split4_inputs) the FOUR instances pass the split4 model and fail the
    split3 model at every non-zero element; the three-product instances the other way round."""
    import cdlnet_video_amd as cva
    o = cva.ops
    cell = BY_ID[cid]
    g = _geom(o, cell)
    r, w = R.crafted_split4_inputs(N, cell.C, cell.M, cell.P, cell.sp, seed=40 + cell.M)
    frags = o.fusedg_prep(g, w.cuda(), _data(cid)["wB"].cuda())
    patches = o.fusedg_patches(g, "cuda")
    tau = torch.zeros(N, cell.M)
    ones = torch.ones(g.code_shape())
    model = {}
    for prec in R.PRECISIONS:
        if mode == "bwd":
            model[prec] = R.reverse_stage(r, w, ones.bool(), None, prec)
        else:
            model[prec] = R.forward_stage(r, w, tau, None if mode == "first" else 0 * ones, 1.0 if mode == "first" else -1.0, prec)
    nz = int((model["split4"][0] != 0).sum())
    assert nz > 0.6 * ones.numel()                            # a tap outside the clip (border, absent frame) gives a zero
    for prec, other in (("split4", "split3"), ("split3", "split4")):
        with o.trace() as t:
            if mode == "bwd":
                got = o.fusedg_stage_bwd(g, r.cuda(), None, o.fusedg_support_map(g, ones.cuda()), frags, patches,
                                         torch.empty(o._fusedg_sizes(g)[2], cell.M, device="cuda"), True, precision=prec)
            else:
                got = o.fusedg_iter(g, r.cuda(), None if mode == "first" else (0 * ones).cuda(), tau.cuda(), frags,
                                    1.0 if mode == "first" else -1.0, patches, precision=prec)
            torch.cuda.synchronize()
        tpl = _pin(t, "tile", dict(cell.want, MODE=MODE_ID[mode], FOUR=prec == "split4"))
        own, worst = R.violations_fp32(got.cpu(), *model[prec])
        impostor, _ = R.violations_fp32(got.cpu(), *model[other])
        log(f"gcell crafted {mode} {cid} {prec}".ljust(56) + f" {tpl} worst|err|/b={worst:.2e} violations of the {other} model: "
            f"{impostor} of {nz}")
        assert own == 0 and impostor == nz, (prec, own, impostor, nz)


# ------------------------------------------------------------------------------------------------ the forward sweep
@pytest.mark.parametrize("kind,cid", [("tile", "P5G3dMT1M24"), ("tile", "P7G3c3MT2M56"), ("strip", "P7S2MT4M121")])
def test_forward_sweep_launch_by_launch_against_the_float64_model(kind, cid):
    """cdl_fusedg_forward (K = 3, every code and residual kept) teacher-forced: each launch's own inputs (z_k, r_k) as the
    device produced them go to the model, the predicate is applied to its z_{k+1} and r_{k+1}; a 3-D, a JDD and a stride-2
    shape."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    K, prec = 3, "split3"
    cell = BY_ID[cid]
    g = _geom(o, cell)
    gen = torch.Generator().manual_seed(17 + cell.M)
    rnd = lambda *s: torch.randn(s, generator=gen)
    yp = rnd(*g.image_shape())
    A, B = [0.1 * rnd(*g.filter_shape()) for _ in range(K)], [0.1 * rnd(*g.filter_shape()) for _ in range(K)]
    tau = 0.3 * torch.rand(K, N, cell.M, generator=gen)
    mask = _data(cid)["mask"] if cell.masked else None
    with o.trace() as t:
        xp, zK, codes, resid, maps = loop._forward_fusedg(g, yp.cuda(), None if mask is None else mask.cuda(), tau.cuda(),
                                                          [w.cuda() for w in A], [w.cuda() for w in B], True, True)
        torch.cuda.synchronize()
    sites = launch_sites(t)
    assert [k for k in sites if k.startswith(STAGES)] == [SITE[kind]], list(sites)
    last = {"FOUR": False} if kind == "tile" else {"MAPPED": True}
    want = [dict(cell.want, MODE=1 if k == 0 else 0, **last) for k in range(K)]
    assert [r.template() for r in sites[SITE[kind]]] == want, sites[SITE[kind]]
    assert len(codes) == K and len(resid) == K - 1 and len(maps) == K
    r_in, z_in = yp, None
    counts, ratios = {}, {}
    for k in range(K):
        z_out = codes[k].cpu()
        counts[f"z{k + 1}"], ratios[f"z{k + 1}"] = R.violations_fp32(
            z_out, *R.forward_stage(r_in, A[k], tau[k], z_in, 1.0 if k == 0 else -1.0, prec, s=cell.s))
        assert torch.equal(maps[k], o.fusedg_support_map(g, codes[k])), f"map of launch {k}"
        if k < K - 1:
            thin, model = resid[k].cpu(), R.synth_assemble(z_out, B[k + 1], prec, False, mask, yp, 1.0, s=cell.s)
        else:
            thin, model = xp.cpu(), R.synth_assemble(z_out, B[0], prec, s=cell.s)
        counts[f"r{k + 1}"], ratios[f"r{k + 1}"] = R.violations_fp32(thin, *model)
        r_in, z_in = thin, z_out
    assert torch.equal(zK, codes[-1])
    log(f"gcell forward-sweep {kind} {cid} {prec}".ljust(56) + f" {want[0]} worst|err|/b " + " ".join(f"{k}={v:.2e}" for k, v in ratios.items()))
    assert not any(counts.values()), (counts, ratios)


# ------------------------------------------------------------------------------------------------ exactly-summable inputs
# operands on which every partial sum in every order is an fp32 number (the cap is asserted on the CPU,
# test_fusedg_arith_cpu.py, for every input enumerated by exact_inputs_of_this_file), so the device must EQUAL the model at
# every element.  The integer chain runs every cell of every kernel; the two hi + lo recipes once per (P, G) and per (P, S),
# MT alternating, on every kernel; the strip kernels with the row-strip layout on one side in one case per P.
def _alternating(cells, key):
    """One cell per value of `key`, MT = 1, 2, 1, ... (strip cells: MT = 1 .. 6 in turn) where the table has it."""
    out, groups = [], {}
    for c in cells:
        groups.setdefault(key(c), []).append(c)
    for i, (_, cs) in enumerate(sorted(groups.items())):
        if "MT" in cs[0].want:                                # tile cells: MT = 1, 2 in turn; G = 3: the c3 and the d form in turn
            cs = [c for c in cs if c.want["MT"] == 1 + i % 2] or cs
            out.append(cs[(i // 4) % len(cs)])
        else:
            out.append(cs[i % len(cs)])
    return out


HILO_TILE = _alternating(TILE_CELLS, lambda c: (c.want["P"], c.want["G"]))
HILO_STRIP = _alternating(STRIP_CELLS, lambda c: (c.want["P"], c.s))
RSC_CASES = {("stripg", c.id) for c in HILO_TILE if c.want["G"] == 3} | {("strip", c.id) for c in HILO_STRIP if c.s == 2}
EXACT_CASES = ([(kind, c.id, prec, "int") for c in TILE_CELLS for kind, prec in (("tile", "split3"), ("tile", "split4"), ("stripg", "split3"))]
               + [("strip", c.id, "split3", "int") for c in STRIP_CELLS]
               + [(kind, c.id, prec, recipe) for c in HILO_TILE for recipe in ("hilo-a", "hilo-p")
                  for kind, prec in (("tile", "split3"), ("tile", "split4"), ("stripg", "split3"))]
               + [("strip", c.id, "split3", recipe) for c in HILO_STRIP for recipe in ("hilo-a", "hilo-p")])
EXACT_MODES = ("first", "fwd", "bwd", "bwd0")


_EXACT_SECONDS = [0.0]                                        # the time the exact cases of this file have added, for the parity log


def _seed(c):
    return 23 + sum(c.P) + c.M + len(c.sp) + c.s


@functools.lru_cache(maxsize=4)
def _exact_operands(cid, recipe, no_bank_lo, first):
    c = BY_ID[cid]
    return R.exact_stage_inputs(recipe, "split4" if no_bank_lo else "split3", N, c.C, c.M, c.P, c.sp, c.s, _seed(c), first, c.bayer)


def exact_data(cid, prec, recipe, mode):
    """The operands of an exact case; they depend on the arithmetic only through split4's rule (no lo part in the banks) and
    on the mode only through the pass-through bank of a first stage."""
    return _exact_operands(cid, recipe, prec == "split4" and recipe != "int", mode == "first" and recipe == "hilo-p")


@functools.lru_cache(maxsize=8)
def exact_model(cid, prec, recipe, mode):
    """{output: (value, S_e, quantum)}: once per (cell, arithmetic, recipe, mode), shared by the tile and the grouped strip
    kernel when they follow each other."""
    c = BY_ID[cid]
    return R.exact_stage_model(mode, exact_data(cid, prec, recipe, mode), prec, c.s, c.masked)


def exact_inputs_of_this_file():
    """(cell id, arithmetic, recipe, mode) of every exact input a test below feeds a kernel."""
    return sorted({(cid, prec, recipe, mode) for (_, cid, prec, recipe) in EXACT_CASES for mode in EXACT_MODES})


@pytest.mark.parametrize("kind,cid,prec,recipe", EXACT_CASES)
def test_exact_inputs_hold_the_stage_to_equality(kind, cid, prec, recipe, hip_env):
    """FIRST, FWD, BWD with and without base on exactly-summable operands: z' / du, the written map (that of the output), the
    assembled r_next / q with mask, sub or the Bayer mosaic, and fusedg_dtau_reduce equal the model in value at every element
    where the recipe holds them (EXACT_HELD); what it does not hold stays inside the bound of the model fed the device's own
    z' / du."""
    import time
    import cdlnet_video_amd as cva
    o = cva.ops
    t0 = time.perf_counter()
    if kind == "stripg":
        hip_env("CDL_FUSEDG_STRIP", "1")
    cell = BY_ID[cid]
    g = _geom(o, cell)
    assert o.fusedg_supported(g)
    held = R.EXACT_HELD[recipe]
    rsc = (kind, cid) in RSC_CASES
    counts, quanta, tpls = {}, {}, []
    for mode in EXACT_MODES:
        e = exact_data(cid, prec, recipe, mode)
        dv = {k: v.cuda() for k, v in e.items() if torch.is_tensor(v)}
        dv["bits"] = o.fusedg_support_map(g, dv["gate"])
        frags = o.fusedg_prep(g, dv["wA"], dv["wB"])
        mask = e["mask"] if cell.masked else None
        on, neg = e["gate"] != 0, e["gate"] < 0
        model = exact_model(cid, prec, recipe, mode)
        fwd = mode in ("first", "fwd")
        if fwd:
            res, bits, tpl = _forward(o, g, kind, cell, dv, frags, mode, prec, True, ("rsc", "nchw") if rsc and mode == "fwd" else ("nchw", "nchw"))
            # the written map is that of the output, which equals the model (the sign bit of a zero is not the model's to say)
            counts[f"{mode}.map"] = int((bits != o.fusedg_support_map(g, res["code"])).sum())
        else:
            res, tpl = _reverse(o, g, kind, cell, dv, frags, mode == "bwd", True, prec, ("nchw", "rsc") if rsc and mode == "bwd" else ("nchw", "nchw"))
            counts[f"{mode}.off"] = R.zeros_off_support(res["code"].cpu(), on)
        tpls.append(tpl)
        code = res["code"].cpu()
        for name in ("code", "thin", "dt"):
            if name in model and name in held:
                val, S, q = model[name]
                counts[f"{mode}.{name}"], _ = R.violations_exact(res[name].cpu(), val, q)
                quanta[f"{mode}.{name}"] = R.cap_quanta(S, q)
                assert quanta[f"{mode}.{name}"] < R.CAP_QUANTA, (cid, mode, name)
        if "thin" not in held:                                # the synthesis half of the analysis recipe: the bound, as today
            counts[f"{mode}.thin<=b"], _ = R.violations_fp32(res["thin"].cpu(), *R.synth_assemble(
                code, e["wB"], prec, False, mask, e["sub"] if fwd else None, 1.0 if fwd else -1.0, s=cell.s))
            if not fwd:
                counts[f"{mode}.dt<=b"], _ = R.violations_fp32(res["dt"].cpu(), *R.dtau_sums(code, on, neg, e["c"]))
    log(f"gcell exact {recipe} {kind} {cid} {prec}{' rsc' if rsc else ''}".ljust(56) + f" {tpls[0]} modes {[t['MODE'] for t in tpls]} "
        f"violations={sum(counts.values())} { {k: v for k, v in counts.items() if v} } largest S_e in quanta "
        f"{max(quanta.values()):.0f} cap={R.CAP_QUANTA:.0f} {time.perf_counter() - t0:.2f} s")
    _EXACT_SECONDS[0] += time.perf_counter() - t0
    log(f"gcell exact: the exact cases of this file so far {_EXACT_SECONDS[0]:.1f} s")
    assert not any(counts.values()), counts
