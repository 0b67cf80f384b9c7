"""Every instance of the three kernels of the sparse matrix-core tier that the plans can reach -- k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>
(cdl_analysis_mfma.hip), k_synth_m<PH,PW,SW,KSM> with both assembles (cdl_synth_mfma.hip) and k_wgm<PH,PW,SW,NG,CT> with
k_wgm_fold (cdl_wgrad_mfma.hip) -- against the float64 model of its arithmetic (generic_arith_restate.py; DESIGN.md section
35): |got - model| <= b at every element, exact zeros off the support, the threshold sums inside the bound of the model
fed the device's own output, the CSR epilogue value for value on the device's own u, outputs and workspaces NaN-filled
before the launch, every output bit for bit the same in a second call, and on exactly-summable inputs bit equality with
the model.  The tier is forced with CDL_MFMA_*=1, CDL_MFMA_DENSE=0; each cell reads its template arguments and plan notes
from the launch trace.  The numeric predicates always run; the pinned values that follow cdl_cu_count() (which tier runs,
tpw, gy, rs, gz) are those of 256 compute units, and a case whose pins differ on another device is skipped with them.

Shapes: the smallest the plans accept, ragged in every tiled axis, M never a whole number of 32-channel tiles.
k_ana_m: code plane 27 x 130 (4 x 5 tiles of 32 x 8, the last ragged both ways; 2 workgroups of 4 and 1 tiles per row).
k_synth_m: code plane 11 x 36 and 11 x 37 (2 x 2 ragged tiles; W % 4 == 0 for the vector assemble, != 0 for the scalar one).
k_wgm: code plane 40 x 72 and 40 x 70 (2 x 2 ragged 64 x 32 tiles; Wz % 8 == 0 for the prefetching fast path, != 0 for the slow)."""
import collections
import functools

import pytest
import torch

import generic_arith_restate as R
from gpu_util import launch_sites, log

pytestmark = pytest.mark.gpu

ENV = {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "0"}
ANA, SYN, WGM = "cdl_analysis_mfma.hip:", "cdl_synth_mfma.hip:", "cdl_wgrad_mfma.hip:"
K_ANA = ANA + "k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_SYN = {4: SYN + "k_synth_m<PH,PW,SW,4>", 0: SYN + "k_synth_m<PH,PW,SW,0>"}
K_ASM = {"vector": SYN + "k_synth_assemble4<PH,PW,SW>", "scalar": SYN + "k_synth_assemble<PH,PW,SW>"}
K_WGM, K_FOLD = WGM + "k_wgm<PH,PW,SW,NG,CT>", WGM + "k_wgm_fold"
PLANES = [(3, 3, 1), (5, 5, 1), (7, 7, 1), (9, 9, 1), (9, 5, 1), (3, 3, 2), (5, 5, 2), (7, 7, 2), (9, 9, 2), (9, 5, 2)]
NAN = float("nan")

Cell = collections.namedtuple("Cell", "id N C M P sp s want notes opt")


def _cell(cid, N, C, M, P, code, s, want, notes=None, **opt):
    """P: ([Pd,]Ph,Pw); code: the code grid ([Dz,]Hz,Wz) -- the image is s times it on every axis."""
    return Cell(cid, N, C, M, tuple(P), tuple(s * d for d in code), s, want, notes or {}, opt)


def _ops(hip_env):
    import cdlnet_video_amd as cva
    for k, v in ENV.items():
        hip_env(k, v)
    return cva.ops


def _geom(o, c):
    return o.Geometry.make(c.N, c.C, c.M, c.sp, c.P, tuple(p // 2 for p in c.P), c.s)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Pins:
    """The launch-trace assertions of one case, held back until its numeric predicates have run."""

    def __init__(self):
        self.failed, self.seen = [], []

    def add(self, trace, site, want, notes=None):
        """The single record of `site`: its template arguments equal `want`, its note values include `notes`."""
        recs = launch_sites(trace).get(site, [])
        tpl = [r.template() for r in recs]
        self.seen.append((site.split(":")[1], tpl, [r.note for r in recs]))
        if len(recs) != 1 or any(tpl[0].get(k) != v for k, v in want.items()) or len(tpl[0]) < len(want):
            self.failed.append(f"{site} {want}: got {tpl or sorted(launch_sites(trace))}")
        elif notes and any(recs[0].values().get(k) != v for k, v in notes.items()):
            self.failed.append(f"{site} notes {notes}: got {recs[0].note}")
        return tpl[0] if tpl else {}

    def done(self):
        if self.failed and _cus() != 256:
            pytest.skip(f"the pinned plan values are those of 256 compute units, this device has {_cus()}: {self.failed}")
        assert not self.failed, self.failed


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan_scratch(o):
    """The grow-only scratch buffer of this stream (workspaces of the analysis and synthesis entry points), NaN-filled."""
    o._scratch(torch.device("cuda", torch.cuda.current_device()), 1).fill_(NAN)


class Tally:
    """Counts of what does NOT satisfy each predicate, worst |err| / b per form, notes on determinism."""

    def __init__(self):
        self.counts, self.ratios, self.notes = {}, {}, []

    def bound(self, name, got, model, where=None):
        val, b = model
        g = got.cpu()
        if where is not None:                                  # elements outside `where` are left out of the comparison
            g, val, b = g[where], val[where], b[where]
        self.counts[name], self.ratios[name] = R.violations_fp32(g, val, b)

    def count(self, name, n):
        self.counts[name] = int(n)

    def twice(self, name, first, second):
        if not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, second)):
            self.notes.append(f"{name}: second call differs")

    def line(self):
        return ("worst|err|/b " + " ".join(f"{k}={v:.2e}" for k, v in self.ratios.items())
                + f" violations={ {k: v for k, v in self.counts.items() if v} } {self.notes}")

    def ok(self):
        return not any(self.counts.values()) and not self.notes


# ================================================================================================ k_ana_m
ANA_CODE = (27, 130)


def _ana_cells():
    """10 planes x MT {1, 2}: M = 24 and 56.  The geometry behind a plane alternates between one channel, three channels and
    depth taps (D so small that a depth plane is absent at both ends); N makes 96 workgroups of four tiles."""
    kind = {(3, 3, 1): "d3", (5, 5, 1): "c3", (7, 7, 1): "c1", (9, 9, 1): "c1", (9, 5, 1): "d3",
            (3, 3, 2): "d5", (5, 5, 2): "c1", (7, 7, 2): "c3", (9, 9, 2): "c1", (9, 5, 2): "d9"}
    out = []
    for (PH, PW, SW) in PLANES:
        for MT, M in ((1, 24), (2, 56)):
            k = kind[(PH, PW, SW)]
            notes = dict(MTW=MT, tpw=4, ngy=1, lds_over_96k=0, wgs=96)
            if k == "d9" and MT == 2:
                k = "d5"                                       # 405 taps leave room for one channel tile only (below)
            if k in ("c1", "c3"):
                N, C, P, code = 12, 1 if k == "c1" else 3, (PH, PW), ANA_CODE
            elif k == "d3":                                    # Pd = 3, D = 2: frame -1 absent at zd = 0, frame 2 at zd = 1
                N, C, P, code = 6, 1, (3, PH, PW), (2,) + ANA_CODE
            elif k == "d5":                                    # stride 2, Pd = 5, D = 2: frames -2, -1 and 2 absent
                N, C, P, code = 12, 1, (5, PH, PW), (1,) + ANA_CODE
            else:                                              # the shipped 9 x 9 x 5 bank, D = 4: frames -4 .. -1 and 4 absent
                N, C, P, code = 6, 1, (9, PH, PW), (2,) + ANA_CODE
                notes.update(lds_over_96k=1)
            out.append(_cell(f"ana-P{PH}x{PW}s{SW}-{k}-M{M}", N, C, M, P, code, SW, dict(PH=PH, PW=PW, SW=SW, MT=MT), notes))
    # three channel tiles: two channel groups on grid.y, the second with one real and one padded tile; one tile per workgroup
    for (PH, PW, SW) in ((7, 7, 1), (5, 5, 2)):
        out.append(_cell(f"ana-P{PH}x{PW}s{SW}-c1-M72", 2, 1, 72, (PH, PW), ANA_CODE, SW, dict(PH=PH, PW=PW, SW=SW, MT=2),
                         dict(MTW=2, tpw=1, ngy=2, wgs=80)))
    # the 405-tap bank at two channel tiles: the plan falls back to MT = 1 with channel groups (53 + 56 KB of LDS)
    out.append(_cell("ana-P9x5s2-d9-M56", 6, 1, 56, (9, 9, 5), (2,) + ANA_CODE, 2, dict(PH=9, PW=5, SW=2, MT=1),
                     dict(MTW=1, ngy=2, lds_over_96k=1, wgs=192)))
    return out


ANA_CELLS = _ana_cells()
# thresholds of both signs: the general shrinkage (tau_neg), compared where |u| > b; one per stride
SIGN_MIXED = [_cell("ana-P5x5s1-c1-M24-mixed", 12, 1, 24, (5, 5), ANA_CODE, 1, dict(PH=5, PW=5, SW=1, MT=1), mixed=True),
              _cell("ana-P7x7s2-c1-M24-mixed", 12, 1, 24, (7, 7), ANA_CODE, 2, dict(PH=7, PW=7, SW=2, MT=1), mixed=True)]

# ================================================================================================ k_synth_m
def _syn_cells():
    """Per plane: KSM = 4 (M = 24, G = 3), KSM = 0 resident (G = 1, M = 56), KSM = 0 per group (M = 72, G = 3), and the
    streamed fragments where the plan streams them (9 x 9: M = 152; 7 x 7 and 9 x 5: M = 360).  G = 3 alternates between three
    channels and three depth taps; mask and sub on half the cases, gated on half."""
    out = []
    for i, (PH, PW, SW) in enumerate(PLANES):
        deep = i % 2 == 1
        for j, (M, G, ksm, streamed) in enumerate(((24, 3, 4, 0), (56, 1, 0, 0), (72, 3, 0, 0), (152 if PH * PW == 81 else 360, 1, 0, 1))):
            if streamed and PH * PW < 45:
                continue                                       # 3 x 3 and 5 x 5 stream above M = 944 only
            if G == 1:
                N, C, P, code = 2, 1, (PH, PW), ()
            elif deep:                                         # Pd = 3 over D = 2 frames
                N, C, P, code = 2, 1, (3, PH, PW), (2 // SW,)
            else:
                N, C, P, code = 2, 3, (PH, PW), ()
            gy = 1 if G == 1 else 3
            out.append(_cell(f"syn-P{PH}x{PW}s{SW}-M{M}G{G}{'d' if G > 1 and deep else 'c'}", N, C, M, P, code, SW,
                             dict(PH=PH, PW=PW, SW=SW), dict(streamed=streamed, gy=gy), ksm=ksm,
                             masked=(i + j) % 2 == 0, gated=(i + j // 2) % 2 == 0))
    return out


SYN_CELLS = _syn_cells()

# ================================================================================================ k_wgm
# (PH, PW, SW, NG, CT) that launch<PH,PW,SW> instantiates: NG in {1, 3, 5} with one tap tile, {1, 3} with two, {1} with three
WGM_COMPILED = {(PH, PW, SW, NG, CT) for (PH, PW, SW) in PLANES for CT in (1, 2)
                for NG in ((1, 3, 5) if PH * PW <= 32 else (1, 3) if PH * PW <= 64 else (1,))}
# compiled and reached by no geometry: (cell, why, the instance a G = 5 geometry of the plane runs instead)
WGM_REFUSED = {
    (3, 3, 2, 5): ("plan_for: five stride-2 planes of 65 x 129 bf16 hi + lo are 164 KB, above LDS_MAX = 128 KB", 3),
    (5, 5, 2, 5): ("plan_for: five stride-2 planes of 67 x 131 bf16 hi + lo are 172 KB, above LDS_MAX = 128 KB", 3),
}


def _wgm_cells():
    """Every (plane, NG, CT) the plan reaches: NG through G = 1, 3, 5 (channels / depth taps alternating), CT = 2 through
    M = 72, CT = 1 through M = 24, 56 and 100.  Below three channel tiles the plan wants 64 tiles, and it keeps NG = 3
    only above 64 (below, one group per pass): those cells run 17 samples of 4 tiles (9 x 2 code depths of 4).  The others
    run 2 samples (1 x 2 depths): the plan then splits rows (rs) and spreads group passes (gz) as its notes say."""
    out = []
    for i, (PH, PW, SW) in enumerate(PLANES):
        T = PH * PW
        for NG in ((1, 3, 5) if T <= 32 else (1, 3) if T <= 64 else (1,)):
            if (PH, PW, SW, NG) in WGM_REFUSED:
                continue
            for CT, M in ((1, 24), (1, 56), (1, 100), (2, 72)):
                deep = NG > 1 and (i + (NG == 5)) % 2 == 0
                big = M < 65 or NG == 3
                if deep:                                       # Pd = G over 2 code depths: absent planes at both ends
                    N, C, P, code = (9 if big else 1), 1, (NG, PH, PW), (2,)
                else:
                    N, C, P, code = (17 if big else 2), NG, (PH, PW), ()
                out.append(_cell(f"wgm-P{PH}x{PW}s{SW}-NG{NG}CT{CT}-M{M}{'d' if deep else 'c'}", N, C, M, P, code, SW,
                                 dict(PH=PH, PW=PW, SW=SW, NG=NG, CT=CT)))
    # CT = 2 with whole tiles per work item (rs = 1): enough tiles that no row split is made
    out.append(_cell("wgm-P3x3s1-NG1CT2-M72c-rs1", 17, 1, 72, (3, 3), (), 1, dict(PH=3, PW=3, SW=1, NG=1, CT=2), dict(rs=1, gz=1)))
    # three groups over NG = 1 on 8 tiles: the plan splits the rows in two (rs) and spreads the group passes over grid.z (gz)
    for SW in (1, 2):
        out.append(_cell(f"wgm-P9x9s{SW}-NG1CT2-M72c-G3", 2, 3, 72, (9, 9), (), SW, dict(PH=9, PW=9, SW=SW, NG=1, CT=2), dict(rs=2, gz=3)))
    # 132 tiles: a paired launch has more work items than compute units, so a workgroup accumulates two tiles (tpw = 2)
    out.append(_cell("wgm-P3x3s1-NG1CT1-M24c-tpw2", 33, 1, 24, (3, 3), (), 1, dict(PH=3, PW=3, SW=1, NG=1, CT=1), dict(rs=1, gz=1, tpw=1),
                     pair_notes=dict(tpw=2)))
    out.append(_cell("wgm-P5x5s2-NG3CT1-M24c-tpw2", 33, 3, 24, (5, 5), (), 2, dict(PH=5, PW=5, SW=2, NG=3, CT=1), dict(rs=1, gz=1, tpw=1),
                     pair_notes=dict(tpw=2)))
    # G = 5 over NG = 3: the second pass holds two real groups and an empty one
    out.append(_cell("wgm-P7x7s1-NG3CT1-M24d-G5", 9, 1, 24, (5, 7, 7), (2,), 1, dict(PH=7, PW=7, SW=1, NG=3, CT=1)))
    return out


WGM_CELLS = _wgm_cells()
WGM_CODE = {True: (40, 72), False: (40, 70)}                  # by Wz % 8 == 0

# ================================================================================================ the exact inputs
# (kernel, cell id, variant): bit equality with the model on generic_arith_restate.exact_inputs
EXACT_CASES = [(k, cid, v) for k, cid in (("ana", "ana-P9x5s2-d9-M24"), ("ana", "ana-P5x5s1-c3-M56"), ("ana", "ana-P7x7s1-c1-M72"),
                                          ("syn", "syn-P7x7s2-M360G1c"), ("syn", "syn-P9x9s1-M24G3d"), ("syn", "syn-P5x5s2-M72G3c"),
                                          ("wgm", "wgm-P5x5s1-NG3CT1-M24c"), ("wgm", "wgm-P9x5s2-NG3CT2-M72c"),
                                          ("wgm", "wgm-P9x9s1-NG1CT1-M100c"))
               for v in ("hilo", "integer")]
BY_ID = {c.id: c for c in ANA_CELLS + SIGN_MIXED + SYN_CELLS + WGM_CELLS}


def _seed(c):
    return 11 + sum(c.P) + c.M + len(c.sp) + 3 * c.s + c.N


def _sized(c, kind, aligned=True):
    """The cell with its code plane filled in (the synthesis and filter-gradient cells run at two widths)."""
    if kind == "ana":
        return c
    plane = (11, 36 if aligned else 37) if kind == "syn" else WGM_CODE[aligned]
    code = tuple(d // c.s for d in c.sp) + plane
    return c._replace(sp=tuple(c.s * d for d in code))


@functools.lru_cache(maxsize=4)
def cell_data(cid, kind="ana", aligned=True):
    c = _sized(BY_ID[cid], kind, aligned)
    return R.stage_inputs(c.N, c.C, c.M, c.P, c.sp, c.s, seed=_seed(c), tau_sign_mixed=bool(c.opt.get("mixed")))


EXACT_ONLY = {"ana": ("x", "w", "u", "gate", "z"), "syn": ("z", "w", "gate", "x2"), "wgm": ("F", "F2", "gate", "x", "x2")}


@functools.lru_cache(maxsize=2)
def exact_data(kind, cid, variant="hilo", aligned=True):
    """The exactly-summable operands of a cell (generic_arith_restate.exact_inputs), the synthesis with mask and sub."""
    c = _sized(BY_ID[cid], kind, aligned)
    d = R.exact_inputs(c.N, c.C, c.M, c.P, c.sp, c.s, seed=_seed(c) + 1, integer=variant == "integer", only=EXACT_ONLY[kind])
    if kind == "syn":
        d["mask"], d["sub"] = (d["x2"] != 0).float(), d["x2"]
    return d


def exact_models(kind, c, d):
    """{form: model value} of the forms compared bit for bit."""
    if kind == "ana":
        core = R.analysis_core(d["x"], d["w"], c.s)
        return {"gated": R.analysis_form(d["x"], d["w"], c.s, 1.0, zin=d["u"], gate=d["gate"], core=core)[0],
                "rev": R.analysis_form(d["x"], d["w"], c.s, -1.0, zin=d["u"], zsup=d["z"], core=core)[0]}
    if kind == "syn":
        return {"synth": R.synth_form(d["z"], d["w"], c.s, gate=d["gate"], mask=d["mask"], sub=d["sub"])[0]}
    return {"single": R.wgrad_value(d["F"], d["x"], c.P, c.s, -1.0), "gated": R.wgrad_value(d["F"], d["x"], c.P, c.s, 0.5, d["gate"]),
            "pair1": R.wgrad_value(d["F2"], d["x2"], c.P, c.s, 1.0)}


def exact_cap_quanta(kind, c, d, variant):
    """Upper bounds, in quanta, of the sum of the absolute kept products per output element of the forms above; the CPU test
    asserts them below generic_arith_restate.CAP_QUANTA for every exact input of this file.  Analysis: C Pd Ph Pw terms and
    the base.  Synthesis: the model's own S_e.  Filter gradient: the non-zero code pixels of a channel, one term each."""
    tq = R.exact_term_quanta(variant == "integer")
    if kind == "ana":
        return {"u": (c.C * torch.tensor(c.P).prod().item() + 1) * tq}
    if kind == "syn":
        S = R.abs_sum(lambda a, b: R.synthesis(a, b, c.s), d["z"] * (d["gate"] != 0), d["w"]) + d["sub"].abs()
        return {"synth": float(S.max()) / d["quantum"]}
    return {k: float((d[k] != 0).sum(dim=(0,) + tuple(range(2, d[k].dim()))).max()) * tq for k in ("F", "F2")}


def exact_inputs_of_this_file():
    """(kind, cell id, variant, aligned) of every exact input a test below feeds a kernel."""
    out = [(k, cid, v, True) for k, cid, v in EXACT_CASES]
    out += [("syn", c.id, "hilo", al) for c in SYN_CELLS for al in (True, False)]
    out += [("wgm", c.id, "hilo", al) for c in WGM_CELLS for al in (True, False)]
    return out


# ================================================================================================ analysis: the runs
def _run_analysis_forms(o, g, c, dc, T, pins):
    """The six kernel forms and the two CSR forms of one cell on seeded random data."""
    dv = {k: v.cuda() for k, v in dc.items()}
    core = R.analysis_core(dc["x"], dc["w"], c.s)
    form = lambda **kw: R.analysis_form(dc["x"], dc["w"], c.s, core=core, **kw)
    new = lambda: torch.full(g.code_shape(), NAN, device="cuda")
    mixed = bool(c.opt.get("mixed"))

    def fwd(name, flags, alpha, zin, gate, tau, cmap=None, tslope=None):
        outs = []
        for _ in range(2):
            _nan_scratch(o)
            out = new()
            with o.trace() as t:
                o.analysis(g, dv["x"], dv["w"], alpha, None if zin is None else dv[zin], None if gate is None else dv[gate],
                           None if tau is None else dv[tau], out, cmap=None if cmap is None else dv[cmap],
                           tslope=None if tslope is None else dv[tslope])
                torch.cuda.synchronize()
            outs.append(out)
        pins.add(t, K_ANA, dict(c.want, PROX=False, REV=False, **flags), c.notes)
        val, b, u = form(alpha=alpha, zin=None if zin is None else dc[zin], gate=None if gate is None else dc[gate],
                         tau=None if tau is None else dc[tau], cmap=None if cmap is None else dc[cmap],
                         tslope=None if tslope is None else dc[tslope], with_u=True)
        where = None
        if mixed and tau is not None:                          # the shrinkage jumps at u = 0 under a negative threshold
            where = u.abs() > b
            T.count(f"{name}.left_out_over_1pc", max(0, int((~where).sum()) - u.numel() // 100))
            T.ratios[f"{name}.left_out"] = float((~where).sum()) / u.numel()
        T.bound(name, outs[0], (val, b), where)
        T.twice(name, outs[:1], outs[1:])

    fwd("first", dict(MAP=False), 1.0, None, None, "tau")
    fwd("iter", dict(MAP=False), -1.0, "z", None, "tau")
    fwd("map", dict(MAP=True), -1.0, "z", None, "tau", "cmap", "tslope")
    if mixed:
        return
    fwd("plain", dict(MAP=False), 1.0, None, None, None)
    fwd("gated", dict(MAP=False), 1.0, "u", "z", None)
    on, neg = dc["z"] != 0, dc["z"] < 0
    for name, cmap in (("rev", None), ("revmap", "cmap")):
        outs = []
        for _ in range(2):
            _nan_scratch(o)
            out, dt = new(), torch.full((2, c.M), NAN, device="cuda")
            with o.trace() as t:
                o.analysis_rev(g, dv["x"], dv["w"], 0.5, dv["u"], dv["z"], None if cmap else dv["c"], dt, out,
                               cmap=dv[cmap] if cmap else None)
                torch.cuda.synchronize()
            outs.append((out, dt))
        pins.add(t, K_ANA, dict(c.want, PROX=False, REV=True, MAP=cmap is not None), c.notes)
        du = outs[0][0].cpu()
        T.bound(name, du, form(alpha=0.5, zin=dc["u"], zsup=dc["z"]))
        T.count(f"{name}.off", R.zeros_off_support(du, on))
        T.bound(f"{name}.dt", outs[0][1], R.dtau_sums_map(du, on, neg, dc["cmap"]) if cmap else R.dtau_sums(du, on, neg, dc["c"]))
        T.twice(name, outs[0], outs[1])
    # the CSR epilogue (the non-descriptor path): u_out inside b of the model, z the pointwise map of the DEVICE's u
    for name, both, cmap in (("prox", False, None), ("prox2", True, None), ("proxmap", False, "cmap"), ("prox2map", True, "cmap")):
        outs = []
        for _ in range(2):
            _nan_scratch(o)
            out, uo = new(), new()
            with o.trace() as t:
                o.analysis_prox(g, dv["x"], dv["w"], -1.0, dv["z"], dv["zp"], dv["lam"], dv["g1"], dv["za"] if both else None,
                                dv["g2"] if both else None, uo, out, cmap=dv[cmap] if cmap else None,
                                tslope=dv["tslope3"] if cmap else None)
                torch.cuda.synchronize()
            outs.append((out, uo))
        pins.add(t, K_ANA, dict(c.want, PROX=True, REV=False, MAP=cmap is not None), c.notes)
        u_dev = outs[0][1].cpu()
        T.bound(f"{name}.u", u_dev, form(alpha=-1.0, zin=dc["z"]))
        lam, g1, g2 = R.prox_thresholds32(dc["lam"], dc["g1"], dc["g2"] if both else None, u_dev,
                                          dc["cmap"] if cmap else None, dc["tslope3"] if cmap else None)
        T.count(f"{name}.z", R.mismatches(outs[0][0].cpu(), R.prox_csr32(u_dev, dc["zp"], lam, g1, dc["za"] if both else None, g2)))
        T.twice(name, outs[0], outs[1])


@pytest.mark.parametrize("cid", [c.id for c in ANA_CELLS + SIGN_MIXED])
def test_analysis_cell_against_the_float64_model(cid, hip_env):
    o = _ops(hip_env)
    c = BY_ID[cid]
    T, pins = Tally(), Pins()
    _run_analysis_forms(o, _geom(o, c), c, cell_data(cid), T, pins)
    log(f"ncell {cid} N{c.N}C{c.C} {c.P} {c.sp}".ljust(60) + f" {pins.seen[0][1:]} " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ synthesis: the runs
def _synth_once(o, g, dv, c, gate, mask, sub, alpha):
    _nan_scratch(o)
    out = torch.full(g.image_shape(), NAN, device="cuda")
    with o.trace() as t:
        o.synthesis(g, dv["z"], dv["w"], alpha, dv["gate"] if gate else None, dv["mask"] if mask else None,
                    dv["sub"] if sub else None, out)
        torch.cuda.synchronize()
    return out, t


@pytest.mark.parametrize("cid", [c.id for c in SYN_CELLS])
def test_synthesis_cell_against_the_float64_model(cid, hip_env):
    o = _ops(hip_env)
    T, pins = Tally(), Pins()
    c0 = BY_ID[cid]
    gated, masked = c0.opt["gated"], c0.opt["masked"]
    alpha = 1.0 if masked else -1.0
    for aligned in (True, False):
        c = _sized(c0, "syn", aligned)
        g = _geom(o, c)
        dc = cell_data(cid, "syn", aligned)
        dv = {k: dc[k].cuda() for k in ("z", "w", "gate", "mask", "sub")}
        model = R.synth_form(dc["z"], dc["w"], c.s, dc["gate"] if gated else None, dc["mask"] if masked else None,
                             dc["sub"] if masked else None, alpha)
        e = exact_data("syn", cid, "hilo", aligned)
        ev, exact = {k: e[k].cuda() for k in ("z", "w", "gate", "mask", "sub")}, exact_models("syn", c, e)["synth"]
        for forced in ((False, True) if aligned else (False,)):
            hip_env("CDL_SCALAR_ASSEMBLE", "1" if forced else "0")
            name = ("vector" if aligned and not forced else "scalar") + ("" if aligned else "W37")
            out, t = _synth_once(o, g, dv, c, gated, masked, masked, alpha)
            pins.add(t, K_SYN[c.opt["ksm"]], c.want, c.notes)
            pins.add(t, K_ASM["vector" if aligned and not forced else "scalar"], c.want)
            T.bound(name, out, model)
            T.twice(name, [out], [_synth_once(o, g, dv, c, gated, masked, masked, alpha)[0]])
            T.count(f"exact.{name}", R.mismatches(_synth_once(o, g, ev, c, True, True, True, 1.0)[0].cpu(), exact))
        hip_env("CDL_SCALAR_ASSEMBLE", "0")
    log(f"ncell {cid} N{c.N}C{c.C} {c.P} gated={int(gated)} masked={int(masked)}".ljust(60) + f" {pins.seen[0][1:]} " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ filter gradients: the runs
def _wgrad_runs(o, g, dv, c):
    """single ungated, single gated, pair: each with the workspace NaN-filled; {name: (outputs, trace)}."""
    ws, _ = o._wgrad_workspace(g, dv["x"].device)
    res = {}
    for name in ("single", "gated", "pair"):
        ws.fill_(NAN)
        with o.trace() as t:
            if name == "single":
                out = (o.wgrad(g, dv["F"], dv["x"], -1.0),)
            elif name == "gated":
                out = (o.wgrad(g, dv["u"], dv["x"], 0.5, dv["gate"]),)
            else:
                out = o.wgrad_pair(g, dv["F"], dv["x"], -1.0, dv["F2"], dv["x2"], 1.0)
            torch.cuda.synchronize()
        res[name] = (out, t)
    return res


@pytest.mark.parametrize("cid", [c.id for c in WGM_CELLS])
def test_filter_gradient_cell_against_the_float64_model(cid, hip_env):
    o = _ops(hip_env)
    T, pins = Tally(), Pins()
    plan = []
    for aligned in (True, False):
        c = _sized(BY_ID[cid], "wgm", aligned)
        g = _geom(o, c)
        dc = cell_data(cid, "wgm", aligned)
        dv = dict(F=dc["z"].cuda(), F2=dc["u"].cuda(), u=dc["u"].cuda(), gate=dc["gate"].cuda(), x=dc["x"].cuda(), x2=dc["x2"].cuda())
        first, second = _wgrad_runs(o, g, dv, c), _wgrad_runs(o, g, dv, c)
        tag = "" if aligned else "W70"
        m_single = R.wgrad_form(dc["z"], dc["x"], c.P, c.s, -1.0)
        models = {"single": (m_single,), "gated": (R.wgrad_form(dc["u"], dc["x"], c.P, c.s, 0.5, gate=dc["gate"]),),
                  "pair": (m_single, R.wgrad_form(dc["u"], dc["x2"], c.P, c.s, 1.0))}
        for name, (outs, t) in first.items():
            notes = dict(c.notes, pair=int(name == "pair"), vec4=int(aligned), **(c.opt.get("pair_notes", {}) if name == "pair" else {}))
            tpl = pins.add(t, K_WGM, c.want, notes)
            pins.add(t, K_FOLD, {})
            for i, (out, model) in enumerate(zip(outs, models[name])):
                T.bound(f"{name}{i if name == 'pair' else ''}{tag}", out, model)
            T.twice(name + tag, outs, second[name][0])
            rec = launch_sites(t).get(K_WGM, [None])[0]
            plan.append((name + tag, tpl, rec.note if rec else None))
        e = exact_data("wgm", cid, "hilo", aligned)
        ev = dict(F=e["F"].cuda(), F2=e["F2"].cuda(), u=e["F"].cuda(), gate=e["gate"].cuda(), x=e["x"].cuda(), x2=e["x2"].cuda())
        runs, exact = _wgrad_runs(o, g, ev, c), exact_models("wgm", c, e)
        for name, outs, want in (("single", runs["single"][0], ("single",)), ("gated", runs["gated"][0], ("gated",)),
                                 ("pair", runs["pair"][0], ("single", "pair1"))):
            T.count(f"exact.{name}{tag}", sum(R.mismatches(out.cpu(), exact[k]) for out, k in zip(outs, want)))
    log(f"ncell {cid} N{c.N}C{c.C} {c.P}".ljust(60) + f" {plan[0][1]} {[(p[0], p[2]) for p in plan]} " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


def test_the_refused_filter_gradient_cells_are_the_listed_ones(hip_env):
    """The compiled (plane, NG, CT) cells are those the cells above reach plus WGM_REFUSED; a G = 5 geometry of a refused plane
    runs the NG = 3 instance instead (two passes, the second with two real groups), at CT = 1 and at CT = 2."""
    o = _ops(hip_env)
    reached = {tuple(c.want[k] for k in ("PH", "PW", "SW", "NG", "CT")) for c in WGM_CELLS}
    refused = {k + (ct,) for k in WGM_REFUSED for ct in (1, 2)}
    assert reached | refused == WGM_COMPILED and not reached & refused and len(WGM_COMPILED) == 44 and len(refused) == 4
    pins, T = Pins(), Tally()
    for (PH, PW, SW, NG), (_, instead) in WGM_REFUSED.items():
        for CT, M, N in ((1, 24, 17), (2, 72, 17)):
            c = _cell(f"refused-P{PH}x{PW}s{SW}-CT{CT}", N, 5, M, (PH, PW), WGM_CODE[True], SW, {})
            g = _geom(o, c)
            dc = R.stage_inputs(c.N, c.C, c.M, c.P, c.sp, c.s, seed=_seed(c))
            with o.trace() as t:
                out = o.wgrad(g, dc["z"].cuda(), dc["x"].cuda(), -1.0)
                torch.cuda.synchronize()
            pins.add(t, K_WGM, dict(PH=PH, PW=PW, SW=SW, NG=instead, CT=CT))
            T.bound(c.id, out, R.wgrad_form(dc["z"], dc["x"], c.P, c.s, -1.0))
    log("ncell refused k_wgm cells".ljust(60) + f" {[s[1] for s in pins.seen]} " + T.line())
    assert T.ok(), (T.counts, T.ratios)
    pins.done()


# ================================================================================================ the exact inputs: the runs
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: f"{c[1]}-{c[2]}")
def test_exact_inputs_reproduce_the_model_bit_for_bit(case, hip_env):
    """Operands whose kept products sum exactly in fp32 in every order (the cap is asserted on the CPU): the device must equal the
    float64 model in value at every element, whatever its summation order."""
    o = _ops(hip_env)
    kind, cid, variant = case
    c = _sized(BY_ID[cid], kind, True)
    g = _geom(o, c)
    d = exact_data(kind, cid, variant)
    q = d["quantum"]
    models = exact_models(kind, c, d)
    dv = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    pins, got = Pins(), {}
    with o.trace() as t:
        if kind == "ana":
            got["gated"] = o.analysis(g, dv["x"], dv["w"], 1.0, dv["u"], dv["gate"], None)
        elif kind == "syn":
            got["synth"] = o.synthesis(g, dv["z"], dv["w"], 1.0, dv["gate"], dv["mask"], dv["sub"])
        else:
            got["single"] = o.wgrad(g, dv["F"], dv["x"], -1.0)
        torch.cuda.synchronize()
    site = {"ana": K_ANA, "syn": K_SYN[c.opt.get("ksm", 0)], "wgm": K_WGM}[kind]
    pins.add(t, site, c.want)
    if kind == "ana":
        got["rev"] = o.analysis_rev(g, dv["x"], dv["w"], -1.0, dv["u"], dv["z"], dv["x"].new_ones(c.N), torch.zeros(2, c.M, device="cuda"))
    elif kind == "wgm":
        got["gated"] = o.wgrad(g, dv["F"], dv["x"], 0.5, dv["gate"])
        got["single_in_pair"], got["pair1"] = o.wgrad_pair(g, dv["F"], dv["x"], -1.0, dv["F2"], dv["x2"], 1.0)
        models["single_in_pair"] = models["single"]
    torch.cuda.synchronize()
    off = {k: R.quanta_off(got[k].cpu(), models[k], q) for k in got}
    log(f"ncell exact {cid} {variant}".ljust(60) + f" {pins.seen[0][1:]} (mismatches, worst in quanta) {off}")
    assert all(n == 0 for n, _ in off.values()), off
    pins.done()
