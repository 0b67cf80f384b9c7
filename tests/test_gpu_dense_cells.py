"""Every compiled instance of the dense matrix-core tier -- k_dense<MT>, the four k_dense_vgg<MODE> forms, k_dense_wgrad<VEC>
with k_dense_wfold and both k_dense_prep launch sites (cdl_dense_mfma.hip) -- against the float64 model of its arithmetic
(dense_arith_restate.py): |got - model| <= b at every element, exact zeros where the form prescribes
them, outputs and workspaces NaN-filled before the launch, every output bit for bit the same in a second call, and on
exactly-summable inputs equality with the model.  The dense launchers are not exported, so every cell goes through a
public entry point (cva.ops.analysis / synthesis / wgrad / analysis_rev, residual_forward / residual_backward,
cdl_vgg_forward / cdl_vgg_backward) with the tier forced by CDL_MFMA_*=1; every case asserts from the launch trace that its
launches are the dense tier's (MT from k_dense<MT>'s template argument, VEC from the site name) and that nothing of the sparse
or tiled files ran.  The numeric predicates always run; the pins are those of 256 compute units and a case whose pins
differ on another device is skipped with them (nothing this tier plans follows the compute-unit count today).

Shapes: the smallest at which a path exists, ragged in every tiled axis, channel counts never a whole number of 32-channel
tiles unless the cell says so, every 3-D geometry with a depth plane absent at both ends (D = 2 under Pd = 3 or 5).
k_dense: image plane 20 x 45 (2 x 2 ragged tiles of 32 x 16), N and D set the tile count.  k_dense_wgrad: tiles of 32 x 4,
W = 72 (VEC) and 70 (scalar loads)."""
import collections
import functools

import pytest
import torch

import dense_arith_restate as R
import perceptual_restate as PR
import vgg_scratch_util as VS
from gpu_util import launch_sites, log
from test_gpu_generic_cells import NAN, Pins, Tally, _bits, _nan_scratch

pytestmark = pytest.mark.gpu

ENV = {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"}
DEN = "cdl_dense_mfma.hip:"
K_DENSE, K_VGG, K_PREP, K_PREP_VGG = DEN + "k_dense<MT>", DEN + "k_dense_vgg<MODE>", DEN + "k_dense_prep", DEN + "k_dense_prep#2"
K_WGRAD = {True: DEN + "k_dense_wgrad<true>", False: DEN + "k_dense_wgrad<false>"}
K_WFOLD = DEN + "k_dense_wfold"
FOREIGN = ("cdl_analysis_mfma.hip", "cdl_synth_mfma.hip", "cdl_wgrad_mfma.hip", "cdl_generic_tiled.hip")
PLANE = (20, 45)

Cell = collections.namedtuple("Cell", "id role N C M P sp I O MT tiles")


def _ops(hip_env):
    import cdlnet_video_amd as cva
    for k, v in ENV.items():
        hip_env(k, v)
    return cva.ops


def _geom(o, c):
    return o.Geometry.make(c.N, c.C, c.M, c.sp, c.P, tuple(p // 2 for p in c.P), 1)


def _foreign(trace):
    """Launches of the sparse matrix-core or tiled operator files in a trace."""
    return sum(1 for r in trace if r.file in FOREIGN)


def _pin_dense(pins, T, t, MT, launches=1):
    """The trace of one dense convolution call: `launches` k_dense<MT> records with their k_dense_prep, nothing foreign."""
    sites = launch_sites(t)
    recs = sites.get(K_DENSE, [])
    pins.seen.append(("k_dense", [r.template() for r in recs], []))
    if len(recs) != launches or any(r.template().get("MT") != MT for r in recs) or len(sites.get(K_PREP, [])) != launches:
        pins.failed.append(f"{launches} x k_dense<{MT}> + k_dense_prep: got {sorted((k, len(v)) for k, v in sites.items())}")
    T.counts["foreign"] = T.counts.get("foreign", 0) + _foreign(t)


# ================================================================================================ k_dense: the cells
# (plane [Pd,]Ph,Pw, channels in, channels out, N): 2-D cells have D = 1, 3-D cells D = 2; tiles = 4 N D
_DENSE = [
    ((1, 1), 16, 24, 1),        # 4 tiles (nb < 8), MT 1, one whole chunk
    ((1, 1), 40, 40, 3),        # 12 tiles (fl = 1, rem = 4), MT 2, three chunks
    ((3, 3), 20, 40, 3),        # 12 tiles; the second chunk's first half ragged, its second half empty
    ((3, 3), 24, 24, 6),        # 24 tiles (rem == 0), MT 1; no weight-staging tail (9 * 128 <= 2560)
    ((5, 5), 24, 24, 5),        # 20 tiles (fl = 2, rem = 4), MT 1, the tail (25 * 128 > 2560)
    ((5, 5), 16, 40, 1),        # 4 tiles, MT 2, the tail
    ((3, 5), 40, 24, 3),        # 12 tiles, MT 1: 15 * 128 <= 2560, no tail
    ((3, 5), 20, 72, 1),        # 4 tiles, MT 2 (the tail: 15 * 256 > 2560), ngy = 2: the second group one real and one padded tile
    ((5, 3), 24, 40, 5),        # 20 tiles, MT 2
    ((5, 3), 16, 24, 1),        # 4 tiles, MT 1
    ((3, 3, 3), 40, 72, 3),     # Pd = 3 over D = 2: 24 tiles, MT 2, ngy = 2
    ((5, 3, 3), 16, 24, 3),     # Pd = 5 over D = 2: kd = 0 and 4 never valid; 24 tiles, MT 1
    ((3, 3, 5), 20, 40, 1),     # Pd = 3, plane 3 x 5: 8 tiles (fl = 1, rem = 0), MT 2
    ((5, 5, 3), 24, 24, 3),     # Pd = 5, plane 5 x 3: 24 tiles, MT 1
]


def _dense_cells():
    out = []
    for role in ("ana", "syn"):
        for P, I, O, N in _DENSE:
            sp = ((2,) if len(P) == 3 else ()) + PLANE
            C, M = (I, O) if role == "ana" else (O, I)
            tiles = 4 * N * (2 if len(P) == 3 else 1)
            out.append(Cell(f"{role}-P{'x'.join(map(str, P))}-I{I}O{O}-t{tiles}", role, N, C, M, P, sp, I, O, 2 if O > 32 else 1, tiles))
    return out


DENSE_CELLS = _dense_cells()
# thresholds of both signs: the general shrinkage, compared where |u| > b.  (The transposed role takes no threshold
# through any public entry point: cva.ops.synthesis has none, so only the analysis role has this case.)
SIGN_MIXED = [Cell("ana-P3x3-I20O40-t12-mixed", "ana", 3, 20, 40, (3, 3), PLANE, 20, 40, 2, 12)]
BY_ID = {c.id: c for c in DENSE_CELLS + SIGN_MIXED}


def _seed(c):
    return 17 + sum(c.P) + c.M + 2 * c.C + len(c.sp) + c.N


@functools.lru_cache(maxsize=4)
def cell_data(cid):
    c = BY_ID[cid]
    return R.stage_inputs(c.N, c.C, c.M, c.P, c.sp, seed=_seed(c), tau_sign_mixed=cid.endswith("mixed"))


@functools.lru_cache(maxsize=4)
def exact_data(cid, variant):
    """The exactly-summable operands of a dense cell; the synthesis role with mask and sub."""
    c = BY_ID[cid]
    d = R.exact_inputs(c.N, c.C, c.M, c.P, c.sp, 1, seed=_seed(c) + 1, integer=variant == "integer",
                       only=("x", "x2", "w", "z", "u", "gate"))
    d["mask"], d["sub"] = (d["x2"] != 0).float(), d["x2"]
    return d


def exact_models(c, d):
    """{form: (model value, S_e)} of the forms a dense cell compares for equality on the exact inputs."""
    if c.role == "ana":
        core = R.dense_core(d["x"], d["w"])
        S = core[1] + d["u"].abs()
        return {"gated": (R.dense_form(d["x"], d["w"], add=d["u"], add_gate=d["gate"], core=core)[0], S),
                "rev": (R.dense_form(d["x"], d["w"], alpha=-1.0, add=d["u"], out_gate=d["z"], core=core)[0], S)}
    core = R.dense_core(d["z"], d["w"], True, d["gate"])
    return {"synth": (R.dense_form(d["z"], d["w"], True, in_gate=d["gate"], mask=d["mask"], sub=d["sub"], core=core)[0],
                      core[1] + d["sub"].abs())}


def exact_inputs_of_the_dense_cells():
    return [(c.id, v) for c in DENSE_CELLS for v in ("hilo", "integer")]


# ================================================================================================ k_dense: the runs
def _twice(fn):
    """fn() run twice, each on a NaN-filled scratch: ((outputs of the first call), (of the second), trace of the first)."""
    outs = []
    for _ in range(2):
        outs.append(fn())
    return outs[0][0], outs[1][0], outs[0][1]


def _run_analysis_role(o, g, c, dc, T, pins):
    dv = {k: v.cuda() for k, v in dc.items()}
    core = R.dense_core(dc["x"], dc["w"])
    form = lambda **kw: R.dense_form(dc["x"], dc["w"], core=core, **kw)
    mixed = c.id.endswith("mixed")

    def fwd(name, alpha, zin, gate, tau):
        def once():
            _nan_scratch(o)
            out = torch.full(g.code_shape(), NAN, device="cuda")
            with o.trace() as t:
                o.analysis(g, dv["x"], dv["w"], alpha, None if zin is None else dv[zin], None if gate is None else dv[gate],
                           None if tau is None else dv[tau], out)
                torch.cuda.synchronize()
            return (out,), t
        first, second, t = _twice(once)
        _pin_dense(pins, T, t, c.MT)
        val, b, u = form(alpha=alpha, add=None if zin is None else dc[zin], add_gate=None if gate is None else dc[gate],
                         tau=None if tau is None else dc[tau], with_u=True)
        where = None
        if mixed:                                              # the shrinkage jumps at u = 0 under a negative threshold
            where = u.abs() > b
            T.count(f"{name}.left_out_over_1pc", max(0, int((~where).sum()) - u.numel() // 100))
            T.ratios[f"{name}.left_out"] = float((~where).sum()) / u.numel()
        T.bound(name, first[0], (val, b), where)
        T.twice(name, first, second)

    fwd("first", 1.0, None, None, "tau")
    fwd("iter", -1.0, "z", None, "tau")
    if mixed:
        return
    fwd("plain", 1.0, None, None, None)
    fwd("gated", 1.0, "u", "z", None)
    fwd("alpha", 0.75, "u", None, None)                        # not a power of two: alpha * acc rounds, fma or not

    def rev():
        _nan_scratch(o)
        out, dt = torch.full(g.code_shape(), NAN, device="cuda"), torch.full((2, c.M), NAN, device="cuda")
        with o.trace() as t:
            o.analysis_rev(g, dv["x"], dv["w"], 0.5, dv["u"], dv["z"], dv["c"], dt, out)
            torch.cuda.synchronize()
        return (out, dt), t
    first, second, t = _twice(rev)
    _pin_dense(pins, T, t, c.MT)
    du, on, neg = first[0].cpu(), dc["z"] != 0, dc["z"] < 0
    T.bound("rev", du, form(alpha=0.5, add=dc["u"], out_gate=dc["z"]))
    T.count("rev.off", R.zeros_off_support(du, on))
    T.bound("rev.dt", first[1], R.dtau_sums(du, on, neg, dc["c"]))
    T.twice("rev", first, second)


def _run_synthesis_role(o, g, c, dc, T, pins):
    dv = {k: dc[k].cuda() for k in ("z", "w", "gate", "mask", "sub")}
    cores = {False: R.dense_core(dc["z"], dc["w"], True), True: R.dense_core(dc["z"], dc["w"], True, dc["gate"])}
    for name, gated, mask, sub, alpha in (("plain", False, False, False, 1.0), ("gated", True, False, False, -1.0),
                                          ("mask", False, True, False, 1.0), ("sub", True, False, True, 1.0),
                                          ("masksub", False, True, True, -1.0)):
        def once():
            _nan_scratch(o)
            out = torch.full(g.image_shape(), NAN, device="cuda")
            with o.trace() as t:
                o.synthesis(g, dv["z"], dv["w"], alpha, dv["gate"] if gated else None, dv["mask"] if mask else None,
                            dv["sub"] if sub else None, out)
                torch.cuda.synchronize()
            return (out,), t
        first, second, t = _twice(once)
        _pin_dense(pins, T, t, c.MT)
        T.bound(name, first[0], R.dense_form(dc["z"], dc["w"], True, alpha, dc["gate"] if gated else None,
                                             dc["mask"] if mask else None, sub=dc["sub"] if sub else None, core=cores[gated]))
        T.twice(name, first, second)


def _run_exact(o, g, c, T, pins):
    """Both exact variants of a cell: the gated and the reverse form (analysis role), gate + mask + sub (synthesis role)."""
    for variant in ("hilo", "integer"):
        d = exact_data(c.id, variant)
        dv = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
        models = exact_models(c, d)
        _nan_scratch(o)
        got = {}
        with o.trace() as t:
            if c.role == "ana":
                got["gated"] = o.analysis(g, dv["x"], dv["w"], 1.0, dv["u"], dv["gate"], None)
                got["rev"] = o.analysis_rev(g, dv["x"], dv["w"], -1.0, dv["u"], dv["z"], dv["x"].new_ones(c.N),
                                            torch.zeros(2, c.M, device="cuda"))
            else:
                got["synth"] = o.synthesis(g, dv["z"], dv["w"], 1.0, dv["gate"], dv["mask"], dv["sub"])
            torch.cuda.synchronize()
        _pin_dense(pins, T, t, c.MT, launches=len(got))
        for k, v in got.items():
            T.count(f"exact.{variant}.{k}", R.mismatches(v.cpu(), models[k][0]))


@pytest.mark.parametrize("cid", [c.id for c in DENSE_CELLS + SIGN_MIXED])
def test_dense_cell_against_the_float64_model(cid, hip_env):
    o = _ops(hip_env)
    c = BY_ID[cid]
    g = _geom(o, c)
    T, pins = Tally(), Pins()
    (_run_analysis_role if c.role == "ana" else _run_synthesis_role)(o, g, c, cell_data(cid), T, pins)
    if not cid.endswith("mixed"):
        _run_exact(o, g, c, T, pins)
    log(f"dcell {cid} N{c.N} C{c.C} M{c.M} {c.P} {c.sp} MT{c.MT}".ljust(64) + " " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ the residual block's forms
RES_SP = (2, 17, 33)


@functools.lru_cache(maxsize=2)
def residual_data(M, kind="random"):
    if kind == "random":
        d = R.stage_inputs(1, M, M, (3, 3, 3), RES_SP, seed=31 + M)
        return dict(x=d["x"], w1=d["w"], w2=d["w2"], g_out=d["x2"])
    e = R.exact_inputs(1, M, M, (3, 3, 3), RES_SP, 1, seed=32 + M, integer=kind == "integer", only=("x", "w"))
    return dict(x=e["x"], w1=e["w"], quantum=e["quantum"])


def _where(cond, v):
    return torch.where(cond, v, torch.zeros_like(v))


@pytest.mark.parametrize("M", [24, 40])
def test_residual_forms_against_the_model_and_the_plain_dense_launches(M, hip_env):
    """relu; relu with add = x; the transposed role with out_gate = h (dh is internal: held through dx and dw1, which are
    computed from it) and with add = g2.  Second predicate: every output equals in every bit the same form computed on the
    host in fp32 from the plain dense cva.ops.analysis / synthesis of the same operands (the same template body)."""
    o = _ops(hip_env)
    MT = 2 if M > 32 else 1
    d = residual_data(M)
    g = o.residual_geometry(d["x"], d["w1"])
    dv = {k: v.cuda() for k, v in d.items()}
    T, pins = Tally(), Pins()

    def forward():
        _nan_scratch(o)
        with o.trace() as t:
            h, out = o.residual_forward(g, dv["x"], dv["w1"], dv["w2"])
            torch.cuda.synchronize()
        return (h, out), t
    (h, out), second, t = _twice(forward)
    _pin_dense(pins, T, t, MT, launches=2)
    T.twice("forward", (h, out), second)
    hc, oc = h.cpu(), out.cpu()
    T.bound("relu", hc, R.dense_form(d["x"], d["w1"], relu=True))
    T.bound("relu_add", oc, R.dense_form(hc, d["w2"], add=d["x"], relu=True))
    zero = torch.zeros((), device="cuda")
    T.count("relu.bits", int((_bits(h) != _bits(torch.maximum(o.analysis(g, dv["x"], dv["w1"]), zero))).sum()))
    T.count("relu_add.bits", int((_bits(out) != _bits(torch.maximum(o.analysis(g, h, dv["w2"], 1.0, dv["x"]), zero))).sum()))

    def backward():
        _nan_scratch(o)
        o._wgrad_workspace(g, h.device)[0].fill_(NAN)
        with o.trace() as t:
            res = o.residual_backward(g, dv["x"], h, out, dv["w1"], dv["w2"], dv["g_out"])
            torch.cuda.synchronize()
        return res, t
    (dx, dw1, dw2), second, t = _twice(backward)
    _pin_dense(pins, T, t, MT, launches=2)
    sites = launch_sites(t)
    vec = RES_SP[-1] % 4 == 0
    if len(sites.get(K_WGRAD[vec], [])) != 2 or len(sites.get(K_WFOLD, [])) != 2:
        pins.failed.append(f"two k_dense_wgrad<{vec}> + k_dense_wfold: got {sorted(sites)}")
    T.twice("backward", (dx, dw1, dw2), second)
    # on the host: g2 = g_out [out > 0] (one exact pass), dh = S(g2; w2) [h != 0] from the plain dense synthesis, dx = S(dh; w1) + g2
    g2 = _where(out > 0, dv["g_out"])
    dh = _where(h != 0, o.synthesis(g, g2, dv["w2"]))
    g2c, dhc = g2.cpu(), dh.cpu()
    T.bound("dh(plain)", dhc, R.dense_form(g2c, d["w2"], True, out_gate=hc))
    T.count("dh.off", R.zeros_off_support(dhc, hc != 0))
    T.bound("dx", dx, R.dense_form(dhc, d["w1"], True, add=g2c))
    T.count("dx.bits", int((_bits(dx) != _bits(o.synthesis(g, dh, dv["w1"]) + g2)).sum()))
    T.bound("dw2", dw2, R.wgrad_form(g2c, hc, (3, 3, 3)))
    T.bound("dw1", dw1, R.wgrad_form(dhc, d["x"], (3, 3, 3)))
    T.count("dw1.bits", int((_bits(dw1) != _bits(o.wgrad(g, dh, dv["x"]))).sum()))
    # exact inputs through the ReLU form
    for variant in ("hilo", "integer"):
        e = residual_data(M, variant)
        he, _ = o.residual_forward(g, e["x"].cuda(), e["w1"].cuda(), dv["w2"])
        T.count(f"exact.{variant}.relu", R.mismatches(he.cpu(), R.dense_form(e["x"], e["w1"], relu=True)[0]))
    log(f"dcell residual M{M} {RES_SP} MT{MT}".ljust(64) + " " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ k_dense_wgrad + k_dense_wfold
WCell = collections.namedtuple("WCell", "id N C M Pd D H why")
WGRAD_CELLS = [
    # the channel cells: Pd = 3 over D = 2, 9 rows (3 tile rows, the last ragged), N = 2: 36 tiles
    WCell("wg-C24M24", 2, 24, 24, 3, 2, 9, "narrow: nine taps over eight waves"),
    WCell("wg-C24M40", 2, 24, 40, 3, 2, 9, "wide with a padded channel pair"),
    WCell("wg-C24M72", 2, 24, 72, 3, 2, 9, "group 0 wide and group 1 narrow in one launch"),
    WCell("wg-C40M72", 2, 40, 72, 3, 2, 9, "both groups wide"),
    WCell("wg-C64M64", 2, 64, 64, 3, 2, 9, "nothing padded"),
    # the tile-walk cells
    WCell("wg-Pd1-one-tile-each", 3, 24, 40, 1, 1, 9, "nwg == ntiles"),
    WCell("wg-Pd3-two-tiles", 2, 24, 72, 3, 2, 20, "ntiles > nwg"),
    WCell("wg-Pd5-empty-kd", 2, 24, 72, 5, 2, 9, "empty kd"),
    WCell("wg-Pd3-D1", 8, 24, 24, 3, 1, 4, "empty kd"),
]
NARROW_IMAGE = WCell("wg-W12H33", 1, 24, 40, 1, 1, 33, "a single ragged tile column")
W_BY_ID = {c.id: c for c in WGRAD_CELLS + [NARROW_IMAGE]}
W_WIDTHS = {True: 72, False: 70}


def _wsp(c, W):
    return ((c.D,) if c.Pd > 1 or c.D > 1 else ()) + (c.H, W)


def _wP(c):
    return ((c.Pd,) if c.Pd > 1 or c.D > 1 else ()) + (3, 3)


def wgrad_widths(c):
    return (12,) if c.id == NARROW_IMAGE.id else (72, 70)


@functools.lru_cache(maxsize=2)
def wgrad_data(cid, W, kind="random"):
    c = W_BY_ID[cid]
    seed = 41 + c.C + c.M + c.Pd + c.H + W
    if kind == "random":
        d = R.stage_inputs(c.N, c.C, c.M, _wP(c), _wsp(c, W), seed=seed)
        return dict(F=d["z"], u=d["u"], gate=d["gate"], x=d["x"])
    e = R.exact_inputs(c.N, c.C, c.M, _wP(c), _wsp(c, W), 1, seed=seed + 1, integer=kind == "integer", only=("F", "gate", "x"))
    return dict(F=e["F"], u=e["F"], gate=e["gate"], x=e["x"], quantum=e["quantum"])


def exact_inputs_of_the_wgrad_cells():
    return [(c.id, W, v) for c in WGRAD_CELLS + [NARROW_IMAGE] for W in wgrad_widths(c) for v in ("hilo", "integer")]


def _wgrad_runs(o, g, dv):
    """ungated and gated, each with the workspace NaN-filled; {name: (output, trace)}."""
    ws, _ = o._wgrad_workspace(g, dv["x"].device)
    res = {}
    for name in ("single", "gated"):
        ws.fill_(NAN)
        with o.trace() as t:
            out = o.wgrad(g, dv["F"], dv["x"], -1.0) if name == "single" else o.wgrad(g, dv["u"], dv["x"], 0.5, dv["gate"])
            torch.cuda.synchronize()
        res[name] = (out, t)
    return res


@pytest.mark.parametrize("cid", list(W_BY_ID))
def test_filter_gradient_cell_against_the_float64_model(cid, hip_env):
    o = _ops(hip_env)
    c = W_BY_ID[cid]
    T, pins = Tally(), Pins()
    for W in wgrad_widths(c):
        vec = W % 4 == 0
        P, sp = _wP(c), _wsp(c, W)
        g = o.Geometry.make(c.N, c.C, c.M, sp, P, tuple(p // 2 for p in P), 1)
        plan = R.wgrad_plan(c.N, c.C, c.M, c.D, c.H, W, c.Pd)
        dc = wgrad_data(cid, W)
        dv = {k: v.cuda() for k, v in dc.items()}
        first, second = _wgrad_runs(o, g, dv), _wgrad_runs(o, g, dv)
        models = {"single": R.wgrad_form(dc["F"], dc["x"], P, -1.0), "gated": R.wgrad_form(dc["u"], dc["x"], P, 0.5, gate=dc["gate"])}
        empty = [kd for kd in range(c.Pd) if plan["valid"][kd] == 0]
        for name, (out, t) in first.items():
            pins.add(t, K_WGRAD[vec], {})
            pins.add(t, K_WFOLD, {})
            T.counts["foreign"] = T.counts.get("foreign", 0) + _foreign(t)
            T.bound(f"{name}W{W}", out, models[name])
            T.twice(f"{name}W{W}", [out], [second[name][0]])
            if empty:                                          # banks of a kd with no valid depth plane: exact zeros
                T.count(f"{name}W{W}.empty_kd", int((~(out[:, :, empty] == 0)).sum()))
        for variant in ("hilo", "integer"):
            e = wgrad_data(cid, W, variant)
            ev = {k: v.cuda() for k, v in e.items() if torch.is_tensor(v)}
            runs = _wgrad_runs(o, g, ev)
            T.count(f"exact.{variant}.singleW{W}", R.mismatches(runs["single"][0].cpu(), R.wgrad_value(e["F"], e["x"], P, -1.0)))
            T.count(f"exact.{variant}.gatedW{W}", R.mismatches(runs["gated"][0].cpu(), R.wgrad_value(e["u"], e["x"], P, 0.5, e["gate"])))
    log(f"dcell {cid} N{c.N} C{c.C} M{c.M} Pd{c.Pd} D{c.D} H{c.H} ({c.why}; nwg {plan['nwg']} of {plan['ntiles']} tiles)".ljust(64)
        + " " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ the VGG forms
def _tied_input(P, H, W):
    """A piecewise-constant input (constant 32 x 32 blocks), as test_gpu_perceptual's tie test builds it."""
    g = torch.Generator().manual_seed(13)
    blocks = torch.rand((P, -(-H // 32), -(-W // 32)), generator=g)
    return blocks.repeat_interleave(32, -2).repeat_interleave(32, -1)[:, :H, :W].contiguous()


VGG_CASES = {"P2-39x51": (2, 39, 51, False), "P3-39x70": (3, 39, 70, False), "ties-P2-64x64": (2, 64, 64, True)}


def _vgg_inputs(P, H, W, tied):
    if tied:
        return _tied_input(P, H, W), torch.zeros(P, H, W)
    g = torch.Generator().manual_seed(5 + P + H + W)
    x = torch.rand((P, H, W), generator=g)
    return x, (x + 0.1 * torch.randn(x.shape, generator=g)).clamp(0, 1)


@pytest.mark.parametrize("case", list(VGG_CASES))
def test_vgg_forms_against_the_model_and_the_plain_dense_launches(case, hip_env):
    """Per layer, on the DEVICE's own input activation: the plain dense analysis of it is inside b of the model (the VGG
    channel counts), and the layer's stored output equals in every bit the form computed on the host in fp32 from that
    plain analysis -- bias, first-maximum floor pool with its codes, the diff form's seeds; every fp64 partial written and
    the loss the sum of d^2 of the device's own seeds; after the backward, g_b the plain dense synthesis of the
    host-unpooled g_a."""
    import cdlnet_video_amd as cva
    o = _ops(hip_env)
    lib = cva._lib.lib()
    P, H, W, tied = VGG_CASES[case]
    sd = PR.random_weights(12)
    if tied:
        for k in list(sd):                                     # positive biases: the ties sit at positive values
            if k.endswith("bias"):
                sd[k] = sd[k].abs() + 0.05
    xc, yc = _vgg_inputs(P, H, W, tied)
    x, y = xc.cuda(), yc.cuda()
    ws, bs = cva.metrics._vgg_tables(sd, x.device)
    wt, bt = o._ptr_table(ws), o._ptr_table(bs)
    n = int(lib.cdl_vgg_scratch_floats(P, H, W, 3))
    L = VS.scratch_layout(P, H, W, 3)
    assert n == L["total"]
    T, pins = Tally(), Pins()

    def forward():
        scr = torch.full((n,), NAN, device="cuda")
        loss = torch.full((), NAN, device="cuda")
        with o.trace() as t:
            cva._lib.check(lib.cdl_vgg_forward(o._ptr(x), o._ptr(y), P, H, W, wt, bt, 3, None, o._ptr(loss), o._ptr(scr), n,
                                               o._stream()), "cdl_vgg_forward")
            torch.cuda.synchronize()
        return (scr, loss), t
    (scr, loss), (scr2, loss2), t = _twice(forward)
    sites = launch_sites(t)
    modes = sorted(r.template().get("MODE") for r in sites.get(K_VGG, []))
    pins.seen.append(("k_dense_vgg", modes, []))
    if modes != [1] * 7 + [3] * 4 + [5] or len(sites.get(K_PREP_VGG, [])) != 12:
        pins.failed.append(f"12 k_dense_vgg launches (7 bias, 4 pool, 1 diff) + preps: got {modes}, {sorted(sites)}")
    T.count("foreign", _foreign(t))
    same = scr.view(torch.int32) == scr2.view(torch.int32)
    T.count("second_call_differs", int((~same).sum()) + int(_bits(loss) != _bits(loss2)))
    s0, s1, fy = VS.scratch_views(scr, P, H, W, 3)
    ex = VS.scratch_extras(scr, P, H, W, 3)
    zero = torch.zeros((), device="cuda")
    names_in, names_out = ("a1", "p1", "a3", "p2", "a5", "a6"), ("p1", "a3", "p2", "a5", "a6", None)
    codes = ("am1", None, "am2", None, None, None)
    ties = []
    for side, s in (("x", s0), ("y", s1)):
        for l, ((ci, co), lev) in enumerate(zip(VS.VGG_LAYERS, VS.VGG_LEVEL)):
            a_in = s[names_in[l]]
            Hl, Wl = L["dims"][lev]
            g = o.Geometry.make(P, ci, co, (Hl, Wl), (3, 3), (1, 1), 1)
            _nan_scratch(o)
            with o.trace() as tl:
                acc = o.analysis(g, a_in, ws[l + 1])
                torch.cuda.synchronize()
            _pin_dense(pins, T, tl, 2)
            tag = f"{side}{l}"
            if side == "x" or l == 5:                          # the model check (once per layer and on the diff layer's input)
                T.bound(f"{tag}.plain{ci}-{co}", acc, R.dense_form(a_in.cpu(), sd[f"{PR.CONVS[l + 1]}.weight"]))
            act = torch.maximum(acc + bs[l + 1].reshape(1, -1, 1, 1), zero)       # max(acc + bias, 0) in fp32
            if codes[l]:
                pooled, code = R.pool_first_max(act.cpu())
                T.count(f"{tag}.pool.bits", int((_bits(s[names_out[l]].cpu()) != _bits(pooled)).sum()))
                T.count(f"{tag}.pool.codes", int((s[codes[l]].cpu() != code).sum()))
                if tied and side == "x":
                    v = act.cpu()[..., :2 * (Hl // 2), :2 * (Wl // 2)].reshape(P, co, Hl // 2, 2, Wl // 2, 2)
                    mx = v.amax(dim=(3, 5), keepdim=True)
                    ties.append(int((((v == mx).sum(dim=(3, 5)) > 1) & (mx.squeeze(5).squeeze(3) > 0)).sum()))
            elif side == "y" or l < 5:
                stored = fy if l == 5 else s[names_out[l]]
                T.count(f"{tag}.bias.bits", int((_bits(stored) != _bits(act)).sum()))
            else:                                              # the diff form: fx itself goes nowhere
                _, sx_, sy_, _ = R.vgg_diff(act, fy)
                T.count("diff.seed_x.bits", int((_bits(ex["seed_x"]) != _bits(sx_)).sum()))
                T.count("diff.seed_y.bits", int((_bits(ex["seed_y"]) != _bits(sy_)).sum()))
    if tied:
        log(f"dcell vgg {case}: tied pool windows at positive values, from the device's pre-pool values: {ties}")
        T.count("no_tied_windows", int(not (len(ties) == 2 and all(k > 0 for k in ties))))
    part = ex["partial"].cpu()
    T.count("partials_unwritten", int(part.isnan().sum()))
    dsum = torch.where(ex["seed_x"] != 0, ex["seed_x"], ex["seed_y"]).double().pow(2).sum().item()
    count = 256.0 * L["px"][2]
    T.count("loss_off", int(not abs(float(loss) * count - dsum) <= 2.0 ** -23 * dsum))
    T.ratios["loss"] = abs(float(loss) * count - dsum) / (2.0 ** -23 * dsum)
    # the backward with dx only: g_a is the 128 -> 64 transposed layer's output, g_b the unpool form's (64 -> 64, level 0)
    g1 = torch.ones((), device="cuda")

    def backward():
        s = scr.clone()
        dx = torch.full((P, H, W), NAN, device="cuda")
        with o.trace() as tb:
            cva._lib.check(lib.cdl_vgg_backward(P, H, W, wt, bt, 3, o._ptr(g1), o._ptr(dx), None, o._ptr(s), n, o._stream()),
                           "cdl_vgg_backward")
            torch.cuda.synchronize()
        return (s, dx), tb
    (sb, dx), (sb2, dx2), tb = _twice(backward)
    sites = launch_sites(tb)
    modes = sorted(r.template().get("MODE") for r in sites.get(K_VGG, []))
    mts = [r.template().get("MT") for r in sites.get(K_DENSE, [])]
    pins.seen.append(("backward", modes, mts))
    if modes != [8, 8] or mts != [2] * 4 or len(sites.get(K_PREP_VGG, [])) != 6:
        pins.failed.append(f"backward: two unpool launches and four plain k_dense<2>: got {modes}, {mts}, {sorted(sites)}")
    T.count("backward.second_call_differs", int((sb.view(torch.int32) != sb2.view(torch.int32)).sum()) + int((_bits(dx) != _bits(dx2)).sum()))
    exb = VS.scratch_extras(sb, P, H, W, 3)
    (H1, W1) = L["dims"][1]
    g_a = exb["g_a"][:64 * L["px"][1]].reshape(P, 64, H1, W1)
    g_b = exb["g_b"][:64 * L["px"][0]].reshape(P, 64, H, W)
    am1 = s0["am1"].cpu()
    placed = R.unpool_place(g_a.cpu(), am1, H, W)
    g = o.Geometry.make(P, 64, 64, (H, W), (3, 3), (1, 1), 1)
    T.count("unpool.bits", int((_bits(g_b) != _bits(o.synthesis(g, placed.cuda(), ws[1]))).sum()))
    T.bound("unpool", g_b, R.vgg_unpool(g_a.cpu(), am1, sd[f"{PR.CONVS[1]}.weight"], H, W))
    T.count("dx_nan", int(dx.isnan().sum()))
    log(f"dcell vgg {case}".ljust(64) + " " + T.line())
    assert T.ok(), (T.counts, T.ratios, T.notes)
    pins.done()


# ================================================================================================ every compiled instance
def test_every_compiled_instance_of_the_file_is_reached(hip_env):
    """The launch sites of cdl_dense_mfma.hip, from the sources, against those the trace of one small call per entry point
    names -- and per site the template arguments seen: k_dense<1>, k_dense<2>, the four k_dense_vgg<MODE>."""
    import cdlnet_video_amd as cva
    o = _ops(hip_env)
    lib = cva._lib.lib()
    seen = collections.defaultdict(set)

    def note(t):
        for sid, recs in launch_sites(t).items():
            for r in recs:
                seen[sid].add(tuple(sorted(r.template().items())))

    for M in (24, 40):                                          # k_dense<1>, k_dense<2>; k_dense_wgrad<false> (W = 33) + fold
        d = residual_data(M)
        g = o.residual_geometry(d["x"], d["w1"])
        with o.trace() as t:
            h, out = o.residual_forward(g, d["x"].cuda(), d["w1"].cuda(), d["w2"].cuda())
            o.residual_backward(g, d["x"].cuda(), h, out, d["w1"].cuda(), d["w2"].cuda(), d["g_out"].cuda())
            torch.cuda.synchronize()
        note(t)
    c = W_BY_ID["wg-Pd1-one-tile-each"]                        # k_dense_wgrad<true>
    dc = wgrad_data(c.id, 72)
    with o.trace() as t:
        o.wgrad(o.Geometry.make(c.N, c.C, c.M, _wsp(c, 72), _wP(c), (1, 1), 1), dc["F"].cuda(), dc["x"].cuda())
        torch.cuda.synchronize()
    note(t)
    P, H, W = 1, 16, 16                                         # the four VGG modes and their prep site
    sd = PR.random_weights(3)
    x, y = _vgg_inputs(P, H, W, False)
    ws, bs = cva.metrics._vgg_tables(sd, torch.device("cuda"))
    n = int(lib.cdl_vgg_scratch_floats(P, H, W, 1))
    scr, loss, dx = torch.zeros(n, device="cuda"), torch.zeros((), device="cuda"), torch.zeros(P, H, W, device="cuda")
    with o.trace() as t:
        cva._lib.check(lib.cdl_vgg_forward(o._ptr(x.cuda()), o._ptr(y.cuda()), P, H, W, o._ptr_table(ws), o._ptr_table(bs), 1, None,
                                           o._ptr(loss), o._ptr(scr), n, o._stream()), "cdl_vgg_forward")
        cva._lib.check(lib.cdl_vgg_backward(P, H, W, o._ptr_table(ws), o._ptr_table(bs), 1, o._ptr(torch.ones((), device="cuda")),
                                            o._ptr(dx), None, o._ptr(scr), n, o._stream()), "cdl_vgg_backward")
        torch.cuda.synchronize()
    note(t)
    import gpu_util
    mod, _ = gpu_util._SITES                                    # tools/launch_coverage.py, loaded by launch_sites
    in_file = sorted(s.id for s in mod.scan_sources() if s.file == "cdl_dense_mfma.hip")
    reached = sorted(k for k in seen if k.startswith(DEN))
    log(f"dcell launch sites of cdl_dense_mfma.hip: {in_file}; reached {[(k, sorted(seen[k])) for k in reached]}")
    assert reached == in_file and len(in_file) == 7, (in_file, reached)
    assert seen[K_DENSE] == {(("MT", 1),), (("MT", 2),)}, seen[K_DENSE]
    assert seen[K_VGG] == {(("MODE", m),) for m in (1, 3, 5, 8)}, seen[K_VGG]
