"""Every rung of the kernel ladder behind the generic entry points, pinned by the launch trace and checked against
float64.

Each case forces a tier with the library's switches, asserts from the trace (cva.ops.trace) which kernel and which
run-time variant of its plan ran, and compares the result with the same operation evaluated in float64 on the CPU
(torch convolutions on .double() inputs; autograd for the filter gradients).  Tolerances, relative to max|ref|:
    split-bf16 matrix-core kernels  2e-5 (4e-5 where the epilogue shrinks, as test_gpu_ops.py)
    fp32 analysis and synthesis     2e-6
    fp32 filter gradients           1e-5
    threshold gradients             2e-5 on the matrix cores (test_gpu_ops.py), 1e-5 in fp32 (cdl_tau_grad's bound there)
Thresholds are positive: below zero the shrinkage jumps by 2|t| at u = 0, where no two evaluations agree.

Several plans read the compute-unit count.  The shapes were chosen against the plan rules at 256 CUs; on another
device the numeric comparison still runs and only the variant assertions are skipped, with that reason.
"""
import functools

import pytest
import torch

from gpu_util import check, launch_sites, log
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

MFMA_TOL, FP32_TOL, FP32_WTOL = 2e-5, 2e-6, 1e-5

ANA, SYN, WGM = "cdl_analysis_mfma.hip:", "cdl_synth_mfma.hip:", "cdl_wgrad_mfma.hip:"
TIL, GEN, DEN = "cdl_generic_tiled.hip:", "cdl_generic.hip:", "cdl_dense_mfma.hip:"
K_ANA = ANA + "k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_WGM = WGM + "k_wgm<PH,PW,SW,NG,CT>"
K_SYN4, K_SYN0 = SYN + "k_synth_m<PH,PW,SW,4>", SYN + "k_synth_m<PH,PW,SW,0>"
K_ASM4, K_ASM1 = SYN + "k_synth_assemble4<PH,PW,SW>", SYN + "k_synth_assemble<PH,PW,SW>"
K_ANA_T = TIL + "k_analysis_t<PW,SW,MAP>"
K_SYN_T, K_SYN_Q = TIL + "k_synthesis_t<PW,SW,CC,MCHS>", TIL + "k_synthesis_q<PW,SW,CC>"
K_FOLD_T, K_FOLD_Q = TIL + "k_synth_fold", TIL + "k_synth_fold#2"
K_WL, K_WP, K_WT = TIL + "k_wgrad_l<PH_,PW_,SW_>", TIL + "k_wgrad_p<PH_,PW_,SW_>", TIL + "k_wgrad_t<PW_,SW_>"

ENV = {
    "mfma": {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"},
    "tiled": {"CDL_MFMA_ANALYSIS": "0", "CDL_MFMA_SYNTHESIS": "0", "CDL_MFMA_WGRAD": "0", "CDL_MFMA_DENSE": "0"},
    "nopipe": {"CDL_MFMA_ANALYSIS": "0", "CDL_MFMA_SYNTHESIS": "0", "CDL_MFMA_WGRAD": "0", "CDL_MFMA_DENSE": "0",
               "CDL_NO_PIPELINED_SYNTHESIS": "1"},
    "plain": {"CDL_NO_TILED": "1"},
    "scalar": {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1",
               "CDL_SCALAR_ASSEMBLE": "1"},
}


def ops():
    import cdlnet_video_amd as cva
    return cva.ops


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def data(N, C, M, sp, P, s):
    """Seeded inputs of one geometry and its float64 references, computed once and shared by the tiers (read-only)."""
    g = torch.Generator().manual_seed(20)
    x = torch.randn((N, C) + sp, generator=g)
    zsp = tuple(d // s for d in sp)
    z = torch.randn((N, M) + zsp, generator=g)
    z = z * (torch.rand(z.shape, generator=g) < 0.3)          # sparse code with exact zeros
    w = torch.randn((M, C) + P, generator=g) * 0.2
    u = torch.randn(z.shape, generator=g)
    tau = torch.rand(N, M, generator=g) * 0.5 + 0.01
    c = torch.rand(N, generator=g)
    mask = (torch.rand(x.shape, generator=g) < 0.4).float()
    return {"x": x, "z": z, "w": w, "u": u, "tau": tau, "c": c, "mask": mask, "pad": tuple(p // 2 for p in P)}


@functools.lru_cache(maxsize=None)
def ref_analysis(key):
    d = data(*key)
    return O.analysis(d["x"].double(), d["w"].double(), key[5], d["pad"])


@functools.lru_cache(maxsize=None)
def ref_synthesis(key, gated):
    d = data(*key)
    z = d["u"].double() * (d["z"] != 0) if gated else d["z"].double()
    return O.synthesis(z, d["w"].double(), key[5], d["pad"])


@functools.lru_cache(maxsize=None)
def ref_wgrad(key, gated):
    """d/dw <A(x; w), F> in float64 by autograd: F = u on the support of z (gated) or z itself."""
    d = data(*key)
    w = d["w"].double().requires_grad_(True)
    F = d["u"].double() * (d["z"] != 0) if gated else d["z"].double()
    (O.analysis(d["x"].double(), w, key[5], d["pad"]) * F).sum().backward()
    return w.grad


def setup(hip_env, tier, key):
    for k, v in ENV[tier].items():
        hip_env(k, v)
    N, C, M, sp, P, s = key
    d = data(*key)
    return ops(), ops().Geometry.make(N, C, M, sp, P, d["pad"], s), d


class Pins:
    """Variant assertions of one test, held back until its numeric comparisons have run."""

    def __init__(self, tag):
        self.tag, self.failed, self.seen = tag, [], []

    def add(self, trace, site, forbid=(), **want):
        """A record of launch site `site` whose template arguments and note values include `want`; none of `forbid`."""
        sites = launch_sites(trace)
        self.seen.append(sorted(sites))
        recs = sites.get(site, [])
        ok = [r for r in recs if all({**r.values(), **r.template()}.get(k) == v for k, v in want.items())]
        if not ok:
            self.failed.append(f"{site} {want}: got {[(r.template(), r.note) for r in recs] or sorted(sites)}")
        for f in forbid:
            if any(k.startswith(f) for k in sites):
                self.failed.append(f"{f}* must not run: {sorted(sites)}")

    def done(self):
        log(f"{self.tag:60s} launch sites {self.seen}")
        if cu_count() != 256 and self.failed:
            pytest.skip(f"variant assertions hold for 256 compute units, this device has {cu_count()}: {self.failed}")
        assert not self.failed, self.failed


# ---------------------------------------------------------------------------------------------------- analysis
def run_analysis(hip_env, tier, key, tol, site, forbid=(), rev_site=None, **want):
    """plain, first and iteration with thresholds, gated, and the reverse step with its threshold gradients."""
    o, geom, d = setup(hip_env, tier, key)
    N, C, M, sp, P, s = key
    tag = f"dispatch analysis[{tier}] N{N}C{C}M{M}{sp}P{P}s{s}"
    pins = Pins(tag)
    ref = ref_analysis(key)
    xd, wd, zd, ud, td = (d[k].cuda() for k in ("x", "w", "z", "u", "tau"))
    z64, u64 = d["z"].double(), d["u"].double()
    tb = d["tau"].double().reshape((N, M) + (1,) * len(sp))
    shrink_tol = 2 * tol if tol == MFMA_TOL else tol
    with o.trace() as t:
        got = o.analysis(geom, xd, wd)
    check(tag + " plain", got, ref, tol)
    pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.analysis(geom, xd, wd, 1.0, None, None, td)
    check(tag + " first", got, O.soft_threshold(ref, tb), shrink_tol)
    pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.analysis(geom, xd, wd, -1.0, zd, None, td)
    check(tag + " iter", got, O.soft_threshold(z64 - ref, tb), shrink_tol)
    pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.analysis(geom, xd, wd, 1.0, ud, zd, None)
    check(tag + " gated", got, u64 * (d["z"] != 0) + ref, tol)
    pins.add(t, site, forbid, **want)
    # reverse step: out = [z != 0] (u + 0.5 A x) and the threshold gradients of `out`
    dt = torch.zeros(2, M, device="cuda")
    with o.trace() as t:
        got = o.analysis_rev(geom, xd, wd, 0.5, ud, zd, d["c"].cuda(), dt)
    want_rev = (u64 + 0.5 * ref) * (d["z"] != 0)
    check(tag + " rev out", got, want_rev, tol)
    assert bool((got[(d["z"] == 0).cuda()] == 0).all())
    s_nm = -(torch.sign(z64) * want_rev).sum(dim=tuple(range(2, z64.dim())))
    dtol = 2e-5 if tol == MFMA_TOL else 1e-5
    check(tag + " rev dt0", dt[0], s_nm.sum(0), dtol)
    check(tag + " rev dt1", dt[1], (d["c"].double()[:, None] * s_nm).sum(0), dtol)
    if rev_site == "fused":                                   # the gate and the partials ride in the matrix-core epilogue
        pins.add(t, site, forbid, **{**want, "REV": True})
        pins.add(t, ANA + "k_ana_tau_final<false>")
    else:                                                     # composed: the analysis, then the gate + threshold pass
        pins.add(t, site, forbid, **want)
        pins.add(t, GEN + "k_tau_partial<true,false>")
    pins.done()


# shapes on the plan thresholds at 256 CUs: (key, expected template arguments and plan values of k_ana_m)
MFMA_ANALYSIS = [
    # MT = 1, 16 x 8 x 1 = 128 workgroups of 4 tiles
    ((16, 1, 8, (60, 121), (5, 5), 1), dict(PH=5, PW=5, SW=1, MT=1, MTW=1, tpw=4, wgs=128)),
    # two channel tiles per workgroup
    ((16, 1, 64, (60, 121), (7, 7), 1), dict(PH=7, SW=1, MT=2, MTW=2, tpw=4, wgs=128)),
    # three channel tiles on a single frame: one tile per workgroup, channel groups on grid.y (32 x 2 workgroups)
    ((1, 1, 72, (60, 121), (7, 7), 1), dict(MT=2, tpw=1, ngy=2, wgs=64)),
    ((1, 1, 169, (120, 242), (7, 7), 2), dict(SW=2, MT=2, tpw=1, ngy=3, wgs=96)),
    ((16, 3, 16, (60, 121), (7, 7), 1), dict(MT=1, tpw=4, wgs=128)),
    ((6, 1, 16, (6, 30, 121), (5, 5, 5), 1), dict(PH=5, MT=1, tpw=4, wgs=144)),
    # exactly the 96-workgroup minimum: 4 x 6 x 4 x 1
    ((4, 1, 16, (6, 30, 61), (3, 5, 5), 1), dict(PH=5, MT=1, tpw=4, wgs=96)),
    ((16, 1, 16, (120, 242), (9, 9), 2), dict(PH=9, PW=9, SW=2, MT=1, wgs=128)),
    # 405 taps over 9 planes: one channel tile per workgroup behind more than 96 KB of LDS
    ((6, 1, 40, (8, 32, 72), (9, 9, 5), 2), dict(PH=9, PW=5, SW=2, MT=1, MTW=1, lds_over_96k=1)),
]


@pytest.mark.parametrize("key,want", MFMA_ANALYSIS)
def test_analysis_matrix_core_variants(key, want, hip_env):
    run_analysis(hip_env, "mfma", key, MFMA_TOL, K_ANA, rev_site="fused", **want)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("key", [MFMA_ANALYSIS[0][0], MFMA_ANALYSIS[1][0]])
def test_analysis_matrix_core_prox_epilogue(key, both, hip_env):
    """k_ana_m<.., PROX = true>: the CSR maps as the matrix-core analysis' epilogue.  The CSR tests run shapes below
    the 96-workgroup minimum, so nothing else reaches it.  u_out against float64; z is the element-wise map of u_out
    (cdl_prox_csr, pinned to the oracle by test_gpu_csr.py), bit for bit; the one-neighbour map, continuous for
    positive thresholds, against float64 as well."""
    o, geom, d = setup(hip_env, "mfma", key)
    N, C, M, sp, P, s = key
    tag = f"dispatch analysis_prox[{'f2' if both else 'f1'}] N{N}C{C}M{M}{sp}P{P}s{s}"
    gen = torch.Generator().manual_seed(21)
    code = lambda: 0.3 * torch.randn(d["z"].shape, generator=gen) * (torch.rand(d["z"].shape, generator=gen) > 0.5)
    zp, za = code(), code()
    lam, g1, g2 = (torch.rand(N, M, generator=gen) * sc + 0.01 for sc in (0.2, 1.2, 1.2))
    dev = lambda t: t.cuda() if both or t is not za and t is not g2 else None
    u_out = torch.empty(d["z"].shape, device="cuda")
    with o.trace() as t:
        z = o.analysis_prox(geom, d["x"].cuda(), d["w"].cuda(), -1.0, d["z"].cuda(), zp.cuda(), lam.cuda(), g1.cuda(),
                            dev(za), dev(g2), u_out=u_out)
    u64 = d["z"].double() - ref_analysis(key)
    check(tag + " u", u_out, u64, MFMA_TOL)
    assert torch.equal(z, o.prox_csr(geom, u_out, zp.cuda(), lam.cuda(), g1.cuda(), dev(za), dev(g2)))
    if not both:
        bc = lambda v: v.double().reshape((N, M) + (1,) * len(sp))
        check(tag + " z", z, O.prox_csr(u64, zp.double(), bc(lam), bc(g1)), 2 * MFMA_TOL)
    pins = Pins(tag)
    pins.add(t, K_ANA, (TIL, DEN), PROX=True, REV=False, MT=1 if M <= 32 else 2)
    pins.done()


def test_analysis_below_the_workgroup_minimum_falls_to_the_tiled_tier(hip_env):
    """One sample fewer than the 96-workgroup case: 72 workgroups, the matrix-core plan declines."""
    run_analysis(hip_env, "mfma", (3, 1, 16, (6, 30, 61), (3, 5, 5), 1), FP32_TOL, K_ANA_T, forbid=(ANA,), PW=5, SW=1)


@pytest.mark.parametrize("key,want", [
    ((16, 1, 8, (60, 121), (5, 5), 1), dict(PW=5, SW=1, MAP=False, chunks=1)),
    # 8 workgroups per channel slice: the 9 groups of 8 channels spread over blockIdx.z
    ((1, 1, 72, (60, 121), (7, 7), 1), dict(PW=7, SW=1, chunks=9)),
    ((4, 1, 16, (6, 30, 61), (3, 5, 5), 1), dict(PW=5, SW=1, chunks=2)),
    ((2, 3, 9, (18, 22), (7, 7), 2), dict(PW=7, SW=2, chunks=2)),
    ((2, 1, 8, (20, 24), (5, 3), 1), dict(PW=3, SW=1, chunks=1)),
])
def test_analysis_tiled_tier(key, want, hip_env):
    run_analysis(hip_env, "tiled", key, FP32_TOL, K_ANA_T, forbid=(ANA, DEN), **want)


@pytest.mark.parametrize("key", [(2, 1, 8, (20, 24), (5, 5), 1), (2, 3, 9, (18, 22), (7, 7), 2),
                                 (1, 1, 6, (8, 16, 16), (5, 5, 5), 1)])
def test_analysis_plain_kernels(key, hip_env):
    """CDL_NO_TILED: the plain kernels of cdl_generic.hip on ordinary shapes."""
    run_analysis(hip_env, "plain", key, FP32_TOL, GEN + "k_analysis<false>", forbid=(ANA, DEN, TIL))


# --------------------------------------------------------------------------------------------------- synthesis
def run_synthesis(hip_env, tier, key, tol, expect, forbid=()):
    """plain, masked residual, gated.  expect: [(site, {values})]"""
    o, geom, d = setup(hip_env, tier, key)
    N, C, M, sp, P, s = key
    tag = f"dispatch synthesis[{tier}] N{N}C{C}M{M}{sp}P{P}s{s}"
    pins = Pins(tag)
    ref = ref_synthesis(key, False)
    assert ref.shape == d["x"].shape
    zd, wd, ud, md, xd = (d[k].cuda() for k in ("z", "w", "u", "mask", "x"))
    m64, x64 = d["mask"].double(), d["x"].double()
    with o.trace() as t:
        got = o.synthesis(geom, zd, wd)
    check(tag + " plain", got, ref, tol)
    for site, want in expect:
        pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.synthesis(geom, zd, wd, 1.0, None, md, xd)
    check(tag + " resid", got, m64 * ref - x64, tol)
    for site, want in expect:
        pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.synthesis(geom, ud, wd, -1.0, zd, md, None)
    check(tag + " gated", got, -m64 * ref_synthesis(key, True), tol)
    for site, want in expect:
        pins.add(t, site, forbid, **want)
    pins.done()


@pytest.mark.parametrize("tier,key,expect", [
    # one (c, kd) group: fragments through LDS only; W % 4 = 1: the scalar assemble
    ("mfma", (16, 1, 8, (60, 121), (5, 5), 1), [(K_SYN0, dict(PH=5, SW=1, streamed=0, gy=1)), (K_ASM1, {})]),
    # three groups share the code values: fragments in registers
    ("mfma", (16, 3, 16, (60, 121), (7, 7), 1), [(K_SYN4, dict(PH=7, streamed=0, gy=1)), (K_ASM1, {})]),
    # 48 tiles on 256 CUs: the three depth groups spread over grid.y
    ("mfma", (1, 1, 16, (6, 30, 61), (3, 5, 5), 1), [(K_SYN4, dict(PH=5, streamed=0, gy=3))]),
    # 9 x 9, M = 169: 165 KB of fragments do not fit, k-steps stream through LDS in chunks; W % 4 = 0: vector assemble
    ("mfma", (2, 1, 169, (68, 132), (9, 9), 2), [(K_SYN0, dict(PH=9, SW=2, streamed=1)), (K_ASM4, {})]),
    ("scalar", (2, 1, 169, (68, 132), (9, 9), 2), [(K_SYN0, dict(streamed=1)), (K_ASM1, {})]),
    ("mfma", (6, 1, 40, (8, 32, 72), (9, 9, 5), 2), [(K_SYN4, dict(PH=9, PW=5, SW=2)), (K_ASM4, {})]),
])
def test_synthesis_matrix_core_variants(tier, key, expect, hip_env):
    run_synthesis(hip_env, tier, key, MFMA_TOL, expect, forbid=(TIL, DEN))


@pytest.mark.parametrize("tier,key,expect", [
    # 2-D, C = 1: eight channels per LDS round; M = 8: one channel slice, no fold
    ("tiled", (16, 1, 8, (60, 121), (5, 5), 1), [(K_SYN_T, dict(PW=5, SW=1, CC=1, MCHS=8, chunks=1))]),
    # 8 workgroups: the channels split over blockIdx.z, partial images folded
    ("tiled", (1, 1, 72, (60, 121), (7, 7), 1), [(K_SYN_T, dict(MCHS=8, chunks=9)), (K_FOLD_T, {})]),
    # C = 3 and 3-D: the pipelined kernel, with and without the fold
    # (image tiles of 64 x 16 pixels: 128 workgroups, so the two groups of 8 channels split; 8 channels do not)
    ("tiled", (16, 3, 16, (60, 121), (7, 7), 1), [(K_SYN_Q, dict(PW=7, CC=3, chunks=2)), (K_FOLD_Q, {})]),
    ("tiled", (2, 3, 8, (20, 24), (5, 5), 1), [(K_SYN_Q, dict(PW=5, CC=3, chunks=1))]),
    ("tiled", (1, 1, 16, (6, 30, 61), (3, 5, 5), 1), [(K_SYN_Q, dict(PW=5, CC=1, chunks=2)), (K_FOLD_Q, {})]),
    ("tiled", (2, 3, 9, (18, 22), (7, 7), 2), [(K_SYN_Q, dict(PW=7, SW=2, CC=3))]),
    # CDL_NO_PIPELINED_SYNTHESIS: two channels per round in 3-D, eight in 2-D
    ("nopipe", (1, 1, 16, (6, 30, 61), (3, 5, 5), 1), [(K_SYN_T, dict(MCHS=2, chunks=2)), (K_FOLD_T, {})]),
    ("nopipe", (16, 3, 16, (60, 121), (7, 7), 1), [(K_SYN_T, dict(CC=3, MCHS=8, chunks=2)), (K_FOLD_T, {})]),
    ("nopipe", (2, 3, 8, (20, 24), (5, 5), 1), [(K_SYN_T, dict(CC=3, MCHS=8, chunks=1))]),
    ("tiled", (2, 1, 8, (20, 24), (5, 3), 1), [(K_SYN_T, dict(PW=3, SW=1, MCHS=8))]),
])
def test_synthesis_tiled_tier(tier, key, expect, hip_env):
    forbid = (SYN, DEN) + ((K_SYN_Q,) if tier == "nopipe" else ())
    run_synthesis(hip_env, tier, key, FP32_TOL, expect, forbid=forbid)


@pytest.mark.parametrize("key", [(2, 1, 8, (20, 24), (5, 5), 1), (2, 3, 9, (18, 22), (7, 7), 2),
                                 (1, 1, 6, (8, 16, 16), (5, 5, 5), 1)])
def test_synthesis_plain_kernels(key, hip_env):
    run_synthesis(hip_env, "plain", key, FP32_TOL, [(GEN + "k_synthesis", {})], forbid=(SYN, DEN, TIL))


# -------------------------------------------------------------------------------------------- filter gradients
def run_wgrad(hip_env, tier, key, tol, expect, forbid=(), pair_expect=None):
    """plain (alpha * z (x) x), gated (u on the support of z), and the two as one paired call."""
    o, geom, d = setup(hip_env, tier, key)
    N, C, M, sp, P, s = key
    tag = f"dispatch wgrad[{tier}] N{N}C{C}M{M}{sp}P{P}s{s}"
    pins = Pins(tag)
    xd, zd, ud = (d[k].cuda() for k in ("x", "z", "u"))
    with o.trace() as t:
        got = o.wgrad(geom, zd, xd, -2.0)
    check(tag + " plain", got, -2.0 * ref_wgrad(key, False), tol)
    for site, want in expect:
        pins.add(t, site, forbid, **want)
    with o.trace() as t:
        got = o.wgrad(geom, ud, xd, 1.0, gate=zd)
    check(tag + " gated", got, ref_wgrad(key, True), tol)
    for site, want in expect:
        pins.add(t, site, forbid, **want)
    ug = (d["u"] * (d["z"] != 0)).cuda()
    with o.trace() as t:
        d0, d1 = o.wgrad_pair(geom, ug, xd, 1.0, zd, xd, -2.0)
    check(tag + " pair[0]", d0, ref_wgrad(key, True), tol)
    check(tag + " pair[1]", d1, -2.0 * ref_wgrad(key, False), tol)
    for site, want in (expect if pair_expect is None else pair_expect):
        pins.add(t, site, forbid, **want)
    pins.done()


def wgm(pair=None, **want):
    single = [(K_WGM, dict(pair=0, rsc=0, **want)), (WGM + "k_wgm_fold", {})]
    both = [(K_WGM, dict(rsc=0, **{**want, **(pair or {}), "pair": 1})), (WGM + "k_wgm_fold", {})]
    return single, both


@pytest.mark.parametrize("key,want,pair", [
    # exactly the 64-tile minimum
    ((16, 1, 8, (60, 121), (5, 5), 1), dict(PH=5, SW=1, NG=1, CT=1, rs=1, gz=1, tpw=1, tiles=64), None),
    # three channel tiles: two per wave; 4 tiles spread by 4 row parts each
    ((1, 1, 72, (60, 121), (7, 7), 1), dict(PH=7, NG=1, CT=2, rs=4, tiles=4), None),
    ((1, 1, 169, (120, 242), (7, 7), 2), dict(SW=2, NG=1, CT=2, rs=8, tiles=4), None),
    # three (c) groups at exactly 64 tiles: one group per pass; one sample more: three
    ((16, 3, 16, (60, 121), (7, 7), 1), dict(NG=1, CT=1, tiles=64), None),
    ((17, 3, 16, (60, 121), (7, 7), 1), dict(NG=3, CT=1, tiles=68), None),
    ((6, 1, 16, (6, 30, 121), (5, 5, 5), 1), dict(PH=5, NG=5, CT=1, tiles=72), None),
    # the deep 9 x 9 x 5 filter: 24 tiles, the three group passes spread over blockIdx.z
    ((6, 1, 40, (8, 32, 72), (9, 9, 5), 2), dict(PH=9, PW=5, SW=2, NG=3, CT=1, gz=3, tiles=24), dict(gz=3)),
    # 130 tiles: the paired launch has 260 work items for 256 CUs, two per workgroup
    ((130, 1, 8, (32, 64), (5, 5), 1), dict(NG=1, CT=1, tpw=1, tiles=130), dict(tpw=2)),
])
def test_wgrad_matrix_core_variants(key, want, pair, hip_env):
    single, both = wgm(pair, **want)
    run_wgrad(hip_env, "mfma", key, MFMA_TOL, single, forbid=(TIL, DEN), pair_expect=both)


def test_wgrad_below_the_tile_minimum_falls_to_the_tiled_tier(hip_env):
    """One sample fewer than the 64-tile case: 60 tiles, the matrix-core plan declines."""
    run_wgrad(hip_env, "mfma", (15, 1, 8, (60, 121), (5, 5), 1), FP32_WTOL, [(K_WP, {})], forbid=(WGM,))


@pytest.mark.parametrize("tier,key,expect", [
    # 64 tiles x 1 group < 128 workgroups: filter planes in registers, code rows in chunks
    ("tiled", (16, 1, 8, (60, 121), (5, 5), 1), [(K_WP, {}), (TIL + "k_wgrad_fold", {})]),
    # 64 tiles x 3 groups: the LDS-tiled kernel
    ("tiled", (16, 3, 16, (60, 121), (7, 7), 1), [(K_WL, dict(tiles=64)), (TIL + "k_wgrad_tfold", {})]),
    ("tiled", (2, 3, 9, (18, 22), (7, 7), 2), [(K_WP, {})]),
    ("tiled", (1, 1, 16, (6, 30, 61), (3, 5, 5), 1), [(K_WP, {})]),
    # a 5 x 3 plane has neither an LDS-tiled nor a register-plane instantiation: the per-filter-row kernel, in
    # the default configuration too (the matrix-core plan takes square planes and 9 x 5 only)
    ("tiled", (2, 1, 8, (20, 24), (5, 3), 1), [(K_WT, {})]),
    ("mfma", (2, 1, 8, (20, 24), (5, 3), 1), [(K_WT, {})]),
    ("tiled", (2, 3, 6, (24, 20), (5, 3), 2), [(K_WT, {})]),
])
def test_wgrad_tiled_tier(tier, key, expect, hip_env):
    run_wgrad(hip_env, tier, key, FP32_WTOL, expect, forbid=(WGM, DEN))


@pytest.mark.parametrize("key", [(2, 1, 8, (20, 24), (5, 5), 1), (2, 3, 9, (18, 22), (7, 7), 2),
                                 (1, 1, 6, (8, 16, 16), (5, 5, 5), 1)])
def test_wgrad_plain_kernels(key, hip_env):
    run_wgrad(hip_env, "plain", key, FP32_WTOL, [(GEN + "k_wgrad", {})], forbid=(WGM, DEN, TIL))


# -------------------------------------------------------------------------------------------------- dense tier
# many channels on both sides, unit stride (test_gpu_ops.py SHAPES), W % 4 in {1, 2} and, added here, 0
DENSE = [
    ((2, 16, 32, (3, 17, 33), (3, 3, 3), 1), 1, False),
    ((1, 24, 40, (20, 45), (3, 3), 1), 2, False),
    ((1, 24, 40, (20, 44), (3, 3), 1), 2, True),
    ((1, 20, 70, (2, 9, 34), (1, 5, 5), 1), 2, None),        # (5 x 5: the dense filter gradient takes 3 x 3 only)
]


@pytest.mark.parametrize("key,mt,vec", DENSE)
def test_dense_tier_analysis(key, mt, vec, hip_env):
    """cdl_dense_mfma.hip in the analysis role, MT channel tiles per workgroup; the reverse step composes it with the
    gate + threshold pass."""
    run_analysis(hip_env, "mfma", key, MFMA_TOL, DEN + "k_dense<MT>", forbid=(ANA, TIL), MT=mt)


@pytest.mark.parametrize("key,mt,vec", DENSE)
def test_dense_tier_synthesis(key, mt, vec, hip_env):
    run_synthesis(hip_env, "mfma", key, MFMA_TOL, [(DEN + "k_dense<MT>", dict(MT=1))], forbid=(SYN, TIL))


@pytest.mark.parametrize("key,mt,vec", DENSE[:3])
def test_dense_tier_wgrad(key, mt, vec, hip_env):
    """3 x 3 planes only; vector loads when W % 4 == 0."""
    site = DEN + ("k_dense_wgrad<true>" if vec else "k_dense_wgrad<false>")
    run_wgrad(hip_env, "mfma", key, MFMA_TOL, [(site, {}), (DEN + "k_dense_wfold", {})], forbid=(WGM, TIL))


def test_dense_switch_off_leaves_the_dense_tier(hip_env):
    key = DENSE[1][0]
    for k, v in ENV["mfma"].items():
        hip_env(k, v)
    hip_env("CDL_MFMA_DENSE", "0")
    o, geom, d = ops(), None, data(*key)
    geom = o.Geometry.make(*key[:5], d["pad"], key[5])
    with o.trace() as t:
        got = o.analysis(geom, d["x"].cuda(), d["w"].cuda())
    check("dispatch dense off analysis", got, ref_analysis(key), MFMA_TOL)
    assert DEN[:-1] not in t.files(), sorted(launch_sites(t))
