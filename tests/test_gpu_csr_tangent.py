"""The tangent of the CSR nets on the GPU: the pointwise tangent of the two proximal maps, the analysis
entry point that applies it, the tangent sweep and its reverse, `jvp_recurrent` and the clip training steps -- against the
reference's own forward-mode derivatives (fixtures c5..c9, tools/make_golden_csr_tangent.py) and against the float64
restatement evaluated at the DEVICE's gates (tests/csr_tangent_restate.py)."""
import functools
import os

import pytest
import torch

import csr_tangent_restate as R
from gpu_util import check, launch_sites, load_golden, log
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

SPLIT_TOL, FP32_TOL = 5e-5, 1e-5          # the project's identical-support tolerances (split-bf16 tier, fp32 tier)
XTOL, GTOL = 1e-5, 2e-4                   # nets against the reference's fixtures (tests/test_gpu_csr.py)


def ops():
    import cdlnet_video_amd as cva
    return cva.ops


def build(g, cls_name):
    import cdlnet_video_amd as cva
    K, M, P, s, C = g["hyper"]
    net = getattr(cva, cls_name)(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=True, init=False)
    net.load_state_dict(g["sd"])
    return net.cuda()


def dev(v):
    return v.cuda() if torch.is_tensor(v) else v


def opt(v):
    return v.cuda() if v is not None else None


# ---------------------------------------------------------------------------------- pointwise tangent
def test_pointwise_tangent_vs_reference_grid():
    """c5: torch.func.jvp of the reference's maps on the c0 grid (exact zeros, ties, negative thresholds)."""
    o = ops()
    g = load_golden("c5_csr_tangent_pointwise")
    n = g["u"].numel()
    shape = (1, 1, n, 1)
    geom = o.Geometry.make(1, 1, 1, (n, 1), (1, 1), (0, 0), 1)
    u, zp, za, ud, zpd, zad = (g[k].reshape(shape).cuda() for k in ("u", "zp", "za", "ud", "zpd", "zad"))
    row = lambda v: torch.full((1, 1), v, device="cuda")
    for i, (lam, g1, g2) in enumerate(g["cases"].reshape(-1, 3).tolist()):
        got = {"jvp_csr": o.prox_csr_tangent(geom, ud, u, zp, row(lam), row(g1), zd_prev=zpd),
               "jvp_csr_u": o.prox_csr_tangent(geom, ud, u, zp, row(lam), row(g1)),
               "jvp_csr_f2": o.prox_csr_tangent(geom, ud, u, zp, row(lam), row(g1), za, row(g2), zpd, zad),
               "jvp_csr_f2_u": o.prox_csr_tangent(geom, ud, u, zp, row(lam), row(g1), za, row(g2))}
        for name, val in got.items():
            ref = g[name][i]
            err = float((val.cpu().reshape(-1) - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            log(f"c5 {name} case {i:<44d} err={err:.3e} tol=1.0e-06")
            assert err <= 1e-6, f"{name} case {i}: {err:.2e}"


def pointwise_case(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    N, M = shape[:2]
    sparse = lambda: 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
    u, zp, za = 0.05 * torch.randn(shape, generator=gen), sparse(), sparse()
    ud, zpd, zad = (torch.randn(shape, generator=gen) for _ in range(3))
    lam = (torch.rand(N, M, generator=gen) - 0.15) * 0.1
    lam.view(-1)[0] = -0.004                                       # at least one negative row: the maps' discontinuous regime
    g1, g2 = (torch.rand(N, M, generator=gen) * 1.2 for _ in range(2))
    return u, zp, za, ud, zpd, zad, lam, g1, g2


@pytest.mark.parametrize("tangents", [False, True])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 9, 13), (1, 3, 4, 20, 24)])
def test_pointwise_tangent_equals_the_restatement_bit_for_bit(shape, both, tangents):
    """The gates are decisions on float32 intermediates: the restatement takes them on the CPU from the same numbers, term
    by term in the reference's order, and the tangent is then a select of the inputs -- every bit must agree."""
    o = ops()
    u, zp, za, ud, zpd, zad, lam, g1, g2 = pointwise_case(shape, sum(shape) + 2 * both + tangents)
    N, M = shape[:2]
    sp = shape[2:]
    bc = lambda t: t.reshape((N, M) + (1,) * len(sp))
    G = R.gates(u, zp, za if both else None, bc(lam), bc(g1), bc(g2) if both else None)
    for gate in G:                                                  # every gate takes both values
        assert 0.02 < float(gate.float().mean()) < 0.998
    ref = R.prox_tangent(G, ud.double(), zpd.double() if tangents else None, zad.double() if tangents and both else None)
    geom = o.Geometry.make(N, 1, M, sp, (1,) * len(sp), (0,) * len(sp), 1)
    args = (geom, None, u.cuda(), zp.cuda(), lam.cuda(), g1.cuda(), za.cuda() if both else None, g2.cuda() if both else None,
            zpd.cuda() if tangents else None, zad.cuda() if tangents and both else None)
    got = o.prox_csr_tangent(args[0], ud.cuda(), *args[2:])
    assert torch.equal(got.cpu(), ref.float())
    buf = ud.cuda().clone()                                        # out may alias ud
    assert o.prox_csr_tangent(args[0], buf, *args[2:], out=buf) is buf and torch.equal(buf, got)


def test_a_nan_in_a_dead_branch_does_not_leak():
    """Selects, not products with 0 / 1: a NaN tangent behind a closed gate stays there."""
    o = ops()
    shape = (2, 5, 9, 13)
    u, zp, za, ud, zpd, zad, lam, g1, g2 = pointwise_case(shape, 5)
    bc = lambda t: t.reshape(2, 5, 1, 1)
    Ga, Gb, Gm = R.gates(u, zp, za, bc(lam), bc(g1), bc(g2))
    ud = torch.where(Gm & Gb & Ga, ud, torch.full_like(ud, float("nan")))      # read only where all three gates are open
    zad = torch.where(Gm & ~Gb, zad, torch.full_like(zad, float("nan")))
    geom = o.Geometry.make(2, 1, 5, (9, 13), (1, 1), (0, 0), 1)
    got = o.prox_csr_tangent(geom, ud.cuda(), u.cuda(), zp.cuda(), lam.cuda(), g1.cuda(), za.cuda(), g2.cuda(), None, zad.cuda())
    assert not bool(torch.isnan(got).any())
    G1 = R.gates(u, zp, None, bc(lam), bc(g1))
    ud1 = torch.where(G1[1] & G1[0], torch.ones_like(u), torch.full_like(u, float("nan")))
    zpd1 = torch.where(G1[1] & ~G1[0], zpd, torch.full_like(zpd, float("nan")))
    got1 = o.prox_csr_tangent(geom, ud1.cuda(), u.cuda(), zp.cuda(), lam.cuda(), g1.cuda(), zd_prev=zpd1.cuda())
    assert not bool(torch.isnan(got1).any())


# ---------------------------------------------------------------------------------- the analysis epilogue
def epilogue_case(geom, seed):
    gen = torch.Generator().manual_seed(seed)
    N, M = geom.N, geom.M
    x = torch.randn(geom.image_shape(), generator=gen).cuda()
    w = (0.1 * torch.randn(geom.filter_shape(), generator=gen)).cuda()
    code = lambda: (0.3 * torch.randn(geom.code_shape(), generator=gen)
                    * (torch.rand(geom.code_shape(), generator=gen) > 0.5)).cuda()
    dense = lambda: torch.randn(geom.code_shape(), generator=gen).cuda()
    zin, zp, za = code(), code(), code()
    u, zpd, zad = 0.6 * dense(), dense(), dense()
    lam, g1, g2 = ((torch.rand(N, M, generator=gen) * sc).cuda() for sc in (0.2, 1.2, 1.2))
    return x, w, zin, u, zp, za, zpd, zad, lam, g1, g2


def epilogue_equals_two_calls(o, geom, both, seed):
    x, w, zin, u, zp, za, zpd, zad, lam, g1, g2 = epilogue_case(geom, seed)
    za, g2, zad = (za, g2, zad) if both else (None, None, None)
    ud = o.analysis(geom, x, w, -1.0, zin, None, None)
    for tp, ta in ((zpd, zad), (None, None)):
        ref = o.prox_csr_tangent(geom, ud, u, zp, lam, g1, za, g2, tp, ta)
        got = o.analysis_prox_tangent(geom, x, w, -1.0, zin, u, zp, lam, g1, za, g2, tp, ta)
        assert torch.equal(got, ref)
        assert 0.02 < float((ref != 0).float().mean()) < 0.98
    first = o.analysis_prox_tangent(geom, x, w, 1.0, None, u, zp, lam, g1, za, g2, zpd, zad)      # iteration 0: no zin
    assert torch.equal(first, o.prox_csr_tangent(geom, o.analysis(geom, x, w, 1.0), u, zp, lam, g1, za, g2, zpd, zad))


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("dims,P,s,C,M", [((24, 40), (5, 5), 1, 1, 11), ((22, 18), (7, 7), 2, 3, 9),
                                           ((4, 12, 16), (3, 5, 5), 1, 1, 6), ((20, 26), (11, 11), 1, 1, 5)])
def test_analysis_prox_tangent_equals_analysis_then_pointwise_tangent(dims, P, s, C, M, both):
    """cdl_analysis_prox_tangent (untiled and tiled kernels) == cdl_analysis then cdl_prox_csr_tangent, bit for bit."""
    o = ops()
    geom = o.Geometry.make(2, C, M, dims, P, tuple(p // 2 for p in P), s)
    epilogue_equals_two_calls(o, geom, both, len(dims) * 7 + P[-1] + both)


MFMA_ENV = {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"}
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_PROX = "cdl_prox.hip:k_prox_fwd"


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("key", [(16, 1, 8, (60, 121), (5, 5), 1), (16, 1, 64, (60, 121), (7, 7), 1)])
def test_analysis_prox_tangent_on_the_matrix_core_analysis(key, both, hip_env):
    """At shapes the matrix-core analysis takes: its plain instance (the CSR epilogue instance stays the primal's alone)
    followed by the pointwise tangent in place, pinned by the launch trace; the bits of the two-call form."""
    for k, v in MFMA_ENV.items():
        hip_env(k, v)
    o = ops()
    N, C, M, sp, P, s = key
    geom = o.Geometry.make(N, C, M, sp, P, tuple(p // 2 for p in P), s)
    x, w, zin, u, zp, za, zpd, zad, lam, g1, g2 = epilogue_case(geom, 31 + both)
    za, g2, zad = (za, g2, zad) if both else (None, None, None)
    ud = o.analysis(geom, x, w, -1.0, zin, None, None)
    with o.trace() as t:
        got = o.analysis_prox_tangent(geom, x, w, -1.0, zin, u, zp, lam, g1, za, g2, zpd, zad)
    assert torch.equal(got, o.prox_csr_tangent(geom, ud, u, zp, lam, g1, za, g2, zpd, zad))
    sites = launch_sites(t)
    recs = sites.get(K_ANA, [])
    assert recs and all(r.template()["PROX"] is False and r.template()["REV"] is False for r in recs), sorted(sites)
    assert len(sites.get(K_PROX, [])) == 1, sorted(sites)
    assert not [k for k in sites if k.startswith(("cdl_generic_tiled.hip:", "cdl_generic.hip:k_analysis"))], sorted(sites)


# ---------------------------------------------------------------------------------- the sweeps
SWEEPS = [((24, 40), (5, 5), 1, 1, 11, False), ((22, 18), (7, 7), 2, 3, 9, True)]


@functools.lru_cache(maxsize=None)
def sweep_case(dims, P, s, C, M, masked):
    """Seeded CPU inputs of one sweep geometry (read-only; shared by the tests below)."""
    o = ops()
    gen = torch.Generator().manual_seed(sum(dims) + M)
    N, K = 2, 3
    geom = o.Geometry.make(N, C, M, dims, P, tuple(p // 2 for p in P), s)
    rnd = lambda shape, sc=1.0: sc * torch.randn(shape, generator=gen)
    d = {"geom": geom, "K": K, "yp": rnd(geom.image_shape()), "vp": rnd(geom.image_shape()),
         "mask": (torch.rand(geom.image_shape(), generator=gen) > 0.3).float() if masked else None,
         "A": [rnd(geom.filter_shape(), 0.08) for _ in range(K)], "B": [rnd(geom.filter_shape(), 0.08) for _ in range(K)],
         "c": torch.rand(N, generator=gen)}
    d["t"], d["g1"], d["g2"] = (torch.rand(K, 2, M, 1, 1, generator=gen) * sc for sc in (0.25, 1.0, 1.0))
    for k in ("zp", "za"):
        d[k] = rnd(geom.code_shape(), 0.5) * (torch.rand(geom.code_shape(), generator=gen) > 0.3)
    for k in ("zdp", "zda", "g_zd"):
        d[k] = rnd(geom.code_shape())
    d["g_xdp"] = rnd(geom.image_shape())
    return d


def on_device(d, both):
    o = ops()
    N = d["geom"].N
    c = d["c"].cuda()
    lam, gam1, gam2 = (o.thresholds(d[k].cuda(), c, N) for k in ("t", "g1", "g2"))
    cu = lambda k: [w.cuda() for w in d[k]] if isinstance(d[k], list) else opt(d[k])
    dd = {k: cu(k) for k in ("yp", "vp", "mask", "A", "B", "zp", "za", "zdp", "zda", "g_zd", "g_xdp")}
    dd.update(lam=lam, gam1=gam1, gam2=gam2 if both else None)
    if not both:
        dd["za"] = dd["zda"] = None
    return dd


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("dims,P,s,C,M,masked", SWEEPS)
def test_csr_tangent_sweeps_equal_stepwise_launches(dims, P, s, C, M, masked, both):
    """cdl_csr_tangent_forward and the reverse sweep (cdl_ista_backward's CSR branch on the tangent's operands) enqueue the
    launches the stepwise Python twins make: every output is bit-identical."""
    from cdlnet_video_amd import loop
    d = sweep_case(dims, P, s, C, M, masked)
    geom, K = d["geom"], d["K"]
    x = on_device(d, both)
    us = loop._forward_csr(geom, x["yp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["A"], x["B"], True)[2]
    args = (geom, x["vp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["zdp"], x["zda"], x["A"], x["B"], us)
    a = loop._tangent_csr(*args, True)
    b = loop._tangent_csr_stepwise(*args, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for la, lb in zip(a[2:], b[2:]):
        assert len(la) == len(lb) and all(torch.equal(p, q) for p, q in zip(la, lb))
    inf = loop._tangent_csr(*args, False)                               # ping-pong buffers
    assert torch.equal(inf[0], a[0]) and torch.equal(inf[1], a[1]) and inf[2] == [] and inf[3] == []
    const = loop._tangent_csr(*args[:8], None, None, *args[10:], False)  # constant neighbours
    assert not torch.equal(const[0], a[0])
    outs = []
    for sweep in (loop._backward_csr, loop._backward_csr_stepwise):
        gzdp, gzda = torch.zeros_like(x["zp"]), torch.zeros_like(x["zp"]) if both else None
        dA, dB = loop._tangent_backward_csr(geom, K, x["vp"], x["mask"], x["A"], x["B"], a[2], a[3], us, x["zp"], x["za"],
                                            x["lam"], x["gam1"], x["gam2"], x["g_xdp"], x["g_zd"], gzdp, gzda, sweep=sweep)
        outs.append(list(dA) + list(dB) + [gzdp] + ([gzda] if both else []))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


@pytest.mark.parametrize("tier,tol", [("split", SPLIT_TOL), ("fp32", FP32_TOL)])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("dims,P,s,C,M,masked", SWEEPS)
def test_tangent_sweep_and_gradients_vs_restatement_at_the_device_gates(dims, P, s, C, M, masked, both, tier, tol):
    """The gates are computed on the CPU from the DEVICE's u_k; given them the sweep is linear, so the float64 restatement
    and its autograd are the reference of the tangent codes, the image tangent, both filter-gradient banks and the
    gradients of the neighbour tangents."""
    from cdlnet_video_amd import loop
    o = ops()
    d = sweep_case(dims, P, s, C, M, masked)
    geom, K = d["geom"], d["K"]
    N = geom.N
    x = on_device(d, both)
    with o.exact_fp32(tier == "fp32"):
        us = loop._forward_csr(geom, x["yp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["A"], x["B"],
                               True)[2]
        xdp, zdK, zd, rd = loop._tangent_csr(geom, x["vp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"],
                                             x["zdp"], x["zda"], x["A"], x["B"], us, True)
        gzdp, gzda = torch.zeros_like(x["zp"]), torch.zeros_like(x["zp"]) if both else None
        dA, dB = loop._tangent_backward_csr(geom, K, x["vp"], x["mask"], x["A"], x["B"], zd, rd, us, x["zp"], x["za"],
                                            x["lam"], x["gam1"], x["gam2"], x["g_xdp"], x["g_zd"], gzdp, gzda)
    bc = lambda t, k: t[k].cpu().reshape((N, M) + (1,) * len(dims))
    G = [R.gates(us[k].cpu(), d["zp"], d["za"] if both else None, bc(x["lam"], k), bc(x["gam1"], k),
                 bc(x["gam2"], k) if both else None) for k in range(K)]
    for k, gates in enumerate(G):
        for level, gate in enumerate(gates):
            dens = float(gate.float().mean())
            log(f"csr tangent {dims} both={both} {tier}: gate density k={k} level={level}: {dens:.3f}")
            assert 0.05 < dens < 0.95, (k, level, dens)
    leaf = lambda t: t.double().requires_grad_(True)
    A64, B64 = [leaf(w) for w in d["A"]], [leaf(w) for w in d["B"]]
    zdp64, zda64 = leaf(d["zdp"]), leaf(d["zda"]) if both else None
    m64 = d["mask"].double() if masked else None
    xdp64, zd64 = R.tangent_sweep(A64, B64, d["vp"].double(), m64, G, zdp64, zda64, s, tuple(p // 2 for p in P))
    ((d["g_xdp"].double() * xdp64).sum() + (d["g_zd"].double() * zd64).sum()).backward()
    tag = f"csr tangent {dims} both={both} {tier}"
    check(f"{tag} xdp", xdp, xdp64, tol)
    check(f"{tag} zd_K", zdK, zd64, tol)
    for k in range(K):
        check(f"{tag} dA[{k}]", dA[k], A64[k].grad, tol)
        check(f"{tag} dB[{k}]", dB[k], B64[k].grad, tol)
    check(f"{tag} dL/dzd_prev", gzdp, zdp64.grad, tol)
    if both:
        check(f"{tag} dL/dzd_after", gzda, zda64.grad, tol)


# ---------------------------------------------------------------------------------- jvp_recurrent
def small_net(cls_name, seed=3):
    import cdlnet_video_amd as cva
    torch.manual_seed(seed)
    net = getattr(cva, cls_name)(K=3, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n in ("t", "t2"):
                p.uniform_(2e-3, 1.5e-2)
            elif n in ("g", "g1", "g2"):
                p.uniform_(0.2, 1.4)
            else:
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net.cuda()


BRANCHES = [("CDLNet_CSR", False, False), ("CDLNet_CSR", True, False), ("CDLNet_CSRf2", False, False),
            ("CDLNet_CSRf2", True, False), ("CDLNet_CSRf2", False, True), ("CDLNet_CSRf2", True, True)]


@pytest.mark.parametrize("cls_name,prev,after", BRANCHES)
def test_jvp_recurrent_properties(cls_name, prev, after):
    """xhat, z are forward's; linear in (v, zdot_*); repeatable bit for bit; the thresholds get exactly zero gradient from
    a loss on (xdot, zdot) alone; the neighbour tangents get theirs."""
    import cdlnet_video_amd as cva
    net = small_net(cls_name)
    f2 = cls_name == "CDLNet_CSRf2"
    y = (cva.utils.synthetic_clip((2, 1, 22, 26), seed=1) + 0.1 * torch.randn(2, 1, 22, 26, generator=torch.Generator().manual_seed(2))).cuda()
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        seed_z = net(y.flip(0), sigma=25.0)[1]                        # a realistic neighbour code
    zshape = tuple(seed_z.shape)
    zp = seed_z if prev else None
    za = seed_z.flip(1) if after else None
    rnd = lambda shape: torch.randn(shape, generator=gen).cuda()
    v1, v2 = rnd(y.shape), rnd(y.shape)
    zd = {k: (rnd(zshape), rnd(zshape)) for k in ("prev", "after")}

    def call(v, i, scale=None):
        pick = lambda k: zd[k][i] if scale is None else scale[0] * zd[k][0] + scale[1] * zd[k][1]
        kw = dict(z_prev=zp, zdot_prev=pick("prev") if prev else None, sigma=25.0)
        if f2:
            kw.update(z_after=za, zdot_after=pick("after") if after else None)
        return net.jvp_recurrent(y, v, **kw)

    with torch.no_grad():
        fwd = net(y, zp, za, 25.0) if f2 else net(y, zp, 25.0)
        o1, o2 = call(v1, 0), call(v2, 1)
        again = call(v1, 0)
        a, b = 0.7, -1.3
        mix = call(a * v1 + b * v2, None, (a, b))
    assert torch.equal(o1[0], fwd[0]) and torch.equal(o1[2], fwd[1])
    assert all(torch.equal(p, q) for p, q in zip(o1, again))
    tol = SPLIT_TOL * (1 + abs(a) + abs(b))
    check(f"jvp_recurrent {cls_name} prev={prev} after={after} linear xdot", mix[1], a * o1[1] + b * o2[1], tol)
    check(f"jvp_recurrent {cls_name} prev={prev} after={after} linear zdot", mix[3], a * o1[3] + b * o2[3], tol)
    assert float(o1[1].abs().max()) > 0 and float(o1[3].abs().max()) > 0

    leaves = {k: t.clone().requires_grad_(True) for k, (t, _) in zd.items()}
    kw = dict(z_prev=zp, zdot_prev=leaves["prev"] if prev else None, sigma=25.0)
    if f2:
        kw.update(z_after=za, zdot_after=leaves["after"] if after else None)
    _, xdot, _, zdot = net.jvp_recurrent(y, v1, **kw)
    (torch.mean(v2 * xdot) + torch.mean(zd["prev"][1] * zdot)).backward()
    for n, p in net.named_parameters():
        if n in ("t", "t2", "g", "g1", "g2"):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
    used = net.A2 if (not f2 and not prev) else net.A
    assert float(used[1].weight.grad.abs().max()) > 0
    for k, on in (("prev", prev), ("after", after)):
        assert (leaves[k].grad is not None and float(leaves[k].grad.abs().max()) > 0) == on, k


def test_no_neighbour_branch_codes_and_gradients_vs_the_oracle_at_the_device_supports():
    """jvp_recurrent without a neighbour is the plain loop on whatever tier takes the geometry (TangentISTA handing out z_K and
    zd_K and taking their upstream gradients).  With the supports of the DEVICE's codes prescribed the oracle is affine in y
    (tangent_util.py), so z, zdot, xdot and the gradients of a loss on all four outputs are compared in float64 at the
    identical-support tolerance."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    net = small_net("CDLNet_CSRf2", seed=8)
    K, P, s = net.K, net.P, net.s
    gen = torch.Generator().manual_seed(12)
    y = cva.utils.synthetic_clip((2, 1, 22, 26), seed=4) + 0.1 * torch.randn(2, 1, 22, 26, generator=gen)
    v = torch.randn(y.shape, generator=gen)
    A, B = net._filters()
    with torch.no_grad():
        c = torch.full((2,), 25.0 / 255.0, device="cuda")
        outs = loop.run(y.cuda(), None, c, net.t, A, B, s, all_codes=True)
    codes = [t.cpu() for t in outs[2:]] + [outs[1].cpu()]
    dens = [float((t != 0).float().mean()) for t in codes]
    log(f"no-neighbour jvp_recurrent: code densities {dens}")
    assert all(0.05 < d < 0.95 for d in dens), dens
    xhat, xdot, z, zdot = net.jvp_recurrent(y.cuda(), v.cuda(), sigma=25.0)
    w = [torch.randn(t.shape, generator=gen) for t in (xdot, zdot, z)]
    loss = torch.mean(w[0].cuda() * xdot) + torch.mean(w[1].cuda() * zdot) + torch.mean(w[2].cuda() * z) \
        + torch.mean((xhat - y.cuda()) ** 2)
    loss.backward()

    sd = {k: t.detach().cpu().double() for k, t in net.state_dict().items()}
    names = [f"A.{k}.weight" for k in range(K)] + [f"B.{k}.weight" for k in range(K)] + ["t"]
    leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
    sd.update(leaves)
    kw = dict(K=K, P=P, s=s, sigma=25.0, adaptive=True, supports=[t.double() for t in codes], all_codes=True)
    xh64, c0 = O.ista(sd, y.double(), **kw)
    xv64, c1 = O.ista(sd, y.double() + v.double(), **kw)
    xd64, z64, zd64 = xv64 - xh64, c0[-1], c1[-1] - c0[-1]
    ref = torch.mean(w[0].double() * xd64) + torch.mean(w[1].double() * zd64) + torch.mean(w[2].double() * z64) \
        + torch.mean((xh64 - y.double()) ** 2)
    ref.backward()
    tag = "no-neighbour jvp_recurrent"
    for name, got, want in (("xhat", xhat, xh64), ("xdot", xdot, xd64), ("z", z, z64), ("zdot", zdot, zd64)):
        check(f"{tag} {name}", got, want, SPLIT_TOL)
    params = dict(net.named_parameters())
    for k in names:
        check(f"{tag} grad {k}", params[k].grad, leaves[k].grad, SPLIT_TOL)


def chain_jvp(net, f2, ys, bs, sigs):
    """The clip chains of the trainer composed by hand from jvp_recurrent calls: [(xhat_t, xdot_t)]."""
    if not f2:
        z = zd = None
        for _ in range(2):
            xp, xdp, zp, zdp = net.jvp_recurrent(ys[0], bs[0], z, zd, sigs[0])
            xc, xdc, z, zd = net.jvp_recurrent(ys[1], bs[1], zp, zdp, sigs[1])
        return [(xp, xdp), (xc, xdc)]
    _, _, zp, zdp = net.jvp_recurrent(ys[0], bs[0], None, None, None, None, sigs[0])
    net.jvp_recurrent(ys[1], bs[1], zp, zdp, None, None, sigs[1])
    xa, xda, za, zda = net.jvp_recurrent(ys[2], bs[2], zp, zdp, None, None, sigs[2])
    xc, xdc, _, _ = net.jvp_recurrent(ys[1], bs[1], zp, zdp, za, zda, sigs[1])
    xp, xdp, _, _ = net.jvp_recurrent(ys[0], bs[0], None, None, za, zda, sigs[0])
    return [(xp, xdp), (xc, xdc), (xa, xda)]


def sure(outs, ys, bs, sigs):
    loss = 0.0
    for (xhat, xdot), y, b, s in zip(outs, ys, bs, sigs):
        loss = loss + torch.mean((y - xhat) ** 2) + 2.0 * torch.mean((s / 255.0) ** 2 * b * xdot)
    return loss


@pytest.mark.parametrize("name,cls_name,D", [("c6_csr_jvp_chain", "CDLNet_CSR", 2), ("c7_csrf2_jvp_chain", "CDLNet_CSRf2", 3)])
def test_clip_chain_jvp_matches_the_reference(name, cls_name, D):
    """torch.func-style jvp of the reference net's clip chain, jointly in all frames, its SURE loss and its gradients; on
    the fp32 tier (the fixture's seed has the same gates in float32 and float64).  sure_loss_clip is that composition."""
    from cdlnet_video_amd import loop, train
    g = load_golden(name)
    net = build(g, cls_name)
    sigs = [dev(g["sigma"])] * D
    ys, bs = [g[f"y{t}"].cuda() for t in range(D)], [g[f"b{t}"].cuda() for t in range(D)]
    with loop.precision_scope("fp32"):
        outs = chain_jvp(net, D == 3, ys, bs, sigs)
        loss = sure(outs, ys, bs, sigs)
        loss.backward()
        for t in range(D):
            check(f"{name} xhat{t}", outs[t][0], g[f"xhat{t}"], XTOL)
            check(f"{name} xdot{t}", outs[t][1], g[f"xdot{t}"], XTOL)
        log(f"{name} loss {loss.item():.9e} ref {g['loss']:.9e} gate margin {g['gate_margin']:.2e}")
        assert abs(loss.item() - g["loss"]) < 1e-6 * abs(g["loss"])
        seen = 0
        for pname, p in net.named_parameters():
            ref = g["grad"].get(pname)
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, pname
                continue
            check(f"{name} grad {pname}", p.grad, ref, GTOL)
            seen += 1
        assert seen == len(g["grad"])
        hand = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        net.zero_grad(set_to_none=True)
        loss2, xhats = train.sure_loss_clip(net, ys, sigs, b=bs)
        loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    assert all(torch.equal(a, o[0]) for a, o in zip(xhats, outs))
    assert all(torch.equal(p.grad, hand[n]) for n, p in net.named_parameters() if p.grad is not None)


# ---------------------------------------------------------------------------------- clip steps
@pytest.mark.parametrize("name,cls_name,D", [("c8_csr_clip_step", "CDLNet_CSR", 2), ("c9_csrf2_clip_step", "CDLNet_CSRf2", 3)])
def test_supervised_clip_step_matches_the_reference(name, cls_name, D):
    """loss, gradient norm and the post-(clip, Adam) parameters of one reference clip step; the noise is the reference's
    (a CPU generator at the fixture's seed).  Tolerances: those of the f7 training-step test."""
    from cdlnet_video_amd import train
    g = load_golden(name)
    net = build(g, cls_name)
    opt_ = torch.optim.Adam(net.parameters(), lr=g["lr"])
    torch.manual_seed(g["noise_seed"])
    total = []

    def sync():                                                     # runs between backward and the clip
        for pname, p in net.named_parameters():
            if pname in g["grad"]:
                check(f"{name} grad {pname}", p.grad, g["grad"][pname], GTOL)
        total.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters() if p.grad is not None))))

    noise_std = tuple(g["noise_std"]) if isinstance(g["noise_std"], list) else g["noise_std"]      # c9: one level, all frames
    loss, sigmas, mse = train.train_step_clip(net, opt_, g["clip"].cuda(), noise_std, clip_grad=g["clip_grad"],
                                              project=False, grad_sync=sync, generator=torch.default_generator)
    for d in range(D):
        assert torch.equal(sigmas[d].cpu(), g[f"sigma{d}"]) if torch.is_tensor(sigmas[d]) else sigmas[d] == g[f"sigma{d}"]
    assert abs(loss.item() - g["loss"]) < 1e-7
    assert abs(mse.item() - g["mse"]) < 1e-7
    assert abs(total[0] - g["grad_norm"]) < 1e-4 * g["grad_norm"]
    sd = net.state_dict()
    for key, ref in g["after"].items():
        check(f"{name} after-step {key}", sd[key], ref, 2e-5)


@pytest.mark.parametrize("cls_name,D", [("CDLNet_CSR", 2), ("CDLNet_CSRf2", 3)])
def test_exact_sure_clip_steps_equal_the_hand_composed_ones(cls_name, D):
    """Two train_step_clip(mcsure="exact") steps == the same two steps written out with jvp_recurrent, bit for bit."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import train
    clip = torch.stack([cva.utils.synthetic_clip((2, 1, 20, 24), seed=10 + t) for t in range(D)], dim=2).cuda()
    nets = [small_net(cls_name, seed=5), small_net(cls_name, seed=5)]
    opts = [torch.optim.Adam(n.parameters(), lr=1e-3) for n in nets]
    gens = [torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)]
    for step in range(2):
        loss, sigmas, mse = train.train_step_clip(nets[0], opts[0], clip, (20, 30), clip_grad=5e-2, generator=gens[0],
                                                  mcsure="exact")
        clean = [clip[:, :, d] for d in range(D)]
        noisy, sigs = zip(*(cva.awgn(x, (20, 30), gens[1]) for x in clean))
        bs = [torch.randn(x.shape, generator=gens[1]).cuda() for x in clean]
        opts[1].zero_grad(set_to_none=True)
        hand = sure(chain_jvp(nets[1], D == 3, noisy, bs, sigs), noisy, bs, sigs)
        hand.backward()
        torch.nn.utils.clip_grad_norm_(nets[1].parameters(), 5e-2)
        opts[1].step()
        nets[1].project()
        assert torch.equal(loss, hand.detach()), step
        assert bool(torch.isfinite(mse)) and float(mse) > 0
    for (n, p), q in zip(nets[0].named_parameters(), nets[1].parameters()):
        assert torch.equal(p, q), n


def test_fit_trains_a_csr_net_on_clips(tmp_path):
    """fit takes the clip steps for a CSR net, logs 10 log10(1 / mse) per phase and writes the reference's files."""
    import cdlnet_video_amd as cva
    net = small_net("CDLNet_CSR", seed=6)
    opt_ = torch.optim.Adam(net.parameters(), lr=1e-3)
    clips = [torch.stack([cva.utils.synthetic_clip((2, 1, 20, 24), seed=20 + 2 * i + t) for t in range(2)], dim=2)
             for i in range(2)]
    hist = cva.fit(net, opt_, {"train": clips, "val": clips[:1], "test": clips[:1]}, epochs=1, device=torch.device("cuda"),
                   save_dir=str(tmp_path), noise_std=(20, 30), clip_grad=5e-2, verbose=False, log=lambda *_: None,
                   generator=torch.Generator().manual_seed(1), mcsure="exact")
    assert [h[1] for h in hist] == ["train", "val", "test"]
    assert all(h[2] == h[2] and abs(h[2]) < float("inf") for h in hist), hist
    for f in ("0.ckpt", "net.ckpt", "train.txt", "val.txt", "test.txt"):
        assert os.path.exists(tmp_path / f), f
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_gradient_bucket_syncs_once_per_clip_backward():
    """A clip step is up to ten reverse sweeps in one backward pass: an attached GradientBucket exchanges once, after all
    of them."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import train
    net = small_net("CDLNet_CSR", seed=7)
    opt_ = torch.optim.Adam(net.parameters(), lr=1e-3)
    clip = torch.stack([cva.utils.synthetic_clip((1, 1, 20, 24), seed=30 + t) for t in range(2)], dim=2).cuda()
    bucket = cva.parallel.GradientBucket(net.parameters()).attach()
    try:
        for i, mode in enumerate((False, "exact", True)):
            train.train_step_clip(net, opt_, clip, 25, generator=torch.Generator().manual_seed(2), mcsure=mode)
            assert bucket.syncs == i + 1, mode
            assert all(p.grad is not None for n, p in net.named_parameters() if n.startswith(("A.", "A2.")))
    finally:
        bucket.detach()
