"""The tangent of the CSR nets under a noise-level map on the GPU: the map form of the pointwise
tangent, the analysis entry point and the sweep that apply it, `csr_jvp_step`, and the exact SURE step with `noise=` --
bit for bit against the restatement at float32 gates (tests/csr_tangent_restate.py), against the float64 restatement on the
DEVICE's pieces (tests/csr_tangent_map_restate.py) and against the reference's forward-mode derivatives (fixtures c6m / c7m,
tools/make_golden_csr_tangent_map.py).  Tolerances: those of tests/test_gpu_csr_tangent.py for the same quantities."""
import contextlib
import functools

import pytest
import torch

import csr_tangent_map_restate as RM
import csr_tangent_restate as R
from arena_util import Arena
from gpu_util import check, launch_sites, load_golden, log
from sigmamap_util import smooth_map

pytestmark = pytest.mark.gpu

SPLIT_TOL, FP32_TOL = 5e-5, 1e-5          # the project's identical-support tolerances (split-bf16 tier, fp32 tier)
XTOL, GTOL = 1e-5, 2e-4                   # nets against the reference's fixtures (tests/test_gpu_csr.py)
K_PROX = "cdl_prox.hip:k_prox_fwd"


def ops():
    import cdlnet_video_amd as cva
    return cva.ops


def opt(v):
    return v.cuda() if v is not None else None


def level_map(shape, seed, lo=10.0, hi=40.0):
    """A noise-level map on the 255 scale: sigmamap_util.smooth_map plus a per-pixel term and a per-sample offset."""
    gen = torch.Generator().manual_seed(seed + 1)
    N = shape[0]
    offs = 2.5 * torch.arange(N, dtype=torch.float32).reshape((N,) + (1,) * (len(shape) - 1))
    return (smooth_map(shape, seed, lo, hi - 2.5 * N) + 2.0 * torch.rand(shape, generator=gen) + offs).contiguous()


# ---------------------------------------------------------------------------------- pointwise tangent
# code grids: 7 x 6 (fewer pixels than one map chunk of 1024), 12 x 20, 33 x 35 (a second pixel chunk), one 3-D grid
POINT = [(2, 4, 7, 6), (1, 9, 12, 20), (2, 9, 33, 35), (2, 4, 3, 20, 19)]


def pointwise_case(shape, seed):
    """Exact zeros (sparse neighbours), ties (u == z_prev, z_after == z_prev on nonzero elements), constant parts and
    slopes of either sign -- so that thresholds are negative on some pixels of a channel and positive on others."""
    gen = torch.Generator().manual_seed(seed)
    N, M = shape[:2]
    sp = shape[2:]
    sparse = lambda: 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
    u, zp, za = 0.05 * torch.randn(shape, generator=gen), sparse(), sparse()
    tie = torch.rand(shape, generator=gen)
    u = torch.where(tie < 0.05, zp, u)
    za = torch.where((tie > 0.9) & (zp != 0), zp, za)
    ud, zpd, zad = (torch.randn(shape, generator=gen) for _ in range(3))
    cmap = level_map((N, 1) + sp, seed) / 255.0
    lam0 = (torch.rand(N, M, generator=gen) - 0.15) * 0.06
    g10, g20 = (torch.rand(N, M, generator=gen) * 0.8 for _ in range(2))
    tsl = torch.stack([(torch.rand(M, generator=gen) - 0.3) * 0.4, torch.rand(M, generator=gen) * 3.0,
                       torch.rand(M, generator=gen) * 3.0])
    lam0.view(-1)[0] = -0.05                                       # a row that is negative whatever the map says
    tsl[0, M - 1] = -0.2                                           # and one whose sign follows the map
    return u, zp, za, ud, zpd, zad, cmap, lam0, g10, g20, tsl


def restated_thresholds(t0, cmap, tsl):
    """float32 t0[n,m] + c[n,pix] * tsl[m]: the product, then the sum (what cdl_map_threshold forms)."""
    N, M = t0.shape
    ones = (1,) * (cmap.dim() - 2)
    prod = cmap * tsl.reshape((1, M) + ones)
    return t0.reshape((N, M) + ones) + prod


@pytest.mark.parametrize("tangents", [False, True])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("shape", POINT)
def test_pointwise_map_tangent_equals_the_restatement_bit_for_bit(shape, both, tangents):
    o = ops()
    u, zp, za, ud, zpd, zad, cmap, lam0, g10, g20, tsl = pointwise_case(shape, sum(shape) + 2 * both + tangents)
    N, M = shape[:2]
    sp = shape[2:]
    lam, g1, g2 = (restated_thresholds(t0, cmap, row) for t0, row in zip((lam0, g10, g20), tsl))
    assert bool((lam < 0).any()) and bool((lam > 0).any())
    G = R.gates(u, zp, za if both else None, lam, g1, g2 if both else None)
    for gate in G:                                                  # every gate takes both values
        assert 0.02 < float(gate.float().mean()) < 0.998
    ref = R.prox_tangent(G, ud.double(), zpd.double() if tangents else None, zad.double() if tangents and both else None)
    geom = o.Geometry.make(N, 1, M, sp, (1,) * len(sp), (0,) * len(sp), 1)
    args = (u.cuda(), zp.cuda(), lam0.cuda(), g10.cuda(), za.cuda() if both else None, g20.cuda() if both else None,
            zpd.cuda() if tangents else None, zad.cuda() if tangents and both else None)
    mp = dict(cmap=cmap.cuda(), tslope=tsl.cuda())
    got = o.prox_csr_tangent(geom, ud.cuda(), *args, **mp)
    assert torch.equal(got.cpu(), ref.float())
    buf = ud.cuda().clone()                                        # out may alias ud
    assert o.prox_csr_tangent(geom, buf, *args, out=buf, **mp) is buf and torch.equal(buf, got)
    # the map changes the gates: the row form at the constant parts alone is another function
    assert not torch.equal(o.prox_csr_tangent(geom, ud.cuda(), *args), got)
    with pytest.raises(ValueError, match="go together"):
        o.prox_csr_tangent(geom, ud.cuda(), *args, cmap=mp["cmap"])


def test_a_constant_map_gives_the_row_forms_gates():
    """cmap = c[n] everywhere: the thresholds are the row form's t0 + c t1 (rounded the same way), so are the bits."""
    o = ops()
    shape = (2, 4, 7, 6)
    u, zp, za, ud, zpd, zad, _, lam0, g10, g20, tsl = pointwise_case(shape, 3)
    c = torch.tensor([0.07, 0.13])
    cmap = c.reshape(2, 1, 1, 1).expand(2, 1, 7, 6).contiguous()
    rows = [restated_thresholds(t0, c.reshape(2, 1, 1, 1), row).reshape(2, 4).contiguous().cuda()
            for t0, row in zip((lam0, g10, g20), tsl)]
    geom = o.Geometry.make(2, 1, 4, (7, 6), (1, 1), (0, 0), 1)
    got = o.prox_csr_tangent(geom, ud.cuda(), u.cuda(), zp.cuda(), lam0.cuda(), g10.cuda(), za.cuda(), g20.cuda(), zpd.cuda(),
                             zad.cuda(), cmap=cmap.cuda(), tslope=tsl.cuda())
    ref = o.prox_csr_tangent(geom, ud.cuda(), u.cuda(), zp.cuda(), rows[0], rows[1], za.cuda(), rows[2], zpd.cuda(), zad.cuda())
    assert torch.equal(got, ref)


def test_a_nan_behind_a_closed_gate_does_not_leak_under_a_map():
    o = ops()
    shape = (2, 9, 33, 35)
    u, zp, za, ud, zpd, zad, cmap, lam0, g10, g20, tsl = pointwise_case(shape, 5)
    lam, g1, g2 = (restated_thresholds(t0, cmap, row) for t0, row in zip((lam0, g10, g20), tsl))
    Ga, Gb, Gm = R.gates(u, zp, za, lam, g1, g2)
    nan = lambda t: torch.full_like(t, float("nan"))
    ud2 = torch.where(Gm & Gb & Ga, ud, nan(ud))                   # read only where all three gates are open
    zpd2 = torch.where(Gm & Gb & Ga, zpd, nan(zpd))
    zad2 = torch.where(Gm & ~Gb, zad, nan(zad))
    geom = o.Geometry.make(2, 1, 9, (33, 35), (1, 1), (0, 0), 1)
    mp = dict(cmap=cmap.cuda(), tslope=tsl.cuda())
    got = o.prox_csr_tangent(geom, ud2.cuda(), u.cuda(), zp.cuda(), lam0.cuda(), g10.cuda(), za.cuda(), g20.cuda(), zpd2.cuda(),
                             zad2.cuda(), **mp)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got.cpu(), R.prox_tangent((Ga, Gb, Gm), ud.double(), zpd.double(), zad.double()).float())
    G1 = R.gates(u, zp, None, lam, g1)
    ud1 = torch.where(G1[1] & G1[0], ud, nan(ud))
    zpd1 = torch.where(G1[1] & ~G1[0], zpd, nan(zpd))
    got1 = o.prox_csr_tangent(geom, ud1.cuda(), u.cuda(), zp.cuda(), lam0.cuda(), g10.cuda(), zd_prev=zpd1.cuda(), **mp)
    assert not bool(torch.isnan(got1).any())


# ---------------------------------------------------------------------------------- the analysis entry point
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
    lam, g1, g2 = ((torch.rand(N, M, generator=gen) * sc).cuda() for sc in (0.1, 0.6, 0.6))
    cmap = (level_map((N, 1) + tuple(geom.code_shape()[2:]), seed) / 255.0).cuda()
    tsl = (torch.rand(3, M, generator=gen) * torch.tensor([[1.0], [5.0], [5.0]])).cuda()
    return x, w, zin, u, zp, za, zpd, zad, lam, g1, g2, dict(cmap=cmap, tslope=tsl)


def epilogue_equals_two_calls(o, geom, both, seed):
    x, w, zin, u, zp, za, zpd, zad, lam, g1, g2, mp = epilogue_case(geom, seed)
    za, g2, zad = (za, g2, zad) if both else (None, None, None)
    ud = o.analysis(geom, x, w, -1.0, zin, None, None)
    for tp, ta in ((zpd, zad), (None, None)):
        ref = o.prox_csr_tangent(geom, ud, u, zp, lam, g1, za, g2, tp, ta, **mp)
        got = o.analysis_prox_tangent(geom, x, w, -1.0, zin, u, zp, lam, g1, za, g2, tp, ta, **mp)
        assert torch.equal(got, ref)
        assert 0.02 < float((ref != 0).float().mean()) < 0.98
        assert not torch.equal(got, o.analysis_prox_tangent(geom, x, w, -1.0, zin, u, zp, lam, g1, za, g2, tp, ta))
    first = o.analysis_prox_tangent(geom, x, w, 1.0, None, u, zp, lam, g1, za, g2, zpd, zad, **mp)      # iteration 0: no zin
    assert torch.equal(first, o.prox_csr_tangent(geom, o.analysis(geom, x, w, 1.0), u, zp, lam, g1, za, g2, zpd, zad, **mp))


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("dims,P,s,C,M", [((14, 12), (5, 5), 2, 1, 4), ((12, 20), (7, 7), 1, 1, 9), ((66, 70), (5, 5), 2, 1, 9)])
def test_analysis_prox_tangent_with_a_map_equals_analysis_then_pointwise(dims, P, s, C, M, both):
    """cdl_analysis_prox_tangent with a map == cdl_analysis then cdl_prox_csr_tangent with it, bit for bit (VALU analysis)."""
    o = ops()
    geom = o.Geometry.make(2, C, M, dims, P, tuple(p // 2 for p in P), s)
    epilogue_equals_two_calls(o, geom, both, len(dims) * 7 + P[-1] + both)


MFMA_ENV = {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"}
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"


@pytest.mark.parametrize("both", [False, True])
def test_analysis_prox_tangent_with_a_map_on_the_matrix_core_analysis(both, hip_env):
    """At a shape the matrix-core analysis takes: its plain instance (no CSR epilogue, no map: the map only enters the
    pointwise pass), then k_prox_fwd once; the bits of the two-call form."""
    for k, v in MFMA_ENV.items():
        hip_env(k, v)
    o = ops()
    geom = o.Geometry.make(16, 1, 8, (60, 121), (5, 5), (2, 2), 1)
    x, w, zin, u, zp, za, zpd, zad, lam, g1, g2, mp = epilogue_case(geom, 31 + both)
    za, g2, zad = (za, g2, zad) if both else (None, None, None)
    ud = o.analysis(geom, x, w, -1.0, zin, None, None)
    with o.trace() as t:
        got = o.analysis_prox_tangent(geom, x, w, -1.0, zin, u, zp, lam, g1, za, g2, zpd, zad, **mp)
    assert torch.equal(got, o.prox_csr_tangent(geom, ud, u, zp, lam, g1, za, g2, zpd, zad, **mp))
    sites = launch_sites(t)
    recs = sites.get(K_ANA, [])
    assert recs and all(r.template()["PROX"] is False and r.template()["REV"] is False and r.template()["MAP"] is False
                        for r in recs), sorted(sites)
    assert len(sites.get(K_PROX, [])) == 1, sorted(sites)


# ---------------------------------------------------------------------------------- the sweeps
# (frame / padded extent, P, s, M, K, masked): code grids 7 x 6, 12 x 20 and 33 x 35
SWEEPS = [((14, 12), 5, 2, 4, 2, True), ((12, 20), 7, 1, 9, 3, False), ((66, 70), 5, 2, 9, 2, True)]


@functools.lru_cache(maxsize=None)
def sweep_case(dims, P, s, M, K, masked):
    """Seeded CPU inputs of one sweep geometry (read-only; shared by the tests below)."""
    o = ops()
    gen = torch.Generator().manual_seed(sum(dims) + M)
    N = 2
    geom = o.Geometry.make(N, 1, M, dims, (P, P), (P // 2, P // 2), s)
    rnd = lambda shape, sc=1.0: sc * torch.randn(shape, generator=gen)
    d = {"geom": geom, "K": K, "yp": rnd(geom.image_shape()), "vp": rnd(geom.image_shape()),
         "mask": (torch.rand(geom.image_shape(), generator=gen) > 0.3).float() if masked else None,
         "A": [rnd(geom.filter_shape(), 0.08) for _ in range(K)], "B": [rnd(geom.filter_shape(), 0.08) for _ in range(K)],
         "cmap": level_map((N, 1) + tuple(geom.code_shape()[2:]), sum(dims)) / 255.0}
    d["t"], d["g1"], d["g2"] = (torch.rand(K, 2, M, 1, 1, generator=gen) * sc for sc in (0.25, 1.0, 1.0))
    for p in ("t", "g1", "g2"):
        d[p][:, 1] *= 4.0                                           # slopes that matter at c ~ 0.04 .. 0.16
    for k in ("zp", "za"):
        d[k] = rnd(geom.code_shape(), 0.5) * (torch.rand(geom.code_shape(), generator=gen) > 0.3)
    for k in ("zdp", "zda", "g_zd"):
        d[k] = rnd(geom.code_shape())
    d["g_xdp"] = rnd(geom.image_shape())
    return d


def on_device(d, both):
    from cdlnet_video_amd import loop
    o = ops()
    N = d["geom"].N
    lam, gam1, gam2 = (o.thresholds(d[k].cuda(), None, N) for k in ("t", "g1", "g2"))      # the constant parts
    cu = lambda k: [w.cuda() for w in d[k]] if isinstance(d[k], list) else opt(d[k])
    dd = {k: cu(k) for k in ("yp", "vp", "mask", "A", "B", "zp", "za", "zdp", "zda", "g_zd", "g_xdp", "cmap")}
    dd.update(lam=lam, gam1=gam1, gam2=gam2 if both else None,
              tslope=loop._csr_slopes(d["t"].cuda(), d["g1"].cuda(), d["g2"].cuda() if both else None))
    if not both:
        dd["za"] = dd["zda"] = None
    return dd


def site_sequence(trace):
    return [next(iter(launch_sites([r]))) for r in trace]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("dims,P,s,M,K,masked", SWEEPS)
def test_map_tangent_sweeps_equal_stepwise_launches(dims, P, s, M, K, masked, both):
    """cdl_csr_tangent_forward with a map and its reverse sweep (cdl_ista_backward's CSR branch with the map, c = NULL,
    dcmap = NULL) enqueue the launches the stepwise Python twins make: every output is bit-identical.  The launch trace
    shows the sequence of the sweep without a map, and every pointwise pass at cdl_prox.hip:k_prox_fwd."""
    from cdlnet_video_amd import loop
    o = ops()
    d = sweep_case(dims, P, s, M, K, masked)
    geom = d["geom"]
    x = on_device(d, both)
    mp = dict(cmap=x["cmap"], tslope=x["tslope"])
    us = loop._forward_csr(geom, x["yp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["A"], x["B"], True,
                           **mp)[2]
    args = (geom, x["vp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["zdp"], x["zda"], x["A"], x["B"], us)
    with o.trace() as t_map:
        a = loop._tangent_csr(*args, True, **mp)
    b = loop._tangent_csr_stepwise(*args, True, **mp)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for la, lb in zip(a[2:], b[2:]):
        assert len(la) == len(lb) and all(torch.equal(p, q) for p, q in zip(la, lb))
    inf = loop._tangent_csr(*args, False, **mp)                         # ping-pong buffers
    assert torch.equal(inf[0], a[0]) and torch.equal(inf[1], a[1]) and inf[2] == [] and inf[3] == []
    with o.trace() as t_row:
        row = loop._tangent_csr(*args, True)                            # the constant parts alone: other gates
    assert not torch.equal(row[0], a[0])
    seq = site_sequence(t_map)
    assert seq == site_sequence(t_row)
    assert seq.count(K_PROX) == K, seq
    outs = []
    for sweep in (loop._backward_csr, loop._backward_csr_stepwise):
        gzdp, gzda = torch.zeros_like(x["zp"]), torch.zeros_like(x["zp"]) if both else None
        dA, dB = loop._tangent_backward_csr(geom, K, x["vp"], x["mask"], x["A"], x["B"], a[2], a[3], us, x["zp"], x["za"],
                                            x["lam"], x["gam1"], x["gam2"], x["g_xdp"], x["g_zd"], gzdp, gzda, sweep=sweep,
                                            **mp)
        outs.append(list(dA) + list(dB) + [gzdp] + ([gzda] if both else []))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


def test_one_of_the_pair_is_refused_before_any_launch():
    """cmap without tslope (or the reverse) is CDL_EINVAL from the C entry points themselves, nothing enqueued."""
    from cdlnet_video_amd import _lib, loop
    o = ops()
    d = sweep_case(*SWEEPS[0])
    geom, K = d["geom"], d["K"]
    x = on_device(d, False)
    us = loop._forward_csr(geom, x["yp"], x["mask"], x["lam"], x["gam1"], None, x["zp"], None, x["A"], x["B"], True)[2]
    out = torch.empty_like(x["zp"])
    ws, n = o.ista_scratch(geom, out.device)
    zd = [torch.empty_like(out) for _ in range(K)]
    rd = [torch.empty_like(x["yp"]) for _ in range(K - 1)]
    for cmap, tsl in ((x["cmap"], None), (None, x["tslope"])):
        with o.trace() as t:
            for name, args in (
                    ("cdl_prox_csr_tangent", (geom, x["zdp"], us[0], x["zp"], None, x["lam"][0], x["gam1"][0], None, None, None,
                                              out, cmap, tsl)),
                    ("cdl_analysis_prox_tangent", (geom, x["vp"], x["A"][0], 1.0, None, us[0], x["zp"], None, x["lam"][0],
                                                   x["gam1"][0], None, None, None, out, None, 0, cmap, tsl)),
                    ("cdl_csr_tangent_forward", (geom, K, x["vp"], x["mask"], x["zp"], None, x["lam"], x["gam1"], None, None,
                                                 None, x["A"], x["B"], us, zd, rd, torch.empty_like(x["yp"]), ws, n, cmap, tsl))):
                with pytest.raises(_lib.HipKernelError, match=rf"^{name}: invalid argument \(CDL_EINVAL\)$"):
                    o._call(name, *args)
        assert len(t) == 0


# ---------------------------------------------------------------------------------- csr_jvp_step against float64
def small_net(cls_name, K, M, P, s, seed=3):
    import cdlnet_video_amd as cva
    torch.manual_seed(seed)
    net = getattr(cva, cls_name)(K=K, M=M, P=P, s=s, C=1, t0=5e-3, adaptive=True, init=True)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n in ("t", "t2"):
                p.uniform_(2e-3, 1.5e-2)
                p[:, 1] *= 4.0
            elif n in ("g", "g1", "g2"):
                p.uniform_(0.2, 1.4)
                p[:, 1] *= 2.0
            else:
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net.cuda()


# frames (2,1,13,11) at s = 2 (code grid 7 x 6, reflect-padded), (1,1,12,20) at s = 1, (1,1,65,69) at s = 2 (33 x 35)
NETS = [((2, 1, 13, 11), 2, 2, 4, 5), ((1, 1, 12, 20), 1, 3, 9, 7), ((1, 1, 65, 69), 2, 2, 4, 5)]
BRANCHES = [("CDLNet_CSR", True, False), ("CDLNet_CSRf2", True, False), ("CDLNet_CSRf2", True, True),
            ("CDLNet_CSRf2", False, True)]


@functools.lru_cache(maxsize=None)
def step_case(shape, s, K, M, P, cls_name, masked):
    """(net, CPU inputs) of one csr_jvp_step case; the neighbour codes are realistic ones (a no-neighbour call's code of
    the flipped frame, and its channel flip)."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd.net import _code_grid
    net = small_net(cls_name, K, M, P, s, seed=3 + M)
    gen = torch.Generator().manual_seed(sum(shape) + K)
    y = cva.utils.synthetic_clip(shape, seed=1) + 0.1 * torch.randn(shape, generator=gen)
    v = torch.randn(shape, generator=gen)
    mask = (torch.rand(shape, generator=gen) > 0.3).float() if masked else None
    grid = _code_grid(shape[2:], s)
    sigma = level_map((shape[0], 1) + grid, sum(shape))
    with torch.no_grad():
        seed_z = cva.temporal.csr_step(net, y.flip(-1).cuda(), sigma=25.0)[1].cpu()
    zshape = tuple(seed_z.shape)
    d = dict(y=y, v=v, mask=mask, sigma=sigma, zp=seed_z, za=seed_z.flip(1).contiguous(),
             zdp=torch.randn(zshape, generator=gen), zda=torch.randn(zshape, generator=gen),
             w=[torch.randn(sh, generator=gen) for sh in (shape, shape, zshape, zshape)])
    return net, d


def branch_params(net, cls_name, prev, after):
    """(t, g1, g2) of the branch, as csr_step picks them."""
    if cls_name == "CDLNet_CSR":
        return net.t, net.g, None
    if prev and after:
        return net.t, net.g1, net.g2
    return net.t, (net.g1 if prev else net.g2), None


def device_pieces(net, cls_name, prev, after, d, per_sample=None):
    """The pieces of every iteration from the DEVICE's u_k (the primal sweep csr_jvp_step runs, repeated through loop's
    front end with the same operands: the same launches, the same bits), evaluated on the CPU in float32 at the restated
    float32 thresholds.  per_sample (N,): the row form at these levels instead of the map d["sigma"], its gates read at the
    device's own (K,N,M) thresholds."""
    from cdlnet_video_amd import loop
    o = ops()
    t, g1, g2 = branch_params(net, cls_name, prev, after)
    A, B = net._filters()
    yp, _, _, mask_p = o.preprocess(d["y"].cuda(), net.s, opt(d["mask"]))
    geom = loop._sweep_geometry(yp, A, net.s)
    N = geom.N
    zp = (d["zp"] if prev else d["za"]).cuda()                     # the after-only branch: the one-neighbour map around z_after
    za = d["za"].cuda() if (prev and after) else None
    c = (d["sigma"] / 255.0).cuda()
    with torch.no_grad():
        cs = None if per_sample is None else (per_sample / 255.0).cuda()
        lam, gam1 = o.thresholds(t, cs, N), o.thresholds(g1, cs, N)
        gam2 = o.thresholds(g2, cs, N) if za is not None else None
        mp = {} if per_sample is not None else dict(cmap=c, tslope=loop._csr_slopes(t, g1, g2 if za is not None else None))
        us = loop._forward_csr(geom, yp, mask_p, lam, gam1, gam2, zp, za, [w.detach() for w in A], [w.detach() for w in B],
                               True, **mp)[2]
    if per_sample is not None:
        row = lambda th, k: th[k].cpu().reshape(N, -1, 1, 1)
        return [RM.pieces(us[k].cpu(), zp.cpu(), za.cpu() if za is not None else None, row(lam, k), row(gam1, k),
                          row(gam2, k) if za is not None else None) for k in range(net.K)]
    cc = d["sigma"] / 255.0
    tc, g1c, g2c = t.detach().cpu(), g1.detach().cpu(), (g2.detach().cpu() if g2 is not None else None)
    return [RM.pieces(us[k].cpu(), zp.cpu(), za.cpu() if za is not None else None, RM.thresholds(tc, k, cc),
                      RM.thresholds(g1c, k, cc), RM.thresholds(g2c, k, cc) if za is not None else None)
            for k in range(net.K)]


@pytest.mark.parametrize("tier,tol", [("split", SPLIT_TOL), ("fp32", FP32_TOL)])
@pytest.mark.parametrize("cls_name,prev,after", BRANCHES)
@pytest.mark.parametrize("shape,s,K,M,P", NETS)
def test_csr_jvp_step_with_a_map_vs_float64_on_the_device_pieces(shape, s, K, M, P, cls_name, prev, after, tier, tol):
    """(xhat, xdot, z, zdot) and every gradient of a loss on all four -- both banks, t, g*, the neighbour codes and their
    tangents; dt[:,1], dg*[:,1] the map-weighted sums -- against float64 autograd of the call restated on the pieces the
    device took."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    masked = (len(cls_name) + prev + 2 * after + s) % 2 == 0        # a mask in half the cases
    net, d = step_case(shape, s, K, M, P, cls_name, masked)
    net.zero_grad(set_to_none=True)
    leaf = lambda k: d[k].cuda().clone().requires_grad_(True)
    dev = {k: leaf(k) for k in (("zp", "zdp") if prev else ()) + (("za", "zda") if after else ())}
    tag = f"csr_jvp_step map {shape} {cls_name} prev={prev} after={after} {tier}"
    scope = loop.precision_scope("fp32") if tier == "fp32" else contextlib.nullcontext()
    with scope, ops().exact_fp32(tier == "fp32"):
        pcs = device_pieces(net, cls_name, prev, after, d)
        outs = cva.temporal.csr_jvp_step(net, d["y"].cuda(), d["v"].cuda(), dev.get("zp"), dev.get("zdp"), dev.get("za"),
                                         dev.get("zda"), sigma=d["sigma"].cuda(), mask=opt(d["mask"]) if masked else 1)
        sum(torch.mean(w.cuda() * o_) for w, o_ in zip(d["w"], outs)).backward()
    for k, pc in enumerate(pcs):
        for level, gate in enumerate(pc["G"]):
            dens = float(gate.float().mean())
            log(f"{tag}: gate density k={k} level={level}: {dens:.3f}")
            assert 0.005 < dens < 0.995, (k, level, dens)       # every gate takes both values

    t, g1, g2 = branch_params(net, cls_name, prev, after)
    l64 = lambda x: x.detach().cpu().double().requires_grad_(True)
    A, B = net._filters()
    A64, B64, t64, g164 = [l64(w) for w in A], [l64(w) for w in B], l64(t), l64(g1)
    g264 = l64(g2) if g2 is not None else None
    n64 = {k: l64(d[k]) for k in dev}
    first, firstd = ("zp", "zdp") if prev else ("za", "zda")       # the one-neighbour map reads its code in z_prev's place
    both = prev and after
    ref = RM.call_at(pcs, A64, B64, t64, g164, g264, d["y"].double(), d["v"].double(), n64[first], n64[firstd],
                     n64["za"] if both else None, n64["zda"] if both else None, d["sigma"].double() / 255.0, s=s, P=P,
                     mask=d["mask"].double() if masked else None)
    sum(torch.mean(w.double() * r) for w, r in zip(d["w"], ref)).backward()
    for name, got, want in zip(("xhat", "xdot", "z", "zdot"), outs, ref):
        check(f"{tag} {name}", got, want, tol)
    for k in range(K):
        check(f"{tag} dA[{k}]", A[k].grad, A64[k].grad, tol)
        check(f"{tag} dB[{k}]", B[k].grad, B64[k].grad, tol)
    check(f"{tag} dt", t.grad, t64.grad, tol)
    check(f"{tag} dt[:,1] (map-weighted)", t.grad[:, 1], t64.grad[:, 1], tol)
    check(f"{tag} dg1", g1.grad, g164.grad, tol)
    check(f"{tag} dg1[:,1] (map-weighted)", g1.grad[:, 1], g164.grad[:, 1], tol)
    if g2 is not None:
        check(f"{tag} dg2", g2.grad, g264.grad, tol)
        check(f"{tag} dg2[:,1] (map-weighted)", g2.grad[:, 1], g264.grad[:, 1], tol)
    for k in dev:
        check(f"{tag} dL/d{k}", dev[k].grad, n64[k].grad, tol)


# ---------------------------------------------------------------------------------- constant maps, scalars
@pytest.mark.parametrize("cls_name,prev,after", [("CDLNet_CSR", False, False), ("CDLNet_CSRf2", False, False)] + BRANCHES)
def test_scalar_and_constant_map_sigma_through_csr_jvp_step(cls_name, prev, after):
    """A float or per-sample sigma: the bits of jvp_recurrent.  A map that is constant per sample: xhat, z are csr_step's
    bit for bit, xdot / zdot are jvp_recurrent's at the per-sample level whenever the gates read off the kept u_k agree
    (the row form rounds t0 + c t1 in cdl_thresholds, the map form per element: the same expression)."""
    import cdlnet_video_amd as cva
    shape, s, K, M, P = NETS[0]
    net, d = step_case(shape, s, K, M, P, cls_name, False)
    y, v = d["y"].cuda(), d["v"].cuda()
    f2 = cls_name == "CDLNet_CSRf2"
    codes = dict(z_prev=opt(d["zp"]) if prev else None, zdot_prev=opt(d["zdp"]) if prev else None)
    if f2:
        codes.update(z_after=opt(d["za"]) if after else None, zdot_after=opt(d["zda"]) if after else None)
    per_sample = torch.tensor([17.0, 31.0]).reshape(2, 1, 1, 1).cuda()
    with torch.no_grad():
        for sigma in (25.0, per_sample):
            a = cva.temporal.csr_jvp_step(net, y, v, sigma=sigma, **codes)
            b = net.jvp_recurrent(y, v, sigma=sigma, **codes)
            assert all(torch.equal(p, q) for p, q in zip(a, b))
        const = per_sample.expand(2, 1, 7, 6).contiguous()
        m = cva.temporal.csr_jvp_step(net, y, v, sigma=const, **codes)
        prim = cva.temporal.csr_step(net, y, codes["z_prev"], codes.get("z_after"), sigma=const)
        assert torch.equal(m[0], prim[0]) and torch.equal(m[2], prim[1])
        same = torch.equal(m[0], b[0]) and torch.equal(m[2], b[2])
        tangent_same = torch.equal(m[1], b[1]) and torch.equal(m[3], b[3])
        log(f"constant map {cls_name} prev={prev} after={after}: primal bits equal the per-sample call's: {same}; "
            f"tangent bits: {tangent_same}")
        if prev or after:
            pm = device_pieces(net, cls_name, prev, after, dict(d, sigma=const.cpu()))
            pr = device_pieces(net, cls_name, prev, after, d, per_sample=per_sample.reshape(-1).cpu())
            gates_agree = all(torch.equal(g_, h_) for a_, b_ in zip(pm, pr) for g_, h_ in zip(a_["G"], b_["G"]))
            log(f"constant map {cls_name} prev={prev} after={after}: gates of the kept u_k agree: {gates_agree}")
            if gates_agree:
                assert tangent_same
        check(f"constant map {cls_name} prev={prev} after={after} xdot", m[1], b[1], SPLIT_TOL)
        check(f"constant map {cls_name} prev={prev} after={after} zdot", m[3], b[3], SPLIT_TOL)
    with pytest.raises(NotImplementedError, match="map"):
        net.jvp_recurrent(y, v, sigma=const, **codes)
    with pytest.raises(NotImplementedError, match="requires grad"):
        cva.temporal.csr_jvp_step(net, y, v, sigma=const.clone().requires_grad_(True), **codes)


# ---------------------------------------------------------------------------------- the fixtures
def build(g, cls_name):
    import cdlnet_video_amd as cva
    K, M, P, s, C = g["hyper"]
    net = getattr(cva, cls_name)(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=True, init=False)
    net.load_state_dict(g["sd"])
    return net.cuda()


def chain_jvp_step(net, f2, ys, bs, sigs):
    """The clip chains of the trainer composed by hand from csr_jvp_step calls: [(xhat_t, xdot_t)]."""
    import cdlnet_video_amd as cva
    step = cva.temporal.csr_jvp_step
    if not f2:
        z = zd = None
        for _ in range(2):
            xp, xdp, zp, zdp = step(net, ys[0], bs[0], z, zd, sigma=sigs[0])
            xc, xdc, z, zd = step(net, ys[1], bs[1], zp, zdp, sigma=sigs[1])
        return [(xp, xdp), (xc, xdc)]
    _, _, zp, zdp = step(net, ys[0], bs[0], sigma=sigs[0])
    step(net, ys[1], bs[1], zp, zdp, sigma=sigs[1])
    xa, xda, za, zda = step(net, ys[2], bs[2], zp, zdp, sigma=sigs[2])
    xc, xdc, _, _ = step(net, ys[1], bs[1], zp, zdp, za, zda, sigma=sigs[1])
    xp, xdp, _, _ = step(net, ys[0], bs[0], None, None, za, zda, sigma=sigs[0])
    return [(xp, xdp), (xc, xdc), (xa, xda)]


def sure(outs, ys, bs, noise):
    loss = 0.0
    for (xhat, xdot), y, b, n in zip(outs, ys, bs, noise):
        loss = loss + torch.mean((y - xhat) ** 2) + 2.0 * torch.mean((n / 255.0) ** 2 * b * xdot)
    return loss


@pytest.mark.parametrize("name,cls_name,D", [("c6m_csr_jvp_chain_map", "CDLNet_CSR", 2),
                                             ("c7m_csrf2_jvp_chain_map", "CDLNet_CSRf2", 3)])
def test_clip_chain_jvp_under_a_map_matches_the_reference(name, cls_name, D):
    """Forward-mode jvp of the reference net's clip chain under per-frame code-grid maps (stride 2, an odd frame), its SURE
    loss with image-resolution weights and its gradients; on the fp32 tier (the fixture's seed has the same gates in float32
    and float64).  sure_loss_clip(.., noise=..) is that composition."""
    from cdlnet_video_amd import loop, train
    g = load_golden(name)
    net = build(g, cls_name)
    sigs, noise = [g[f"sigma{t}"].cuda() for t in range(D)], [g[f"noise{t}"].cuda() for t in range(D)]
    ys, bs = [g[f"y{t}"].cuda() for t in range(D)], [g[f"b{t}"].cuda() for t in range(D)]
    with loop.precision_scope("fp32"):
        outs = chain_jvp_step(net, D == 3, ys, bs, sigs)
        loss = sure(outs, ys, bs, noise)
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
        loss2, xhats = train.sure_loss_clip(net, ys, sigs, b=bs, noise=noise)
        loss2.backward()
        with pytest.raises(ValueError, match="noise="):
            train.sure_loss_clip(net, ys, sigs, b=bs)
    assert torch.equal(loss2.detach(), loss.detach())
    assert all(torch.equal(a, o_[0]) for a, o_ in zip(xhats, outs))
    assert all(torch.equal(p.grad, hand[n]) for n, p in net.named_parameters() if p.grad is not None)


@pytest.mark.parametrize("cls_name,D", [("CDLNet_CSR", 2), ("CDLNet_CSRf2", 3)])
def test_exact_sure_clip_step_with_a_level_map_on_a_stride_2_net(cls_name, D):
    """train_step_clip(mcsure="exact") with a tensor noise_std (one image-resolution level map per frame) on a stride-2 net:
    the net takes the level on its code grid, the divergence weight stays at image resolution; the loss is finite and the
    parameters move.  eval_step_clip takes the same levels."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import train
    net = small_net(cls_name, 2, 4, 5, 2, seed=5)
    opt_ = torch.optim.Adam(net.parameters(), lr=1e-3)
    clip = torch.stack([cva.utils.synthetic_clip((2, 1, 13, 11), seed=10 + t) for t in range(D)], dim=2).cuda()
    nstd = torch.stack([level_map((2, 1, 13, 11), 40 + t) for t in range(D)], dim=2).cuda()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    loss, sigmas, mse = train.train_step_clip(net, opt_, clip, nstd, clip_grad=5e-2, generator=torch.Generator().manual_seed(7),
                                              mcsure="exact")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(mse)) and float(mse) > 0
    assert all(torch.equal(sigmas[t], nstd[:, :, t]) for t in range(D))
    moved = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert any(n.startswith("A.") for n in moved) and "t" in moved, moved
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    with torch.no_grad():
        el, _, emse = train.eval_step_clip(net, clip, nstd, torch.Generator().manual_seed(8))
    assert bool(torch.isfinite(el)) and float(emse) > 0


@pytest.mark.parametrize("per_frame", [False, True])
def test_fit_takes_a_level_map_for_a_csr_net(tmp_path, per_frame):
    """fit(noise_std=<tensor>, mcsure="exact") on a stride-2 CDLNet_CSR: one map for every frame (B,1,H,W), or one per frame
    (B,1,D,H,W); train, val and test all take it."""
    import cdlnet_video_amd as cva
    net = small_net("CDLNet_CSR", 2, 4, 5, 2, seed=6)
    opt_ = torch.optim.Adam(net.parameters(), lr=1e-3)
    clips = [torch.stack([cva.utils.synthetic_clip((2, 1, 13, 11), seed=20 + 2 * i + t) for t in range(2)], dim=2)
             for i in range(2)]
    nstd = torch.stack([level_map((2, 1, 13, 11), 50 + t) for t in range(2)], dim=2) if per_frame \
        else level_map((2, 1, 13, 11), 50)
    before = net.t.detach().clone()
    hist = cva.fit(net, opt_, {"train": clips, "val": clips[:1], "test": clips[:1]}, epochs=1, device=torch.device("cuda"),
                   save_dir=str(tmp_path), noise_std=nstd, clip_grad=5e-2, verbose=False, log=lambda *_: None,
                   generator=torch.Generator().manual_seed(1), mcsure="exact")
    assert [h[1] for h in hist] == ["train", "val", "test"]
    assert all(h[2] == h[2] and abs(h[2]) < float("inf") for h in hist), hist
    assert not torch.equal(net.t.detach(), before) and all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_sure_loss_with_noise_on_a_stride_2_cdlnet():
    """The plain nets too: a code-grid map as sigma, the image-resolution level as noise=; train_step derives the one from
    the other."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import train
    torch.manual_seed(2)
    net = cva.CDLNet(K=2, M=8, P=5, s=2, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    y = (cva.utils.synthetic_clip((2, 1, 13, 11), seed=3)).cuda()
    noise = level_map((2, 1, 13, 11), 9).cuda()
    sigma = cva.utils.sigma_to_code_grid(noise, 2)
    b = torch.randn(y.shape, generator=torch.Generator().manual_seed(4)).cuda()
    with pytest.raises(ValueError, match="noise="):
        train.sure_loss(net, y, sigma, b=b)
    loss, xhat = train.sure_loss(net, y, sigma, b=b, noise=noise)
    xh, xd = net.jvp(y, b, sigma)
    assert torch.equal(loss, torch.mean((y - xh) ** 2) + 2.0 * torch.mean((noise / 255.0) ** 2 * b * xd))
    loss.backward()
    assert float(net.t.grad.abs().max()) > 0
    fd = train.mcsure_loss(net, y, net(y, sigma)[0], sigma, b=b, noise=noise)
    assert bool(torch.isfinite(fd))
    opt_ = torch.optim.Adam(net.parameters(), lr=1e-3)
    before = net.t.detach().clone()
    l2, level = train.train_step(net, opt_, y, noise, mcsure="exact", generator=torch.Generator().manual_seed(5))
    assert level is noise and bool(torch.isfinite(l2)) and not torch.equal(net.t.detach(), before)


# ---------------------------------------------------------------------------------- guard-banded operands
@pytest.mark.parametrize("both", [False, True])
def test_map_operands_on_guard_banded_4_byte_aligned_views(both):
    """cmap, tslope and the constant parts need float alignment only: the three entry points on arena views at element
    offset 1 return the bits of the aligned call and write nothing outside their payloads."""
    from cdlnet_video_amd import loop
    o = ops()
    d = sweep_case(*SWEEPS[2])                                      # 33 x 35: two pixel chunks, the second one partial
    geom, K = d["geom"], d["K"]
    x = on_device(d, both)
    mp = dict(cmap=x["cmap"], tslope=x["tslope"])
    us = loop._forward_csr(geom, x["yp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["A"], x["B"], True,
                           **mp)[2]
    A = Arena("cuda")
    put = lambda t, name: A.put(t.cpu(), 1, name) if t is not None else None
    cm, ts = put(x["cmap"], "cmap"), put(x["tslope"], "tslope")
    lam, g1, g2 = put(x["lam"], "lam"), put(x["gam1"], "gam1"), put(x["gam2"], "gam2")
    u0, zp, za = put(us[0], "u"), put(x["zp"], "z_prev"), put(x["za"], "z_after")
    zdp, zda, ud = put(x["zdp"], "zd_prev"), put(x["zda"], "zd_after"), put(x["g_zd"], "ud")
    g2k = (lambda k: g2[k]) if both else (lambda k: None)
    g2r = (lambda k: x["gam2"][k]) if both else (lambda k: None)

    out = A.out(geom.code_shape(), 1, name="zd")
    o.prox_csr_tangent(geom, ud, u0, zp, lam[0], g1[0], za, g2k(0), zdp, zda, out=out, cmap=cm, tslope=ts[0])
    ref = o.prox_csr_tangent(geom, x["g_zd"], us[0], x["zp"], x["lam"][0], x["gam1"][0], x["za"], g2r(0), x["zdp"], x["zda"],
                             cmap=x["cmap"], tslope=x["tslope"][0])
    torch.cuda.synchronize()
    A.check()
    A.assert_defined(out)
    assert torch.equal(out, ref)

    out2 = A.out(geom.code_shape(), 1, name="zd2")
    o.analysis_prox_tangent(geom, x["vp"], x["A"][0], 1.0, None, u0, zp, lam[0], g1[0], za, g2k(0), zdp, zda, out=out2, cmap=cm,
                            tslope=ts[0])
    ref2 = o.analysis_prox_tangent(geom, x["vp"], x["A"][0], 1.0, None, us[0], x["zp"], x["lam"][0], x["gam1"][0], x["za"],
                                   g2r(0), x["zdp"], x["zda"], cmap=x["cmap"], tslope=x["tslope"][0])
    torch.cuda.synchronize()
    A.check()
    A.assert_defined(out2)
    assert torch.equal(out2, ref2)

    got = o.csr_tangent_forward(geom, x["vp"], x["mask"], lam, g1, g2 if both else None, zp, za, zdp, zda, x["A"], x["B"], us,
                                True, cmap=cm, tslope=ts)
    want = o.csr_tangent_forward(geom, x["vp"], x["mask"], x["lam"], x["gam1"], x["gam2"], x["zp"], x["za"], x["zdp"], x["zda"],
                                 x["A"], x["B"], us, True, **mp)
    torch.cuda.synchronize()
    A.check()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(p, q) for p, q in zip(got[2], want[2]))
