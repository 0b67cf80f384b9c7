"""Noise-level maps and data gradients of the CSR sweeps, kernel by kernel: the PROX + MAP epilogue of
the three analysis tiers, the map form of the reverse kernel against the element-wise broadcast form, and the one-call
sweeps against the stepwise loops."""
import functools

import pytest
import torch

from gpu_util import check, launch_sites
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

MFMA_TOL, FP32_TOL = 2e-5, 2e-6            # the tiers' tolerances of tests/test_gpu_dispatch.py
ENV = {
    "mfma": {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"},
    "tiled": {"CDL_MFMA_ANALYSIS": "0", "CDL_MFMA_SYNTHESIS": "0", "CDL_MFMA_WGRAD": "0", "CDL_MFMA_DENSE": "0"},
    "plain": {"CDL_NO_TILED": "1"},
}
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_ANA_T = "cdl_generic_tiled.hip:k_analysis_t<PW,SW,MAP>"
K_ANA_P = "cdl_generic.hip:k_analysis<true>"
# matrix cores: the two smallest keys that pass the 96-workgroup rule; the other tiers: the stride-padded extent of the
# 19 x 21 fixture (code grid 10 x 11) with P = 7, s = 2, and 20 x 24 with P = 5, s = 1
MFMA_KEYS = [(16, 1, 8, (60, 121), (5, 5), 1), (16, 1, 16, (120, 242), (9, 9), 2)]
SMALL_KEYS = [(2, 1, 5, (20, 22), (7, 7), 2), (2, 1, 5, (20, 24), (5, 5), 1)]


def ops():
    import cdlnet_video_amd as cva
    return cva.ops


def sigma_map(shape, gen):
    """A smooth noise-level map in [10, 40] / 255: a low-resolution random field, upsampled."""
    low = torch.rand(shape[:2] + tuple(max(2, d // 4) for d in shape[2:]), generator=gen)
    m = torch.nn.functional.interpolate(low, size=shape[2:], mode="bilinear", align_corners=True)
    return ((10.0 + 30.0 * m) / 255.0).contiguous()


@functools.lru_cache(maxsize=None)
def data(N, C, M, sp, P, s):
    """Seeded inputs of one geometry and the float64 analysis, computed once and shared by the tiers (read-only)."""
    g = torch.Generator().manual_seed(24)
    zsp = tuple(d // s for d in sp)
    code = lambda: 0.3 * torch.randn((N, M) + zsp, generator=g) * (torch.rand((N, M) + zsp, generator=g) > 0.5)
    d = {"x": torch.randn((N, C) + sp, generator=g), "w": torch.randn((M, C) + P, generator=g) * 0.2,
         "zin": code(), "zp": code(), "za": code(), "pad": tuple(p // 2 for p in P),
         "t0": [torch.rand(N, M, generator=g) * sc + 0.01 for sc in (0.2, 1.2, 1.2)],
         "tsl": torch.stack([torch.rand(M, generator=g) * sc for sc in (1.0, 4.0, 4.0)]),
         "cm": sigma_map((N, 1) + zsp, g)}
    d["u64"] = d["zin"].double() - O.analysis(d["x"].double(), d["w"].double(), s, d["pad"])
    return d


def fat(t0, cm, slope):
    """The threshold tensor torch's broadcast builds: t0[n,m] + cm[n,pix] * slope[m], the product rounded first."""
    return (t0[:, :, None, None] + cm * slope[None, :, None, None]).contiguous()


def run_epilogue(hip_env, tier, key, both, tol, site, **want):
    for k, v in ENV[tier].items():
        hip_env(k, v)
    o = ops()
    N, C, M, sp, P, s = key
    d = data(*key)
    geom = o.Geometry.make(N, C, M, sp, P, d["pad"], s)
    tag = f"csr map epilogue[{tier} {'f2' if both else 'f1'}] N{N}M{M}{sp}P{P}s{s}"
    cu = lambda t: t.cuda()
    zp, za, cm, tsl = cu(d["zp"]), cu(d["za"]) if both else None, cu(d["cm"]), cu(d["tsl"])
    lam0, g10, g20 = (cu(t) for t in d["t0"])
    u_out = torch.empty(geom.code_shape(), device="cuda")
    with o.trace() as t:
        z = o.analysis_prox(geom, cu(d["x"]), cu(d["w"]), -1.0, cu(d["zin"]), zp, lam0, g10, za, g20 if both else None,
                            u_out=u_out, cmap=cm, tslope=tsl)
    check(tag + " u", u_out, d["u64"], tol)
    ref = o.prox_csr_b(geom, u_out, zp, fat(lam0, cm, tsl[0]), fat(g10, cm, tsl[1]), za,
                       fat(g20, cm, tsl[2]) if both else None)
    assert torch.equal(z, ref), tag
    z2 = o.analysis_prox(geom, cu(d["x"]), cu(d["w"]), -1.0, cu(d["zin"]), zp, lam0, g10, za, g20 if both else None,
                         cmap=cm, tslope=tsl)                    # without u_out
    assert torch.equal(z2, ref), tag
    sites = launch_sites(t)
    recs = sites.get(site, [])
    ok = [r for r in recs if all({**r.values(), **r.template()}.get(k) == v for k, v in want.items())]
    if torch.cuda.get_device_properties(0).multi_processor_count == 256 or tier != "mfma":
        assert ok, f"{tag}: {site} {want}: got {[(r.template(), r.note) for r in recs] or sorted(sites)}"


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("key", MFMA_KEYS)
def test_prox_map_epilogue_matrix_core(key, both, hip_env):
    run_epilogue(hip_env, "mfma", key, both, MFMA_TOL, K_ANA, PROX=True, MAP=True, REV=False)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("key", SMALL_KEYS)
def test_prox_map_epilogue_tiled(key, both, hip_env):
    run_epilogue(hip_env, "tiled", key, both, FP32_TOL, K_ANA_T, MAP=True)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("key", SMALL_KEYS)
def test_prox_map_epilogue_plain(key, both, hip_env):
    run_epilogue(hip_env, "plain", key, both, FP32_TOL, K_ANA_P)


# ------------------------------------------------------------------------------------------ the reverse map kernel
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("M,sp", [(5, (37, 41)),      # per_m = 1517: no multiple of 256, two pixel chunks
                                  (5, (7, 9)),        # smaller than a workgroup
                                  (20, (7, 9))])      # three channel ranges of uneven length
def test_reverse_map_kernel_vs_broadcast_form(M, sp, both):
    """cdl_prox_csr_bwd with a map against cdl_prox_csr_b_bwd on the fat thresholds t0 + c * t1, whose element-wise
    threshold gradients are reduced here in float64."""
    o = ops()
    N = 2
    gen = torch.Generator().manual_seed(M + sp[0] + both)
    geom = o.Geometry.make(N, 1, M, sp, (1, 1), (0, 0), 1)
    rnd = lambda sc=1.0: (sc * torch.randn(geom.code_shape(), generator=gen)).cuda()
    sparse = lambda: (0.3 * torch.randn(geom.code_shape(), generator=gen)
                      * (torch.rand(geom.code_shape(), generator=gen) > 0.5)).cuda()
    gz, u, zp, za = rnd(), rnd(0.5), sparse(), sparse() if both else None
    lam0, g10, g20 = ((torch.rand(N, M, generator=gen) * sc + 0.01).cuda() for sc in (0.2, 1.2, 1.2))
    tsl = torch.stack([torch.rand(M, generator=gen) * sc for sc in (1.0, 4.0, 4.0)]).cuda()
    cm = sigma_map((N, 1) + sp, gen).cuda()
    seed_p, seed_a, seed_c = rnd(0.1), rnd(0.1), (0.1 * torch.randn(cm.shape, generator=gen)).cuda()
    fl, f1, f2 = fat(lam0, cm, tsl[0]), fat(g10, cm, tsl[1]), fat(g20, cm, tsl[2]) if both else None

    rp, ra = seed_p.clone(), seed_a.clone() if both else None
    gu_r, dl, d1, d2 = o.prox_csr_b_bwd(geom, gz, u, zp, fl, f1, za, f2, gz_prev=rp, gz_after=ra)
    els = [dl.double(), d1.double()] + ([d2.double()] if both else [])
    ref_dt = [torch.stack([e.sum((0, 2, 3)), (cm.double() * e).sum((0, 2, 3))]) for e in els]
    ref_dc = seed_c.double() + sum((tsl[i].double()[None, :, None, None] * e).sum(1, keepdim=True)
                                   for i, e in enumerate(els))

    def run():
        gp, ga, dc = seed_p.clone(), seed_a.clone() if both else None, seed_c.clone()
        dts = [torch.full((2, M), float("nan"), device="cuda") for _ in els]
        gu = o.prox_csr_bwd(geom, gz, u, zp, lam0, g10, None, dts[0], dts[1], za, g20 if both else None,
                            dts[2] if both else None, gp, ga, cmap=cm, tslope=tsl, dcmap=dc)
        return [gu, gp, ga, dc] + dts

    got, again = run(), run()
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)          # fixed-order reductions
    tag = f"csr map reverse[{'f2' if both else 'f1'}] M{M}{sp}"
    check(tag + " gu", got[0], gu_r, 1e-6)
    check(tag + " gz_prev", got[1], rp, 1e-5)
    if both:
        check(tag + " gz_after", got[2], ra, 1e-5)
    check(tag + " dcmap", got[3], ref_dc, 2e-5)
    for name, a, b in zip(("dt", "dg1", "dg2"), got[4:], ref_dt):
        check(f"{tag} {name}", a, b, 2e-5)
    # without dcmap the other outputs are the same bits
    gp = seed_p.clone()
    dts = [torch.empty(2, M, device="cuda") for _ in els]
    gu = o.prox_csr_bwd(geom, gz, u, zp, lam0, g10, None, dts[0], dts[1], za, g20 if both else None,
                        dts[2] if both else None, gp, None, cmap=cm, tslope=tsl)
    assert torch.equal(gu, got[0]) and torch.equal(gp, got[1]) and all(torch.equal(a, b) for a, b in zip(dts, got[4:]))


# ------------------------------------------------------------------------------------------ whole-sweep C calls
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("dims,P,s,C,M,masked", [((24, 40), (5, 5), 1, 1, 11, False), ((22, 18), (7, 7), 2, 3, 9, True)])
def test_csr_sweeps_with_map_and_data_gradients_equal_stepwise(dims, P, s, C, M, masked, mapped):
    """cdl_ista_forward / cdl_ista_backward on the CSR branch with a noise-level map (dyp, dcmap) and without one (dyp and
    the per-sample threshold sums) against the stepwise Python loops."""
    from cdlnet_video_amd import loop
    o = ops()
    gen = torch.Generator().manual_seed(sum(dims) + M + mapped)
    N, K = 2, 3
    geom = o.Geometry.make(N, C, M, dims, P, tuple(p // 2 for p in P), s)
    rnd = lambda shape, sc=1.0: (sc * torch.randn(shape, generator=gen)).cuda()
    yp = rnd(geom.image_shape())
    mask = (torch.rand(geom.image_shape(), generator=gen) > 0.3).float().cuda() if masked else None
    A = [rnd(geom.filter_shape(), 0.08) for _ in range(K)]
    B = [rnd(geom.filter_shape(), 0.08) for _ in range(K)]
    t, g1, g2 = ((torch.rand(K, 2, M, 1, 1, generator=gen) * sc).cuda() for sc in (0.05, 1.0, 1.0))
    c = torch.rand(N, generator=gen).cuda()
    cm = (255.0 / 40.0 * sigma_map((N, 1) + geom.code_spatial, gen)).cuda()        # in [0.25, 1], as c
    g_xp, g_z = rnd(geom.image_shape()), rnd(geom.code_shape(), 0.1)
    zp, za = rnd(geom.code_shape(), 0.2), rnd(geom.code_shape(), 0.2)
    cs = None if mapped else c
    lam, gam1, gam2 = (o.thresholds(p, cs, N) for p in (t, g1, g2))
    for zaft, gm2, p2 in ((None, None, None), (za, gam2, g2)):
        tag = f"csr sweep[{'map' if mapped else 'c'} {'f2' if zaft is not None else 'f1'} mask={masked}] {dims}s{s}"
        mp = dict(cmap=cm, tslope=loop._csr_slopes(t, g1, p2)) if mapped else {}
        a = loop._forward_csr(geom, yp, mask, lam, gam1, gm2, zp, zaft, A, B, True, **mp)
        b = loop._forward_csr_stepwise(geom, yp, mask, lam, gam1, gm2, zp, zaft, A, B, True, **mp)
        check(tag + " xp", a[0], b[0], 1e-6)
        for name, la, lb in zip(("u", "z", "r"), a[2:], b[2:]):
            assert len(la) == len(lb)
            for k, (x, y) in enumerate(zip(la, lb)):
                check(f"{tag} {name}{k}", x, y, 1e-6)
        inf = loop._forward_csr(geom, yp, mask, lam, gam1, gm2, zp, zaft, A, B, False, **mp)
        assert torch.equal(inf[0], a[0]) and torch.equal(inf[1], a[1])

        outs = []
        for fn, f in ((loop._backward_csr, a), (loop._backward_csr_stepwise, b)):
            dt, dg1, dg2 = (torch.zeros(K, 2, M, device="cuda") for _ in range(3))
            gzp, gza = torch.zeros_like(zp), torch.zeros_like(zp) if zaft is not None else None
            dyp = torch.empty(geom.image_shape(), device="cuda")
            dtau = None if mapped else torch.zeros(K, 3, N, M, device="cuda")
            bm = dict(mp, dcmap=torch.empty_like(cm)) if mapped else {}
            dA, dB = fn(geom, K, yp, mask, cs, A, B, f[3], f[4], f[2], zp, zaft, lam, gam1, gm2, g_xp, g_z, dt, dg1,
                        dg2 if zaft is not None else None, gzp, gza, dyp=dyp, dtau=dtau, **bm)
            outs.append(dict(dt=dt, dg1=dg1, dg2=dg2, gzp=gzp, gza=gza, dyp=dyp, dtau=dtau, dcmap=bm.get("dcmap"),
                             **{f"dA{k}": w for k, w in enumerate(dA)}, **{f"dB{k}": w for k, w in enumerate(dB)}))
        for name, x in outs[0].items():
            if x is not None:
                check(f"{tag} {name}", x, outs[1][name], 1e-6)
        if not mapped:                                   # the per-sample sums against the folded parameter gradients
            dtau = outs[0]["dtau"]
            for f, name in enumerate(("dt", "dg1", "dg2")[:3 if zaft is not None else 2]):
                check(f"{tag} sum_n dtau vs {name}[:,0]", dtau[:, f].sum(1), outs[0][name][:, 0], 1e-5)
                check(f"{tag} sum_n c dtau vs {name}[:,1]", torch.einsum("knm,n->km", dtau[:, f], c), outs[0][name][:, 1], 1e-5)
        # with no data gradient asked for, the parameter outputs are the bits of the plain call
        dt, dg1, dg2 = (torch.zeros(K, 2, M, device="cuda") for _ in range(3))
        gzp = torch.zeros_like(zp)
        dA, dB = loop._backward_csr(geom, K, yp, mask, cs, A, B, a[3], a[4], a[2], zp, zaft, lam, gam1, gm2, g_xp, g_z, dt,
                                    dg1, dg2 if zaft is not None else None, gzp, None, **mp)
        assert torch.equal(dt, outs[0]["dt"]) and torch.equal(dg1, outs[0]["dg1"]) and torch.equal(gzp, outs[0]["gzp"])
        assert all(torch.equal(x, outs[0][f"dA{k}"]) for k, x in enumerate(dA))
