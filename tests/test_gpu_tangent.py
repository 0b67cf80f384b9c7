"""net.jvp -- the forward-mode tangent sweeps at the primal's supports (loop.TangentISTA) -- and the
exact SURE objective built on it: against the float64 oracle at identical support on every tier the router picks
(tangent_util: ista(y + v; supports) - ista(y; supports) and its autograd), and the properties the feature promises.
Case builder, shapes and tolerances are those of tests/test_gpu_datagrad.py (the smallest shapes that reach each route)."""
import pytest
import torch

from gpu_util import build_from_golden, check, hyper, launch_sites, load_golden, log
from oracle import cdl_oracle as O
from tangent_util import code_density, tangent_and_grads
from test_gpu_datagrad import FP32_TOL, SPLIT_TOL, _case, _geom, _supports

pytestmark = pytest.mark.gpu

FUSED_FILES = {"cdl_fused2d.hip", "cdl_fusedg.hip", "cdl_strip.hip", "cdl_stripg.hip"}


def _oracle_kw(net, y, sigma, mask):
    A0 = net.A[0].weight
    nd = y.dim() - 2
    P = tuple(A0.shape[2:]) if nd == 3 else A0.shape[-1]
    return dict(K=len(net.A), P=P, s=net.s, sigma=sigma, adaptive=True, mask=mask, ndim=nd)


def _direction(y, mask, seed):
    gen = torch.Generator().manual_seed(seed)
    v, w1, w2 = (torch.randn(y.shape, generator=gen) for _ in range(3))
    return (mask * v if mask is not None else v), w1, w2


def _grads(net):
    return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


def _vs_oracle(tag, net, sd, x, y, sigma, mask, tol, sigma_dev=None, supports=None):
    """xdot and every parameter gradient of mean(w1 xdot) + mean(w2 xhat) + mse against the oracle at the device's own
    supports; xhat bit-identical to the plain forward; t.grad = the gradient of the xhat terms alone."""
    sig = sigma.cuda() if sigma_dev is None else sigma_dev
    m = mask.cuda() if mask is not None else 1
    if supports is None:
        supports = _supports(net, y, sigma, mask)
    dens = code_density(supports)
    log(f"tangent {tag}: code densities {['%.2f' % d for d in dens]}")
    assert all(0.10 < d < 0.90 for d in dens), dens            # both gate values are exercised in every code
    v, w1, w2 = _direction(y, mask, 41)
    net.zero_grad(set_to_none=True)
    xhat, xdot = net.jvp(y.cuda(), v.cuda(), sig, mask=m)
    xc = x.cuda()
    (torch.mean(w1.cuda() * xdot) + torch.mean(w2.cuda() * xhat) + torch.mean((xhat - xc) ** 2)).backward()
    got = _grads(net)
    with torch.no_grad():
        plain, _ = net(y.cuda(), sig, mask=m)
    assert torch.equal(xhat, plain), f"{tag}: jvp's xhat is not the forward's"
    net.zero_grad(set_to_none=True)
    xh2, _ = net(y.cuda(), sig, mask=m)
    (torch.mean(w2.cuda() * xh2) + torch.mean((xh2 - xc) ** 2)).backward()
    assert torch.equal(got["t"], net.t.grad), f"{tag}: t.grad must come from the xhat terms alone"

    x64, w164, w264 = x.double(), w1.double(), w2.double()
    loss_fn = lambda xh, xd: torch.mean(w164 * xd) + torch.mean(w264 * xh) + torch.mean((xh - x64) ** 2)
    xo, xdo, _, ref = tangent_and_grads(sd, y, v, supports, loss_fn, **_oracle_kw(net, y, sigma, mask))
    check(f"tangent {tag} xhat", xhat, xo, 1e-5)
    check(f"tangent {tag} xdot", xdot, xdo, tol)
    for name, gr in got.items():
        if name != "g":
            check(f"tangent {tag} grad {name}", gr, ref[name], tol)
    return xhat.detach(), xdot.detach()


# ------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("layout", ["nchw", "blocked"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,shape", [(32, (2, 1, 48, 40)), (64, (2, 1, 45, 39))])
def test_fused2d_vs_oracle(layout, masked, M, shape):
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, sigma, mask, w = _case("2d", 11, shape, 1, masked, K=4, M=M, P=7)
    assert ops.fused_supported(_geom(net, y, 1))
    saved = loop.CODE_LAYOUT
    loop.set_code_layout(layout)
    try:
        _vs_oracle(f"fused2d {layout} M{M} {shape} mask={masked}", net, sd, x, y, sigma, mask, SPLIT_TOL)
    finally:
        loop.set_code_layout(saved)


def test_fused2d_split4_and_fp32_scope_vs_oracle():
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, sigma, mask, w = _case("2d", 12, (2, 1, 40, 36), 1, True, K=3, M=32, P=5)
    assert ops.fused_supported(_geom(net, y, 1))
    with loop.precision_scope("split4"):
        _vs_oracle("fused2d split4", net, sd, x, y, sigma, mask, SPLIT_TOL)
    with loop.precision_scope("fp32"):            # no fused kernels: the generic tangent sweep on the fp32 VALU kernels
        _vs_oracle("fp32 scope", net, sd, x, y, sigma, mask, FP32_TOL)
    # four products at M = 64 in the default blocked layout (split4 ran at M = 32 only)
    net, sd, x, y, sigma, mask, w = _case("2d", 13, (2, 1, 45, 39), 1, True, K=4, M=64, P=7)
    assert ops.fused_supported(_geom(net, y, 1)) and loop.CODE_LAYOUT == "blocked"
    with loop.precision_scope("split4"):
        _vs_oracle("fused2d split4 M64 blocked", net, sd, x, y, sigma, mask, SPLIT_TOL)


@pytest.mark.parametrize("label,kind,shape,s,masked,kw", [
    ("fusedg 2-D C3 bayer", "2d", (2, 3, 24, 28), 1, "bayer", dict(K=3, M=32, P=7)),
    ("fusedg 3-D cfg3-like", "3d", (1, 1, 6, 24, 40), 1, False, dict(K=3, M=16, P=[3, 5, 5])),
    ("fusedg 3-D odd", "3d", (2, 1, 7, 13, 11), 1, False, dict(K=2, M=16, P=[3, 5, 5])),
])
def test_fusedg_vs_oracle(label, kind, shape, s, masked, kw):
    from cdlnet_video_amd import ops
    net, sd, x, y, sigma, mask, w = _case(kind, 13, shape, s, masked, **kw)
    g = _geom(net, y, s)
    assert ops.fusedg_supported(g) and not ops.fused_supported(g)
    _vs_oracle(label, net, sd, x, y, sigma, mask, SPLIT_TOL)


@pytest.mark.parametrize("shape", [(2, 1, 50, 78), (2, 1, 49, 77)])
def test_strip_route_vs_oracle(shape):
    from cdlnet_video_amd import ops
    net, sd, x, y, sigma, mask, w = _case("2d", 14, shape, 2, False, K=3, M=96, P=7)
    g = _geom(net, y, 2)
    assert ops.fusedg_supported(g) and not ops.fused_supported(g)
    _vs_oracle(f"strip {shape}", net, sd, x, y, sigma, mask, SPLIT_TOL)


def test_generic_3d_s2_p9_vs_oracle():
    """M = 16, not the M = 5 test_gpu_datagrad runs this geometry with: at stride 2 in 3-D a code has M / 8 entries per
    pixel, so M = 5 is an undercomplete dictionary whose codes cannot be sparse.  The float64 oracle's own codes are
    89 % / 91 % non-zero there whatever the seed (15..39), outside the 10-90 % this file demands of every case; they fall
    as M grows (8: 87 / 88 %, 16: 84 / 86 %, 32: 81 / 80 %).  M = 16 is twice overcomplete and routes to the same
    generic kernels."""
    from cdlnet_video_amd import ops
    net, sd, x, y, sigma, mask, w = _case("3d", 15, (2, 1, 8, 20, 12), 2, False, K=2, M=16, P=[9, 9, 5])
    g = _geom(net, y, 2)
    assert not ops.fusedg_supported(g) and not ops.fused_supported(g)
    _vs_oracle("generic 3-D s2 P9", net, sd, x, y, sigma, mask, SPLIT_TOL)


@pytest.mark.parametrize("masked", [False, True])
def test_generic_backend_2d_vs_oracle(masked):
    from cdlnet_video_amd import loop
    net, sd, x, y, sigma, mask, w = _case("2d", 16, (2, 1, 33, 31), 2, masked, K=3, M=16, P=7)
    loop.set_backend("generic")
    try:
        _vs_oracle(f"generic backend 2-D mask={masked}", net, sd, x, y, sigma, mask, SPLIT_TOL)
    finally:
        loop.set_backend("auto")


def test_sigma_map_runs_the_generic_tangent_vs_oracle():
    """A (N,1,Hc,Wc) noise-level map on a fused 2-D geometry: the primal runs the generic sweep with the map, the tangent
    the generic tangent sweep (no threshold, hence no map, appears in it)."""
    from cdlnet_video_amd import ops
    net, sd, x, y, _, mask, w = _case("2d", 18, (2, 1, 48, 40), 1, False, K=4, M=32, P=7)
    assert ops.fused_supported(_geom(net, y, 1))
    smap = 15.0 + 20.0 * torch.rand((2, 1, 48, 40), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        outs = net._run(y.cuda(), smap.cuda(), 1, True)
    supports = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
    with ops.trace() as t:
        _vs_oracle("sigma map (generic)", net, sd, x, y, smap, mask, SPLIT_TOL, supports=supports)
        torch.cuda.synchronize()
    assert not (t.files() & FUSED_FILES), t.files()


# ------------------------------------------------------------------------------------------ fixtures of the reference
@pytest.mark.parametrize("name,kind", [("j1_2d_s2_odd", "2d"), ("j2_jdd_c3_mask", "2d"), ("j3_3d_p555", "3d")])
def test_jvp_matches_the_reference_fixtures(name, kind):
    """xdot and the gradients of mean(w xdot) + mean((xhat - y)^2) against the unmodified reference under forward-mode
    autograd, at the f-fixture gradient tolerance on the fp32 tier (whose supports must agree with the reference's: a
    flipped near-tie moves xdot by a P x P patch)."""
    from cdlnet_video_amd import loop
    g = load_golden(name)
    net = build_from_golden(g, kind)
    K, M, P, s, C = hyper(g)
    sigma = g["sigma"].cuda() if torch.is_tensor(g["sigma"]) else g["sigma"]
    mask = g["mask"].cuda() if "mask" in g else 1
    with torch.no_grad():
        _, ref_codes = O.ista(g["sd"], g["y"], K=K, P=P, s=s, sigma=g["sigma"], adaptive=True, mask=g.get("mask"),
                              ndim=g["y"].dim() - 2, all_codes=True)
    with loop.precision_scope("fp32"):
        with torch.no_grad():
            outs = net._run(g["y"].cuda(), sigma, mask, True)
        codes = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
        assert sum(int(((a != 0) != (b != 0)).sum()) for a, b in zip(codes, ref_codes)) == 0
        xhat, xdot = net.jvp(g["y"].cuda(), g["v"].cuda(), sigma, mask=mask)
        loss = torch.mean(g["w"].cuda() * xdot) + torch.mean((xhat - g["y"].cuda()) ** 2)
    loss.backward()
    assert abs(loss.item() - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"])) + 1e-8
    check(f"{name} xhat", xhat, g["xhat"], 1e-5)
    check(f"{name} xdot", xdot, g["xdot"], 2e-4)
    for pname, ref in g["grad"].items():
        check(f"{name} grad {pname}", dict(net.named_parameters())[pname].grad, ref, 2e-4)


# ------------------------------------------------------------------------------------------ properties
PROPERTY_CASES = {
    "fused2d": ("2d", (2, 1, 48, 40), 1, True, dict(K=4, M=32, P=7)),
    "fusedg": ("2d", (2, 3, 24, 28), 1, "bayer", dict(K=3, M=32, P=7)),
    "strip": ("2d", (2, 1, 50, 78), 2, False, dict(K=3, M=96, P=7)),
    "generic": ("3d", (2, 1, 8, 20, 12), 2, False, dict(K=2, M=16, P=[9, 9, 5])),     # M: test_generic_3d_s2_p9_vs_oracle
}


@pytest.mark.parametrize("tier", list(PROPERTY_CASES))
def test_linearity_repeatability_and_no_grad(tier):
    kind, shape, s, masked, kw = PROPERTY_CASES[tier]
    net, sd, x, y, sigma, mask, w = _case(kind, 23, shape, s, masked, **kw)
    yd, sg, m = y.cuda(), sigma.cuda(), (mask.cuda() if mask is not None else 1)
    v1, v2, _ = _direction(y, mask, 7)
    v1, v2 = v1.cuda(), v2.cuda()
    a, b = 0.5, -2.0
    with torch.no_grad():
        xh1, d1 = net.jvp(yd, v1, sg, mask=m)
        xh2, d2 = net.jvp(yd, v2, sg, mask=m)
        xh3, d3 = net.jvp(yd, a * v1 + b * v2, sg, mask=m)
        _, d1_again = net.jvp(yd, v1, sg, mask=m)
    assert torch.equal(xh1, xh2) and torch.equal(xh1, xh3)              # the primal does not see v
    assert torch.equal(d1, d1_again)                                    # repeated calls: bit for bit
    # each of the three tangents is within `tol` (of its own maximum) of the exact linear map J, so the identity holds
    # to (1 + |a| + |b|) tol of the largest of them
    tol = SPLIT_TOL * (1 + abs(a) + abs(b))
    check(f"tangent {tier} linearity in v", d3, a * d1 + b * d2, tol)
    xh_g, d1_g = net.jvp(yd, v1, sg, mask=m)                             # grad enabled: codes kept, same launches
    assert xh_g.requires_grad and d1_g.requires_grad
    assert torch.equal(xh_g, xh1) and torch.equal(d1_g, d1)
    assert float(d1.abs().max()) > 0


@pytest.mark.parametrize("tier", list(PROPERTY_CASES))
def test_adjoint_identity_with_the_data_gradient(tier):
    """<w, J v> = <J^T w, v>, J^T w from the existing dL/dy path of the reverse sweeps."""
    kind, shape, s, masked, kw = PROPERTY_CASES[tier]
    net, sd, x, y, sigma, mask, w = _case(kind, 24, shape, s, masked, **kw)
    sg, m = sigma.cuda(), (mask.cuda() if mask is not None else 1)
    v, w1, _ = _direction(y, mask, 9)
    v, w1 = v.cuda(), w1.cuda()
    with torch.no_grad():
        _, xdot = net.jvp(y.cuda(), v, sg, mask=m)
    yg = y.cuda().requires_grad_(True)
    xhat, _ = net(yg, sg, mask=m)
    (jtw,) = torch.autograd.grad((w1 * xhat).sum(), (yg,))
    lhs, rhs = float((w1.double() * xdot.double()).sum()), float((jtw.double() * v.double()).sum())
    bound = SPLIT_TOL * float(w1.double().norm()) * float(xdot.double().norm())
    log(f"tangent {tier} adjoint identity: <w,Jv>={lhs:.6e} <JTw,v>={rhs:.6e} |diff|={abs(lhs - rhs):.3e} bound={bound:.3e}")
    assert abs(lhs - rhs) <= bound


def _sweep_inputs(masked, layout, seed=21, K=3, M=32, P=7, shape=(2, 1, 40, 36)):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    net, sd, x, y, sigma, mask, w = _case("2d", seed, shape, 1, masked, K=K, M=M, P=P)
    yp, mean, pads, mask_p = o.preprocess(y.cuda(), 1, mask.cuda() if mask is not None else None)
    v, _, _ = _direction(y, mask, 3)
    vp = o.preprocess(v.cuda(), 1, mask.cuda() if mask is not None else None)[0]
    g = o.Geometry.make(shape[0], 1, M, yp.shape[2:], (P, P), (P // 2, P // 2), 1)
    tau = o.thresholds(net.t.detach(), (sigma.reshape(-1) / 255.0).cuda(), shape[0])
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    xp, z, codes, resid, maps = loop._forward_fused(g, yp, mask_p, tau, A, B, True, True, layout=layout)
    g_xp = torch.randn(xp.shape, generator=torch.Generator().manual_seed(8)).cuda()
    return g, K, vp, mask_p, A, B, codes, maps, g_xp


@pytest.mark.parametrize("layout", ["nchw", "blocked"])
@pytest.mark.parametrize("masked", [False, True])
def test_fused_stepwise_equals_the_c_sweep_and_launches_only_its_file(masked, layout):
    from cdlnet_video_amd import loop, ops
    g, K, vp, mask_p, A, B, codes, maps, g_xp = _sweep_inputs(masked, layout)
    with ops.trace() as t:
        xdp, zd, nrd = loop._tangent_fused(g, vp, mask_p, A, B, maps, True, layout=layout)
        torch.cuda.synchronize()
    assert t.files() == {"cdl_fused2d.hip"}, t.files()
    sites = launch_sites(t)
    count = lambda key: sum(len(r) for sid, r in sites.items() if key in sid)
    assert count("k_stage") == K and count("k_assemble") == K, {sid: len(r) for sid, r in sites.items()}
    xs, zs, ns = loop._tangent_fused_stepwise(g, vp, mask_p, A, B, maps, True, layout=layout)
    assert torch.equal(xdp, xs)
    nchw = lambda codes: [ops.fused_to_nchw(g, c, layout) for c in codes[:-1]] + [codes[-1]]    # image pixels only
    assert all(torch.equal(a, b) for a, b in zip(nchw(zd) + list(nrd), nchw(zs) + list(ns)))
    x0, z0, n0 = loop._tangent_fused(g, vp, mask_p, A, B, maps, False, layout=layout)       # ping-pong buffers
    assert torch.equal(x0, xdp) and z0 == [] and n0 == []


@pytest.mark.parametrize("M,P", [(32, 5), (64, 7)])
@pytest.mark.parametrize("precision", ["split3", "bf16", "split4"])
@pytest.mark.parametrize("layout", ["nchw", "blocked"])
def test_fused_tangent_sweep_in_every_arithmetic(layout, precision, M, P):
    """The tangent sweep's stages are non-riding reverse stages in the sweep's layout (with plain-bf16 arithmetic, blocked
    storage and M = 64 the instance of DESIGN.md section 6b): in every arithmetic the C sweep equals the step-wise launches
    bit for bit, and run twice it is bit-identical."""
    from cdlnet_video_amd import loop, ops
    with loop.precision_scope(precision):
        g, K, vp, mask_p, A, B, codes, maps, g_xp = _sweep_inputs(True, layout, M=M, P=P)
        with ops.trace() as t:
            xdp, zd, nrd = loop._tangent_fused(g, vp, mask_p, A, B, maps, True, layout=layout)
            torch.cuda.synchronize()
        xd2, zd2, nrd2 = loop._tangent_fused(g, vp, mask_p, A, B, maps, True, layout=layout)
        xs, zs, ns = loop._tangent_fused_stepwise(g, vp, mask_p, A, B, maps, True, layout=layout)
    assert t.files() == {"cdl_fused2d.hip"}, t.files()
    stages = [r.template() for sid, recs in launch_sites(t).items() if "k_stage<" in sid for r in recs]
    assert len(stages) == K and all((tp["MT"], tp["PREC"], tp["MODE"], tp["WY"]) == (M // 32, ops.PRECISION[precision], 2, 2)
                                    for tp in stages), stages
    log(f"tangent sweep {layout} {precision} M{M}P{P}: MT={M // 32} PREC={ops.PRECISION[precision]} (LIN, LOUT) launched "
        f"{[(tp['LIN'], tp['LOUT']) for tp in stages]}")
    nchw = lambda codes: [ops.fused_to_nchw(g, c, layout) for c in codes[:-1]] + [codes[-1]]    # image pixels only
    first = [xdp] + nchw(zd) + list(nrd)
    assert all(torch.equal(a, b) for a, b in zip(first, [xd2] + nchw(zd2) + list(nrd2))), "the sweep does not repeat itself"
    assert all(torch.equal(a, b) for a, b in zip(first, [xs] + nchw(zs) + list(ns))), "sweep and step-wise launches differ"


def test_bf16_arithmetic_m64_blocked_is_reproducible_through_the_net():
    """Plain-bf16 arithmetic with the default blocked storage at M = 64: net.jvp plus backward, and a training backward, give
    the same bits in a second call (what the arithmetic computes is held cell by cell in test_gpu_fused_cells.py)."""
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, sigma, mask, w = _case("2d", 14, (2, 1, 45, 39), 1, True, K=4, M=64, P=7)
    assert ops.fused_supported(_geom(net, y, 1)) and loop.CODE_LAYOUT == "blocked"
    v, w1, w2 = _direction(y, mask, 43)
    yc, sc, mc, xc = y.cuda(), sigma.cuda(), mask.cuda(), x.cuda()

    def jvp_step():
        net.zero_grad(set_to_none=True)
        xhat, xdot = net.jvp(yc, v.cuda(), sc, mask=mc)
        (torch.mean(w1.cuda() * xdot) + torch.mean((xhat - xc) ** 2)).backward()
        return [xhat.detach(), xdot.detach()] + [gr.clone() for _, gr in sorted(_grads(net).items())]

    def train_step():
        net.zero_grad(set_to_none=True)
        xhat, _ = net(yc, sc, mask=mc)
        torch.mean((xhat - xc) ** 2).backward()
        return [xhat.detach()] + [gr.clone() for _, gr in sorted(_grads(net).items())]

    with loop.precision_scope("bf16"):
        for step in (jvp_step, train_step):
            with ops.trace() as t:
                a = step()
                torch.cuda.synchronize()
            b = step()
            stages = [r.template() for sid, recs in launch_sites(t).items() if "cdl_fused2d.hip:k_stage<" in sid for r in recs]
            assert stages and all(tp["PREC"] == 1 and tp["MT"] == 2 for tp in stages), stages
            assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b)), step.__name__


@pytest.mark.parametrize("masked", [False, True])
def test_generic_stepwise_equals_the_c_sweeps_and_launches_no_fused_file(masked):
    from cdlnet_video_amd import loop, ops
    g, K, vp, mask_p, A, B, codes, maps, g_xp = _sweep_inputs(masked, "nchw")
    with ops.trace() as t:
        xdp, zd, rd = loop._tangent_generic(g, vp, mask_p, A, B, codes, True)
        dA, dB = loop._tangent_backward_generic(g, K, vp, mask_p, A, B, codes, zd, rd, g_xp)
        torch.cuda.synchronize()
    assert t and not (t.files() & FUSED_FILES), t.files()
    xs, zs, rs = loop._tangent_generic_stepwise(g, vp, mask_p, A, B, codes, True)
    assert torch.equal(xdp, xs)
    assert all(torch.equal(a, b) for a, b in zip(list(zd) + list(rd), list(zs) + list(rs)))
    sA, sB = loop._tangent_backward_generic_stepwise(g, K, vp, mask_p, A, B, codes, zs, rs, g_xp)
    assert all(torch.equal(a, b) for a, b in zip(list(dA) + list(dB), list(sA) + list(sB)))
    # the fused sweep computes the same tangent: its negated residuals are the generic sweep's, to the tiers' tolerance
    xf, zf, nf = loop._tangent_fused(g, vp, mask_p, A, B, maps, True, layout="nchw")
    check(f"fused vs generic tangent xdp mask={masked}", xf, xdp, SPLIT_TOL)
    check(f"fused vs generic tangent -rd_1 mask={masked}", nf[0], -rd[0], SPLIT_TOL)


@pytest.mark.parametrize("tier,files", [("fusedg", {"cdl_fusedg.hip"}), ("strip", {"cdl_fusedg.hip", "cdl_strip.hip", "cdl_stripg.hip"}),
                                        ("generic", None)])
def test_routes_launch_their_own_files(tier, files):
    """jvp under no_grad, the primal included: the fused routes launch only their own files (plus the thin pre / post
    processing), the generic route no fused file; the fused tangent: K stage launches and K assembles on top of the
    primal's K + K."""
    from cdlnet_video_amd import ops
    kind, shape, s, masked, kw = PROPERTY_CASES[tier]
    net, sd, x, y, sigma, mask, w = _case(kind, 25, shape, s, masked, **kw)
    v, _, _ = _direction(y, mask, 2)
    K = kw["K"]
    with torch.no_grad(), ops.trace() as t:
        net.jvp(y.cuda(), v.cuda(), sigma.cuda(), mask=mask.cuda() if mask is not None else 1)
        torch.cuda.synchronize()
    fused = t.files() & FUSED_FILES
    if files is None:
        assert not fused, fused
        return
    assert fused and fused <= files, t.files()
    if tier == "strip":
        assert fused & {"cdl_strip.hip", "cdl_stripg.hip"}
    sites = launch_sites(t)
    count = lambda keys: sum(len(r) for sid, r in sites.items() if any(k in sid for k in keys))
    assert count(("k_stage_g", "k_strip")) == 2 * K and count(("k_assemble",)) == 2 * K, \
        {sid: len(r) for sid, r in sites.items()}


def test_a_missing_upstream_gradient_skips_its_sweep():
    """A loss on xdot alone launches no primal reverse sweep (t.grad is zero), a loss on xhat alone gives the plain
    forward's gradients bit for bit; the two add up to the joint loss's gradients."""
    kind, shape, s, masked, kw = PROPERTY_CASES["fused2d"]
    net, sd, x, y, sigma, mask, w = _case(kind, 26, shape, s, masked, **kw)
    yd, sg, m = y.cuda(), sigma.cuda(), mask.cuda()
    v, w1, w2 = (t.cuda() for t in _direction(y, mask, 4))

    def grads(use_hat, use_dot):
        net.zero_grad(set_to_none=True)
        xhat, xdot = net.jvp(yd, v, sg, mask=m)
        loss = (torch.mean(w2 * xhat) if use_hat else 0.0) + (torch.mean(w1 * xdot) if use_dot else 0.0)
        loss.backward()
        return _grads(net)

    both, hat, dot = grads(True, True), grads(True, False), grads(False, True)
    assert float(dot["t"].abs().max()) == 0.0
    net.zero_grad(set_to_none=True)
    xh, _ = net(yd, sg, mask=m)
    torch.mean(w2 * xh).backward()
    plain = _grads(net)
    for n in plain:
        assert torch.equal(hat[n], plain[n]), n
        if n != "t":
            assert torch.equal(both[n], hat[n] + dot[n]), n
    assert torch.equal(both["t"], hat["t"])


def test_bucket_syncs_once_per_backward():
    from cdlnet_video_amd import loop
    kind, shape, s, masked, kw = PROPERTY_CASES["fused2d"]
    net, sd, x, y, sigma, mask, w = _case(kind, 27, shape, s, masked, **kw)
    v, w1, w2 = (t.cuda() for t in _direction(y, mask, 4))
    calls = []
    remove = loop.on_backward_end(lambda: calls.append(1))
    try:
        xhat, xdot = net.jvp(y.cuda(), v, sigma.cuda(), mask=mask.cuda())
        (torch.mean(w1 * xdot) + torch.mean(w2 * xhat)).backward()
    finally:
        remove()
    assert calls == [1]


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device():
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    x = cva.utils.synthetic_clip((1, 1, 24, 24), seed=1).cuda()
    v = torch.ones_like(x)
    net = cva.CDLNet(K=2, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    for bad in (dict(v=v.clone().requires_grad_(True)), dict(y=x.clone().requires_grad_(True)),
                dict(sigma=torch.tensor(25.0, device="cuda", requires_grad=True)),
                dict(mask=torch.ones_like(x).requires_grad_(True))):
        args = dict(y=x, v=v, sigma=25.0, mask=1)
        args.update(bad)
        with pytest.raises(NotImplementedError, match="requires grad"):
            net.jvp(args["y"], args["v"], args["sigma"], mask=args["mask"])
    with pytest.raises(ValueError, match="shape"):
        net.jvp(x, v[..., :-1], 25.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        net.jvp(x, v.cpu(), 25.0)
    saved = loop.CODE_LAYOUT
    loop.set_code_layout("blocked_bf16")
    try:
        with pytest.raises(NotImplementedError, match="blocked_bf16"):
            net.jvp(x, v, 25.0)
    finally:
        loop.set_code_layout(saved)
    csr = cva.CDLNet_CSR(K=2, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    with pytest.raises(NotImplementedError, match="CSR"):
        csr.jvp(x, v, 25.0)
    xv = cva.utils.synthetic_clip((1, 1, 4, 16, 16), seed=2).cuda()
    vid = cva.CDLNetVideo(K=2, M=8, P=[3, 3, 3], s=1, C=1, t0=5e-3, adaptive=True, depth=4, residual=True,
                          init=True).cuda()
    with pytest.raises(NotImplementedError, match="residual"):
        vid.jvp(xv, torch.ones_like(xv), 25.0)
    with torch.no_grad():                                   # and the nets that have one still run
        xhat, xdot = net.jvp(x, v, 25.0)
    assert xhat.shape == x.shape == xdot.shape and torch.isfinite(xdot).all()


def test_gdlnet_jvp_reaches_the_gabor_parameters():
    g = load_golden("f5b_gabor_plain")
    net = build_from_golden(g, "gabor")
    y = g["y"].cuda()
    v = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).cuda()
    sigma = g["sigma"].cuda() if torch.is_tensor(g.get("sigma")) else g.get("sigma")
    xhat, xdot = net.jvp(y, v, sigma)
    with torch.no_grad():
        assert torch.equal(xhat, net(y, sigma)[0])
    torch.mean(v * xdot).backward()
    grads = [p.grad for n, p in net.named_parameters() if n != "t" and p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)


# ------------------------------------------------------------------------------------------ exact SURE
def _sure_ref(sd, y, b, supports, s2, **kw):
    y64, b64 = y.double(), b.double()
    s2 = s2.double() if torch.is_tensor(s2) else s2
    loss_fn = lambda xh, xd: torch.mean((y64 - xh) ** 2) + 2.0 * torch.mean(s2 * b64 * xd)
    return tangent_and_grads(sd, y, b, supports, loss_fn, **kw)


@pytest.mark.parametrize("precision", ["split3", "fp32"])
def test_sure_loss_on_the_fused_geometry_vs_oracle(precision):
    """The geometry of test_gpu_nets.test_mcsure_gradients_on_the_fused_path_with_both_supports_prescribed (K=3, M=32,
    P=5, 2x1x48x64): the exact objective and every gradient against the oracle's autograd of the same objective, at the
    tolerances of every other gradient of the suite (the finite-difference form is gated at 1e-4 / 2e-5 there)."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    torch.manual_seed(31)
    K, M, P = 3, 32, 5
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=1, t0=5e-3, adaptive=True, init=True)
    with torch.no_grad():
        for n_, p_ in net.named_parameters():
            if n_ == "t":
                p_.uniform_(2e-3, 2e-2)
            elif n_ != "g":
                p_.add_(0.05 * p_.abs().mean() * torch.randn_like(p_))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda()
    x = cva.utils.synthetic_clip((2, 1, 48, 64), seed=9)
    y = x + torch.randn(x.shape, generator=torch.Generator().manual_seed(10)) * 25 / 255
    b = torch.randn(y.shape, generator=torch.Generator().manual_seed(12))
    sigma = torch.tensor(25.0)
    tol = FP32_TOL if precision == "fp32" else SPLIT_TOL
    with loop.precision_scope(precision):
        with torch.no_grad():
            outs = net._run(y.cuda(), 25.0, 1, True)
        sup = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
        loss, xhat = cva.sure_loss(net, y.cuda(), sigma.cuda(), b=b.cuda())
        loss.backward()
    xo, _, ref_loss, ref = _sure_ref(sd, y, b, sup, (25.0 / 255.0) ** 2, K=K, P=P, s=1, sigma=25.0, adaptive=True,
                                     mask=None, ndim=2)
    log(f"sure_loss[{precision}] loss={loss.item():.8e} ref={ref_loss:.8e}")
    assert abs(loss.item() - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    for pname, p_ in net.named_parameters():
        if pname != "g":
            check(f"sure_loss[{precision}] K3 M32 P5 grad {pname}", p_.grad, ref[pname], tol)


def test_sure_loss_on_fixture_f2_vs_oracle():
    import cdlnet_video_amd as cva
    g = load_golden("f2_2d_s2_odd")
    net = build_from_golden(g, "2d")
    K, M, P, s, C = hyper(g)
    y, sigma = g["y"], g["sigma"]
    b = torch.randn(y.shape, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        outs = net._run(y.cuda(), sigma.cuda(), 1, True)
    sup = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
    loss, xhat = cva.sure_loss(net, y.cuda(), sigma.cuda(), b=b.cuda())
    loss.backward()
    _, _, ref_loss, ref = _sure_ref(g["sd"], y, b, sup, (sigma / 255.0) ** 2, K=K, P=P, s=s, sigma=sigma, adaptive=True,
                                    mask=None, ndim=2)
    log(f"sure_loss f2 loss={loss.item():.8e} ref={ref_loss:.8e}")
    assert abs(loss.item() - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    for pname, p_ in net.named_parameters():
        if pname != "g":
            check(f"sure_loss f2 grad {pname}", p_.grad, ref[pname], SPLIT_TOL)


# ------------------------------------------------------------------------------------------ trainer
def _small_trainer_net(seed=5):
    import cdlnet_video_amd as cva
    torch.manual_seed(seed)
    return cva.CDLNet(K=3, M=32, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()


def test_two_exact_train_steps_equal_the_hand_composed_ones():
    import copy

    import cdlnet_video_amd as cva
    net = _small_trainer_net()
    twin = copy.deepcopy(net)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt2 = torch.optim.Adam(twin.parameters(), lr=1e-3)
    batches = [cva.utils.synthetic_clip((2, 1, 40, 36), seed=40 + i).cuda() for i in range(2)]
    gen, gen2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for batch in batches:
        loss, sigma = cva.train_step(net, opt, batch, (20, 30), clip_grad=1.0, generator=gen, mcsure="exact")
        noisy, sig2 = cva.awgn(batch, (20, 30), gen2)
        opt2.zero_grad(set_to_none=True)
        b = torch.randn(noisy.shape, device=gen2.device, dtype=noisy.dtype, generator=gen2).to(noisy.device)
        xhat, xdot = twin.jvp(noisy, b, sig2, mask=1)
        l2 = torch.mean((noisy - xhat) ** 2) + 2.0 * torch.mean((sig2 / 255.0) ** 2 * b * xdot)
        l2.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
        opt2.step()
        twin.project()
        assert torch.equal(sigma, sig2) and torch.equal(loss, l2.detach())
    for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n


def test_short_exact_fit_stays_finite_and_mcsure_true_is_unchanged(tmp_path):
    import cdlnet_video_amd as cva
    net = _small_trainer_net(6)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    data = {"train": [cva.utils.synthetic_clip((2, 1, 40, 36), seed=50 + i) for i in range(3)]}
    hist = cva.fit(net, opt, data, epochs=2, device=torch.device("cuda"), save_dir=str(tmp_path), noise_std=25,
                   verbose=False, mcsure="exact", generator=torch.Generator().manual_seed(4), log=lambda *_: None)
    assert [e for e, p, _ in hist] == [1, 2] and all(torch.isfinite(torch.tensor(v)) for _, _, v in hist)
    assert not (tmp_path / "backtrack.txt").exists()
    assert all(torch.isfinite(p).all() for p in net.parameters())

    # mcsure=True: the finite-difference objective, exactly as composed by hand from net() and mcsure_loss
    net = _small_trainer_net(7)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    batch = data["train"][0].cuda()
    with torch.no_grad():
        noisy, sigma = cva.awgn(batch, 25, torch.Generator().manual_seed(8))
        gen = torch.Generator().manual_seed(8)
        cva.awgn(batch, 25, gen)                                   # advance to where train_step draws b
    xhat, _ = net(noisy, sigma, mask=1)
    want = cva.mcsure_loss(net, noisy, xhat, sigma, mask=1, generator=gen).detach()
    got, _ = cva.train_step(net, opt, batch, 25, generator=torch.Generator().manual_seed(8), mcsure=True)
    assert torch.equal(got, want)
