"""Gradients with respect to the noisy input y and the noise level sigma through the HIP reverse sweeps
(loop.UnrolledISTA): against the oracle's autograd at identical support on every tier the router picks, against the
reference's fixtures, and the properties the feature promises (no change to the parameter gradients, C sweep =
stepwise launches, the refusals that remain, composition with torch)."""
import pytest
import torch

from gpu_util import build_from_golden, check, load_golden, log
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

SPLIT_TOL = 5e-5     # split-bf16 tiers (test_fused_reverse_sweep_equals_generic_on_same_activations)
FP32_TOL = 1e-5      # precision_scope("fp32"): the fp32 VALU kernels
BF16_TOL = 2e-2      # blocked_bf16 code STORAGE: bf16-rounded du / codes, outside the 1e-5 gate (PSNR parity only)


def _perturbed(net, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n == "t":
                p.uniform_(2e-3, 2e-2)
            elif n != "g":
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net


def _padded(shape, s):
    from cdlnet_video_amd import ops
    return tuple(int(d) + sum(ops.split_pad(int(d), s)) for d in shape)


def _geom(net, y, s):
    from cdlnet_video_amd import ops
    A0 = net.A[0].weight
    P = tuple(A0.shape[2:])
    nd = y.dim() - 2
    return ops.Geometry.make(y.shape[0], y.shape[1], A0.shape[0], _padded(y.shape[2:], s), P,
                             tuple(p // 2 for p in P), [s] * nd)


def _case(kind, seed, shape, s, masked, **kw):
    import cdlnet_video_amd as cva
    torch.manual_seed(seed)
    if kind == "2d":
        net = cva.CDLNet(s=s, C=shape[1], t0=5e-3, adaptive=True, init=True, **kw)
    else:
        net = cva.CDLNetVideo(s=s, C=shape[1], t0=5e-3, adaptive=True, depth=shape[2], init=True, **kw)
    net = _perturbed(net, seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = cva.utils.synthetic_clip(shape, seed=seed + 2)
    N, nd = shape[0], len(shape) - 2
    sigma = torch.linspace(15.0, 35.0, N).reshape((N,) + (1,) * (nd + 1))
    mask = None
    if masked == "bayer":
        mask = O.bayer_mask(x)
    elif masked:
        mask = (torch.rand(shape, generator=gen) < 0.6).float()
    y = x + torch.randn(shape, generator=gen) * sigma / 255
    if mask is not None:
        y = mask * y
    w = torch.randn(shape, generator=gen)
    return net.cuda(), sd, x, y, sigma, mask, w


def _loss(xhat, x, w):
    return torch.mean((xhat - x) ** 2) + torch.mean(w * xhat)


def _hip_grads(net, x, y, sigma, mask, w):
    yg = y.cuda().requires_grad_(True)
    sg = sigma.cuda().requires_grad_(True)
    m = mask.cuda() if mask is not None else 1
    xhat, _ = net(yg, sg, mask=m)
    dy, ds = torch.autograd.grad(_loss(xhat, x.cuda(), w.cuda()), (yg, sg))
    return xhat.detach(), dy, ds


def _supports(net, y, sigma, mask):
    with torch.no_grad():
        outs = net._run(y.cuda(), sigma.cuda(), mask.cuda() if mask is not None else 1, True)
    return [c.detach().cpu() for c in outs[2:]] + [outs[1].detach().cpu()]


def _oracle_grads(net, sd, x, y, sigma, mask, w, supports):
    K = len(net.A)
    A0 = net.A[0].weight
    nd = y.dim() - 2
    P = tuple(A0.shape[2:]) if nd == 3 else A0.shape[-1]
    yo = y.clone().requires_grad_(True)
    so = sigma.clone().requires_grad_(True)
    xo, _ = O.ista(sd, yo, K=K, P=P, s=net.s, sigma=so, adaptive=True, mask=mask, ndim=nd, supports=supports)
    dy, ds = torch.autograd.grad(_loss(xo, x, w), (yo, so))
    return xo, dy, ds


def _vs_oracle(tag, net, sd, x, y, sigma, mask, w, tol):
    supports = _supports(net, y, sigma, mask)
    xhat, dy, ds = _hip_grads(net, x, y, sigma, mask, w)
    xo, dyo, dso = _oracle_grads(net, sd, x, y, sigma, mask, w, supports)
    assert dy.shape == y.shape and ds.shape == sigma.shape
    check(f"datagrad {tag} xhat", xhat, xo, 1e-5 if tol < BF16_TOL else BF16_TOL)
    check(f"datagrad {tag} dL/dy", dy, dyo, tol)
    check(f"datagrad {tag} dL/dsigma", ds, dso, tol)


@pytest.mark.parametrize("layout", ["nchw", "blocked", "blocked_bf16"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,shape", [(32, (2, 1, 48, 40)), (64, (2, 1, 45, 39))])
def test_fused2d_vs_oracle(layout, masked, M, shape):
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, sigma, mask, w = _case("2d", 11, shape, 1, masked, K=4, M=M, P=7)
    assert ops.fused_supported(_geom(net, y, 1))
    saved = loop.CODE_LAYOUT
    loop.set_code_layout(layout)
    try:
        _vs_oracle(f"fused2d {layout} M{M} {shape} mask={masked}", net, sd, x, y, sigma, mask, w,
                   BF16_TOL if layout == "blocked_bf16" else SPLIT_TOL)
    finally:
        loop.set_code_layout(saved)


def test_fused2d_split4_and_fp32_scope_vs_oracle():
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, sigma, mask, w = _case("2d", 12, (2, 1, 40, 36), 1, True, K=3, M=32, P=5)
    assert ops.fused_supported(_geom(net, y, 1))
    with loop.precision_scope("split4"):
        _vs_oracle("fused2d split4", net, sd, x, y, sigma, mask, w, SPLIT_TOL)
    with loop.precision_scope("fp32"):            # no fused kernels: the generic sweep on the fp32 VALU kernels
        _vs_oracle("fp32 scope", net, sd, x, y, sigma, mask, w, FP32_TOL)
    # four products at M = 64 in the default blocked layout (split4 ran at M = 32 only)
    net, sd, x, y, sigma, mask, w = _case("2d", 13, (2, 1, 45, 39), 1, True, K=4, M=64, P=7)
    assert ops.fused_supported(_geom(net, y, 1)) and loop.CODE_LAYOUT == "blocked"
    with loop.precision_scope("split4"):
        _vs_oracle("fused2d split4 M64 blocked", net, sd, x, y, sigma, mask, w, SPLIT_TOL)


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
    _vs_oracle(label, net, sd, x, y, sigma, mask, w, SPLIT_TOL)


@pytest.mark.parametrize("shape", [(2, 1, 50, 78), (2, 1, 49, 77)])
def test_strip_route_vs_oracle(shape):
    """C = 1, s = 2, M > 64: the strip kernel behind the cdl_fusedg_* entry points (and its rsc code layout)."""
    from cdlnet_video_amd import ops
    net, sd, x, y, sigma, mask, w = _case("2d", 14, shape, 2, False, K=3, M=96, P=7)
    g = _geom(net, y, 2)
    assert ops.fusedg_supported(g) and not ops.fused_supported(g)
    log(f"strip route code layout: {ops.fusedg_code_layout(g)}")
    _vs_oracle(f"strip {shape}", net, sd, x, y, sigma, mask, w, SPLIT_TOL)


def test_generic_3d_s2_p9_vs_oracle():
    from cdlnet_video_amd import ops
    net, sd, x, y, sigma, mask, w = _case("3d", 15, (2, 1, 8, 20, 12), 2, False, K=2, M=5, P=[9, 9, 5])
    g = _geom(net, y, 2)
    assert not ops.fusedg_supported(g) and not ops.fused_supported(g)
    _vs_oracle("generic 3-D s2 P9", net, sd, x, y, sigma, mask, w, SPLIT_TOL)


@pytest.mark.parametrize("masked", [False, True])
def test_generic_backend_2d_vs_oracle(masked):
    from cdlnet_video_amd import loop
    net, sd, x, y, sigma, mask, w = _case("2d", 16, (2, 1, 33, 31), 2, masked, K=3, M=16, P=7)
    loop.set_backend("generic")
    try:
        _vs_oracle(f"generic backend 2-D mask={masked}", net, sd, x, y, sigma, mask, w, SPLIT_TOL)
    finally:
        loop.set_backend("auto")


FIXTURES = [("d1_2d_s1", "2d"), ("d2_2d_s2_odd", "2d"), ("d3_jdd_c3_mask", "2d"), ("d3b_jdd_s2_odd", "2d"),
            ("d4a_3d_p555", "3d"), ("d4c_3d_s2_odd", "3d"), ("d0_adaptive_false", "2d")]


def _fixture_grads(g, kind):
    net = build_from_golden(g, kind)
    net.adaptive = bool(g["has_dsigma"])
    y = g["y"].cuda().requires_grad_(True)
    sigma = g["sigma"].cuda().requires_grad_(True)
    mask = g["mask"].cuda() if "mask" in g else 1
    xhat, _ = net(y, sigma, mask=mask)
    loss = _loss(xhat, g["x"].cuda(), g["w"].cuda())
    loss.backward()
    with torch.no_grad():
        outs = net._run(g["y"].cuda(), g["sigma"].cuda(), mask, True)
    codes = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
    return loss, y.grad, sigma.grad, codes


@pytest.mark.parametrize("name,kind", FIXTURES)
def test_data_gradients_match_reference(name, kind):
    """y.grad and sigma.grad at the fixture sizes against the reference, to the f-fixture gradient tolerance.
    dL/dy is per pixel, so one code on the other side of a near-tie of ST (|u| within split-bf16 rounding of tau: d3 has
    one at 5e-6 relative) moves a P x P patch of it: where the fused tier's supports differ from the reference's in a few
    elements, the comparison is made on the fp32 tier, whose supports must then agree (identical-support parity of the
    fused tiers is the oracle tests above)."""
    from cdlnet_video_amd import loop
    g = load_golden(name)
    K, _, P, s, _ = g["hyper"]
    P = tuple(g["P3"]) if "P3" in g else P
    nd = g["x"].dim() - 2
    with torch.no_grad():
        _, ref_codes = O.ista(g["sd"], g["y"], K=K, P=P, s=s, sigma=g["sigma"], adaptive=bool(g["has_dsigma"]),
                              mask=g.get("mask"), ndim=nd, all_codes=True)

    def flips(codes):
        return sum(int(((a != 0) != (b != 0)).sum()) for a, b in zip(codes, ref_codes))

    loss, dy, ds, codes = _fixture_grads(g, kind)
    nflip = flips(codes)
    log(f"{name} support flips against the reference: {nflip}")
    if nflip:
        assert nflip <= 4, f"{name}: {nflip} support flips is more than near-ties"
        with loop.precision_scope("fp32"):
            loss, dy, ds, codes = _fixture_grads(g, kind)
        assert flips(codes) == 0
    assert abs(loss.item() - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"])) + 1e-8
    check(f"{name} dL/dy", dy, g["dy"], 2e-4)
    if g["has_dsigma"]:
        check(f"{name} dL/dsigma", ds, g["dsigma"], 2e-4)
    else:
        assert ds is None


def _param_grads(net, y, sigma, mask, x, w, want_y):
    for p in net.parameters():
        p.grad = None
    yy = y.cuda().requires_grad_(want_y)
    xhat, _ = net(yy, sigma.cuda(), mask=mask.cuda() if mask is not None else 1)
    _loss(xhat, x.cuda(), w.cuda()).backward()
    return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tier", ["fused2d", "fused2d-bf16", "fusedg", "strip", "generic"])
def test_parameter_gradients_unchanged_by_y_requires_grad(tier):
    """Asking for dL/dy adds outputs to the sweeps and changes none of the parameter gradients: bit for bit."""
    from cdlnet_video_amd import loop
    spec = {"fused2d": ("2d", (2, 1, 48, 40), 1, True, dict(K=4, M=32, P=7)),
            "fused2d-bf16": ("2d", (2, 1, 48, 40), 1, False, dict(K=4, M=32, P=7)),
            "fusedg": ("2d", (2, 3, 24, 28), 1, "bayer", dict(K=3, M=32, P=7)),
            "strip": ("2d", (2, 1, 50, 78), 2, False, dict(K=3, M=96, P=7)),
            "generic": ("3d", (2, 1, 8, 20, 12), 2, False, dict(K=2, M=5, P=[9, 9, 5]))}[tier]
    kind, shape, s, masked, kw = spec
    net, sd, x, y, sigma, mask, w = _case(kind, 17, shape, s, masked, **kw)
    saved = loop.CODE_LAYOUT
    if tier == "fused2d-bf16":
        loop.set_code_layout("blocked_bf16")
    try:
        plain = _param_grads(net, y, sigma, mask, x, w, False)
        with_y = _param_grads(net, y, sigma, mask, x, w, True)
    finally:
        loop.set_code_layout(saved)
    assert plain.keys() == with_y.keys()
    for n in plain:
        assert torch.equal(plain[n], with_y[n]), f"{tier}: {n}"


def _sweep_inputs(masked, seed=21, K=3, M=32, P=7, shape=(2, 1, 40, 36)):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    net, sd, x, y, sigma, mask, w = _case("2d", seed, shape, 1, masked, K=K, M=M, P=P)
    yp, mean, pads, mask_p = o.preprocess(y.cuda(), 1, mask.cuda() if mask is not None else None)
    N = shape[0]
    g = o.Geometry.make(N, 1, M, yp.shape[2:], (P, P), (P // 2, P // 2), 1)
    c = (sigma.reshape(-1) / 255.0).cuda()
    tau = o.thresholds(net.t.detach(), c, N)
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    xp, z, codes, resid, maps = loop._forward_fused(g, yp, mask_p, tau, A, B, True, True, layout="nchw")
    g_xp = torch.randn(xp.shape, generator=torch.Generator().manual_seed(8)).cuda()
    g_z = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).cuda() * 0.01
    return g, K, yp, mask_p, c, A, B, codes, resid, maps, g_xp, g_z


@pytest.mark.parametrize("masked", [False, True])
def test_stepwise_equals_whole_sweep_data_gradients(masked):
    """dyp / dtau of the C whole sweeps equal those of the Python stepwise sweeps (same launches: fused bit for bit)."""
    from cdlnet_video_amd import loop
    g, K, yp, mask_p, c, A, B, codes, resid, maps, g_xp, g_z = _sweep_inputs(masked)
    out = {}
    for name, sweep, kw in (("fused", loop._backward_fused, dict(layout="nchw")),
                            ("fused_step", loop._backward_fused_stepwise, dict(layout="nchw")),
                            ("generic", loop._backward_generic, {}),
                            ("generic_step", loop._backward_generic_stepwise, {})):
        dt = torch.zeros(K, 2, g.M, device="cuda")
        dyp = torch.empty(g.image_shape(), device="cuda")
        dtau = torch.empty((K, g.N, g.M), device="cuda")
        dA, dB = sweep(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps, dyp=dyp, dtau=dtau, **kw)
        out[name] = (dyp, dtau, dt, dA, dB)
        # the per-sample threshold gradients fold into dt exactly as the sweep's own reduction does, to rounding
        check(f"{name} mask={masked} sum_n dtau vs dt0", dtau.sum(1), dt[:, 0], 1e-5)
        check(f"{name} mask={masked} sum_n c dtau vs dt1", torch.einsum("knm,n->km", dtau, c), dt[:, 1], 1e-5)
    for a, b in (("fused", "fused_step"),):
        assert torch.equal(out[a][0], out[b][0]) and torch.equal(out[a][1], out[b][1]), (a, b)
    check(f"generic stepwise dyp mask={masked}", out["generic_step"][0], out["generic"][0], 1e-6)
    check(f"generic stepwise dtau mask={masked}", out["generic_step"][1], out["generic"][1], 1e-6)
    check(f"fused vs generic dyp mask={masked}", out["fused"][0], out["generic"][0], SPLIT_TOL)
    check(f"fused vs generic dtau mask={masked}", out["fused"][1], out["generic"][1], SPLIT_TOL)
    # and with no data gradient requested the sweep's parameter outputs are those of the plain call
    dt = torch.zeros(K, 2, g.M, device="cuda")
    dA, dB = loop._backward_fused(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps, layout="nchw")
    assert torch.equal(dt, out["fused"][2])
    assert all(torch.equal(a, b) for a, b in zip(dA + dB, out["fused"][3] + out["fused"][4]))


def test_still_refused():
    import cdlnet_video_amd as cva
    x = cva.utils.synthetic_clip((1, 1, 24, 24), seed=1).cuda()
    net = cva.CDLNet(K=2, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    mask = torch.ones_like(x).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        net(x, 25.0, mask=mask)
    csr = cva.CDLNet_CSR(K=2, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    with torch.no_grad():
        _, zp = csr(x, None, 25.0)
    with pytest.raises(NotImplementedError):
        csr(x.clone().requires_grad_(True), None, 25.0)
    with pytest.raises(NotImplementedError):
        csr(x.clone().requires_grad_(True), zp, 25.0)
    with pytest.raises(NotImplementedError):
        csr(x, zp, torch.tensor(25.0, device="cuda", requires_grad=True))
    xv = cva.utils.synthetic_clip((1, 1, 4, 16, 16), seed=2).cuda()
    vid = cva.CDLNetVideo(K=2, M=8, P=[3, 3, 3], s=1, C=1, t0=5e-3, adaptive=True, depth=4, residual=True,
                          init=True).cuda()
    with pytest.raises(NotImplementedError):
        vid(xv.clone().requires_grad_(True), 25.0)


@pytest.mark.parametrize("sigma_kind", ["per_sample", "scalar_tensor", "float", "not_adaptive"])
def test_sigma_forms(sigma_kind):
    """A per-sample (N,1,1,1) sigma, a 0-d sigma tensor and a float behave as the reference; adaptive=False: sigma
    is unused and gets no gradient."""
    import cdlnet_video_amd as cva
    net, sd, x, y, _, mask, w = _case("2d", 19, (2, 1, 40, 36), 1, False, K=3, M=32, P=5)
    net.adaptive = sigma_kind != "not_adaptive"
    sig = {"per_sample": torch.tensor([18.0, 30.0]).reshape(2, 1, 1, 1), "scalar_tensor": torch.tensor(25.0),
           "float": 25.0, "not_adaptive": torch.tensor(25.0)}[sigma_kind]
    supports = _supports(net, y, sig if torch.is_tensor(sig) else torch.tensor(sig), mask)
    yg = y.cuda().requires_grad_(True)
    sg = sig.cuda().requires_grad_(True) if torch.is_tensor(sig) else sig
    xhat, _ = net(yg, sg)
    _loss(xhat, x.cuda(), w.cuda()).backward()
    yo = y.clone().requires_grad_(True)
    so = sig.clone().requires_grad_(True) if torch.is_tensor(sig) else sig
    xo, _ = O.ista(sd, yo, K=3, P=5, s=1, sigma=so, adaptive=net.adaptive, supports=supports)
    _loss(xo, x, w).backward()
    check(f"sigma form {sigma_kind} dL/dy", yg.grad, yo.grad, SPLIT_TOL)
    if torch.is_tensor(sig):
        if sigma_kind == "not_adaptive":
            assert sg.grad is None and so.grad is None
        else:
            assert sg.grad.shape == sig.shape
            check(f"sigma form {sigma_kind} dL/dsigma", sg.grad, so.grad, SPLIT_TOL)
    del cva


def test_loss_on_code_only_and_composition():
    """A loss on z alone gives dL/dy without the mean term; a noise parameter upstream of the net gets its gradient."""
    net, sd, x, y, sigma, mask, w = _case("2d", 20, (2, 1, 40, 36), 1, False, K=3, M=32, P=5)
    supports = _supports(net, y, sigma, mask)
    yg = y.cuda().requires_grad_(True)
    _, z = net(yg, sigma.cuda())
    wz = torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
    (z * wz.cuda()).sum().backward()
    yo = y.clone().requires_grad_(True)
    _, zo = O.ista(sd, yo, K=3, P=5, s=1, sigma=sigma, adaptive=True, supports=supports)
    (zo * wz).sum().backward()
    check("loss on z only: dL/dy", yg.grad, yo.grad, SPLIT_TOL)

    noise = (0.01 * torch.randn(y.shape, generator=torch.Generator().manual_seed(4))).cuda().requires_grad_(True)
    xhat, _ = net(x.cuda() + noise, sigma.cuda())
    (gn,) = torch.autograd.grad(_loss(xhat, x.cuda(), w.cuda()), (noise,))
    assert gn is not None and gn.shape == noise.shape and torch.isfinite(gn).all() and gn.abs().max() > 0
