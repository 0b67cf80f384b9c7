"""Noise-level maps on the device: `sigma` as a tensor that broadcasts to (N, 1, *code grid) -- one level per frame, or a
full map -- through the shape-generic sweeps.  Against the reference's s-fixtures, against the
oracle's autograd at identical support, a constant map against the per-sample path, one case at a user's size, the
routing of everything that is not a map, and the refusals.

Tolerances are those of tests/test_gpu_datagrad.py for the same quantities."""
import pytest
import torch

from gpu_util import build_from_golden, check, load_golden, log
from oracle import cdl_oracle as O
from sigmamap_util import FIXTURES, RESIDUAL_FIXTURE, fixture_args, loss_of, oracle_grads, smooth_map

pytestmark = pytest.mark.gpu

XTOL = 1e-5          # xhat
SPLIT_TOL = 5e-5     # gradients at identical support, split-bf16 matrix-core kernels
FP32_TOL = 1e-5      # the same under precision_scope("fp32")
FIX_TOL = 2e-4       # against the reference's recorded data gradients (test_data_gradients_match_reference)
FIX_GTOL = 2e-4      # parameter gradients of the f-fixtures (tests/test_gpu_nets.py GTOL)
RES_GTOL = 1e-4      # parameter gradients of r1 (tests/test_gpu_residual.py)


def _run_all(net, x, y, sigma, mask, w):
    """(xhat, z, loss, parameter gradients, dL/dy, dL/dsigma, codes) of the product."""
    for p in net.parameters():
        p.grad = None
    yg = y.cuda().requires_grad_(True)
    sg = sigma.cuda().requires_grad_(True)
    m = mask.cuda() if mask is not None else 1
    xhat, z = net(yg, sg, mask=m)
    loss = loss_of(xhat, x.cuda(), w.cuda())
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    with torch.no_grad():
        outs = net._run(y.cuda(), sigma.cuda(), m, True)
    codes = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
    return xhat.detach(), z.detach(), float(loss.detach()), grads, yg.grad, sg.grad, codes


# ------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("name,kind", FIXTURES)
def test_fixture_matches_reference(name, kind):
    """Outputs and every gradient against the reference's record.  Near-ties as in test_data_gradients_match_reference: at
    most 4 support flips against the oracle's codes, and then the comparison is made on the fp32 tier, where flips must
    be 0."""
    from cdlnet_video_amd import loop
    g = load_golden(name)
    args = fixture_args(g, kind)
    net = build_from_golden(g, kind, **({"adaptive": True} if kind == "gabor" else {}))
    with torch.no_grad():
        _, ref_codes = O.ista(g["sd"], g["y"], sigma=g["sigma"], adaptive=True, all_codes=True, **args)

    def flips(codes):
        return sum(int(((a != 0) != (b != 0)).sum()) for a, b in zip(codes, ref_codes))

    out = _run_all(net, g["x"], g["y"], g["sigma"], g.get("mask"), g["w"])
    nflip = flips(out[-1])
    log(f"{name} support flips against the reference: {nflip}")
    if nflip:
        assert nflip <= 4, f"{name}: {nflip} support flips is more than near-ties"
        with loop.precision_scope("fp32"):
            out = _run_all(net, g["x"], g["y"], g["sigma"], g.get("mask"), g["w"])
        assert flips(out[-1]) == 0
    xhat, z, loss, grads, dy, ds, _ = out
    check(f"{name} xhat", xhat, g["xhat"], XTOL)
    check(f"{name} z", z, g["z"], XTOL)
    assert abs(loss - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"])) + 1e-8
    check(f"{name} dL/dy", dy, g["dy"], FIX_TOL)
    assert ds.shape == g["sigma"].shape
    check(f"{name} dL/dsigma", ds, g["dsigma"], FIX_TOL)
    seen = 0
    for pname, ref in g["grad"].items():
        if pname == "g":
            continue
        check(f"{name} grad {pname}", grads[pname], ref, FIX_GTOL)
        seen += 1
    assert seen == len([k for k in g["grad"] if k != "g"]) and seen > 0


def test_residual_fixture_matches_reference():
    import cdlnet_video_amd as cva
    g = load_golden(RESIDUAL_FIXTURE)
    K, M, Pd, Ph, Pw, s, C = g["hyper"]
    net = cva.CDLNetVideo(K=K, M=M, P=(Pd, Ph, Pw), s=s, C=C, t0=0.0, adaptive=True, init=False, residual=True)
    net.load_state_dict(g["sd"])
    net = net.cuda()
    xhat, z = net(g["y"].cuda(), g["sigma"].cuda())
    check("sr1 xhat", xhat, g["xhat"], XTOL)
    check("sr1 z", z, g["z"], XTOL)
    loss = loss_of(xhat, g["x"].cuda(), g["w"].cuda())
    assert abs(float(loss.detach()) - g["loss"]) < 1e-5 * max(1.0, abs(g["loss"]))
    loss.backward()
    params = dict(net.named_parameters())
    for key, ref in g["grad"].items():
        check(f"sr1 grad {key}", params[key].grad, ref, RES_GTOL)
    # the data gradients of the chain stay refused, with a map as without
    with pytest.raises(NotImplementedError):
        net(g["y"].cuda(), g["sigma"].cuda().requires_grad_(True))


# ------------------------------------------------------------------------------------------ 2. the oracle, same support
def _perturbed(net, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n == "t":
                p.uniform_(2e-3, 2e-2)
            elif n != "g":
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net


def _case(kind, seed, shape, s, masked, sigma_shape, **kw):
    import cdlnet_video_amd as cva
    torch.manual_seed(seed)
    if kind == "2d":
        net = cva.CDLNet(s=s, C=shape[1], t0=5e-3, adaptive=True, init=True, **kw)
    elif kind == "3d":
        net = cva.CDLNetVideo(s=s, C=shape[1], t0=5e-3, adaptive=True, depth=shape[2], init=True, **kw)
    else:
        net = cva.GDLNet(s=s, C=shape[1], t0=5e-3, order=1, adaptive=True, shared="", init=True, **kw)
    net = _perturbed(net, seed)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = cva.utils.synthetic_clip(shape, seed=seed + 2)
    sigma = smooth_map(sigma_shape, seed + 3)
    mask = O.bayer_mask(x) if masked == "bayer" else None
    grid = tuple(-(-d // s) for d in shape[2:])
    level = sigma.reshape((1,) * (len(shape) - sigma.dim()) + tuple(sigma.shape)).expand((shape[0], 1) + grid)
    if s > 1:                                          # noise at the image grid: each code pixel's level over its block
        level = level.repeat_interleave(s, -1).repeat_interleave(s, -2)
        if len(shape) == 5:
            level = level.repeat_interleave(s, -3)
        level = level[(..., ) + tuple(slice(0, d) for d in shape[2:])]
    y = x + torch.randn(shape, generator=gen) * level / 255
    if mask is not None:
        y = mask * y
    w = torch.randn(shape, generator=gen)
    return net.cuda(), sd, x, y, sigma, mask, w


def _geom(net, y, s):
    from cdlnet_video_amd import ops
    A0 = net.A[0].weight if hasattr(net.A[0], "weight") else None
    P = tuple(A0.shape[2:]) if A0 is not None else (net.P, net.P)
    M = A0.shape[0] if A0 is not None else net.M
    padded = tuple(int(d) + sum(ops.split_pad(int(d), s)) for d in y.shape[2:])
    return ops.Geometry.make(y.shape[0], y.shape[1], M, padded, P, tuple(p // 2 for p in P), [s] * (y.dim() - 2))


def _mfma_analysis_covers(g):
    import ctypes
    from cdlnet_video_amd import _lib
    gs = g.c_struct()
    return int(_lib.lib().cdl_analysis_workspace_floats(ctypes.byref(gs))) > 0


ORACLE_CASES = [
    # label, kind, shape, s, mask, sigma shape, net kwargs, matrix-core analysis (k_ana_m) expected to cover it
    ("2-D s1 k_ana_m", "2d", (4, 1, 200, 64), 1, None, (4, 1, 200, 64), dict(K=3, M=16, P=7), True),
    ("2-D s1 k_ana_m M40", "2d", (4, 1, 200, 64), 1, None, (4, 1, 200, 64), dict(K=2, M=40, P=5), True),   # two channel tiles
    ("2-D s1 small", "2d", (2, 1, 33, 31), 1, None, (2, 1, 33, 31), dict(K=3, M=16, P=7), False),
    ("2-D s2 odd", "2d", (2, 1, 33, 31), 2, None, (2, 1, 17, 16), dict(K=3, M=16, P=7), False),
    ("C3 bayer", "2d", (2, 3, 24, 28), 1, "bayer", (2, 1, 24, 28), dict(K=3, M=32, P=7), False),
    ("3-D s1 per frame", "3d", (1, 1, 6, 24, 40), 1, None, (1, 1, 6, 1, 1), dict(K=3, M=16, P=[3, 5, 5]), False),
    ("3-D s2 P995", "3d", (2, 1, 8, 20, 12), 2, None, (2, 1, 4, 10, 6), dict(K=2, M=5, P=[9, 9, 5]), None),
    ("GDLNet", "gabor", (2, 1, 32, 28), 1, None, (1, 1, 32, 28), dict(K=2, M=8, P=7), False),
]


@pytest.mark.parametrize("arith", ["default", "fp32"])
@pytest.mark.parametrize("label,kind,shape,s,masked,sshape,kw,mfma", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_vs_oracle_on_identical_support(label, kind, shape, s, masked, sshape, kw, mfma, arith):
    from cdlnet_video_amd import loop
    net, sd, x, y, sigma, mask, w = _case(kind, 31, shape, s, masked, sshape, **kw)
    if mfma is not None:
        assert _mfma_analysis_covers(_geom(net, y, s)) == mfma, label
    else:
        log(f"sigmamap {label}: matrix-core analysis covers it: {_mfma_analysis_covers(_geom(net, y, s))}")
    tol = FP32_TOL if arith == "fp32" else SPLIT_TOL
    with loop.precision_scope("fp32" if arith == "fp32" else loop.PRECISION):
        xhat, z, loss, grads, dy, ds, codes = _run_all(net, x, y, sigma, mask, w)
    nd = len(shape) - 2
    P = tuple(kw["P"]) if nd == 3 else kw["P"]
    if kind == "gabor":
        sd = O.gabor_alias(dict(sd), kw["K"], "")
    xo, zo, lo, go, dyo, dso = oracle_grads(sd, x, y, w, sigma, K=kw["K"], P=P, s=s, mask=mask, ndim=nd,
                                            gabor=kind == "gabor", supports=codes)
    tag = f"sigmamap {label} [{arith}]"
    check(f"{tag} xhat", xhat, xo, XTOL)
    assert dy.shape == y.shape and ds.shape == sigma.shape
    check(f"{tag} dL/dy", dy, dyo, tol)
    check(f"{tag} dL/dsigma", ds, dso, tol)
    seen = 0
    for pname, ref in go.items():
        if pname == "g" or ref is None:
            continue
        check(f"{tag} grad {pname}", grads[pname], ref, tol)
        seen += 1
    assert seen >= 1 + 2 * kw["K"]


@pytest.mark.parametrize("masked", [None, "bayer"])
def test_stepwise_equals_whole_sweep(masked, monkeypatch):
    """The C whole sweeps (cdl_ista_forward / cdl_ista_backward with a map) against the same launches driven one by one
    from Python."""
    from cdlnet_video_amd import loop
    shape = (2, 3, 24, 28) if masked else (4, 1, 200, 64)
    net, sd, x, y, sigma, mask, w = _case("2d", 32, shape, 1, masked, (shape[0], 1) + shape[2:], K=3, M=16, P=7)
    whole = _run_all(net, x, y, sigma, mask, w)
    monkeypatch.setattr(loop, "_forward_generic", loop._forward_generic_stepwise)
    monkeypatch.setattr(loop, "_backward_generic", loop._backward_generic_stepwise)
    step = _run_all(net, x, y, sigma, mask, w)
    assert torch.equal(whole[0], step[0]) and torch.equal(whole[1], step[1])        # forward: the same launches
    same = torch.equal(whole[4], step[4]) and torch.equal(whole[5], step[5]) and \
        all(torch.equal(whole[3][n], step[3][n]) for n in whole[3])
    log(f"sigmamap stepwise vs whole sweep mask={masked}: gradients bit-identical: {same}")
    check(f"sigmamap stepwise dL/dy mask={masked}", step[4], whole[4], 1e-6)
    check(f"sigmamap stepwise dL/dsigma mask={masked}", step[5], whole[5], 1e-6)
    for n in whole[3]:
        check(f"sigmamap stepwise grad {n} mask={masked}", step[3][n], whole[3][n], 1e-6)


# ------------------------------------------------------------------------------------------ 3. against the per-sample path
def test_constant_map_equals_per_sample_path():
    from cdlnet_video_amd import loop
    shape = (4, 1, 200, 64)
    net, sd, x, y, _, mask, w = _case("2d", 33, shape, 1, None, (4, 1, 200, 64), K=3, M=16, P=7)
    per = torch.tensor([15.0, 22.0, 30.0, 38.0]).reshape(4, 1, 1, 1)
    dense = per.expand(4, 1, 200, 64).contiguous()
    loop.set_backend("generic")
    try:
        a = _run_all(net, x, y, per, mask, w)
        b = _run_all(net, x, y, dense, mask, w)
    finally:
        loop.set_backend("auto")
    assert b[5].shape == dense.shape and a[5].shape == per.shape
    bit = torch.equal(a[0], b[0]) and all(torch.equal(ca, cb) for ca, cb in zip(a[6], b[6]))
    log(f"sigmamap constant map vs per-sample: forward bit-identical: {bit}; dL/dy bit-identical: {torch.equal(a[4], b[4])}")
    check("sigmamap constant map xhat", b[0], a[0], XTOL)
    check("sigmamap constant map dL/dy", b[4], a[4], SPLIT_TOL)
    check("sigmamap constant map sum dL/dsigma", b[5].sum((2, 3), keepdim=True), a[5], SPLIT_TOL)
    for n in a[3]:
        check(f"sigmamap constant map grad {n}", b[3][n], a[3][n], SPLIT_TOL)


@pytest.mark.parametrize("kind,shape,sshape,kw", [
    ("3d", (2, 1, 6, 24, 20), (2, 1, 6, 1, 1), dict(K=2, M=8, P=[3, 5, 5])),
    ("2d", (3, 1, 30, 26), (1, 1, 30, 26), dict(K=3, M=8, P=5)),
])
def test_broadcast_forms_equal_their_dense_expansion(kind, shape, sshape, kw):
    net, sd, x, y, sigma, mask, w = _case(kind, 34, shape, 1, None, sshape, **kw)
    dense = sigma.expand((shape[0], 1) + shape[2:]).contiguous()
    a = _run_all(net, x, y, sigma, mask, w)
    b = _run_all(net, x, y, dense, mask, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4])
    assert all(torch.equal(a[3][n], b[3][n]) for n in a[3])
    assert a[5].shape == sigma.shape and b[5].shape == dense.shape
    check(f"sigmamap {sshape} dL/dsigma vs the dense map's, summed", a[5], b[5].sum_to_size(sigma.shape), 1e-6)


# ------------------------------------------------------------------------------------------ 4. a user's size
def test_user_size_256x256_k30_m64():
    import cdlnet_video_amd as cva
    torch.manual_seed(1)
    K, M, P = 30, 64, 7
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=1, t0=5e-3, adaptive=True, init=True)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda()
    x = cva.utils.synthetic_clip((1, 1, 256, 256), seed=0)
    sigma = smooth_map((1, 1, 256, 256), 5)
    y = x + torch.randn(x.shape, generator=torch.Generator().manual_seed(6)) * sigma / 255
    with torch.no_grad():
        xhat, _ = net(y.cuda(), sigma.cuda())
        xr, _ = O.ista(sd, y, K=K, P=P, s=1, sigma=sigma, adaptive=True)
    check("sigmamap 1x1x256x256 K30 M64 xhat", xhat, xr, XTOL)
    p_ref, p_got = O.psnr(x, xr), O.psnr(x, xhat.cpu())
    log(f"sigmamap 1x1x256x256 K30 M64: PSNR ref={p_ref:.4f} ours={p_got:.4f} noisy={O.psnr(x, y):.2f}")
    assert round(p_ref, 2) == round(p_got, 2)


# ------------------------------------------------------------------------------------------ 5. unchanged ground
def test_per_sample_sigma_keeps_its_route(monkeypatch):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop, ops
    seen = []
    orig_fwd = loop.UnrolledISTA.forward

    def spy(ctx, *args):
        out = orig_fwd(ctx, *args)
        seen.append((ctx.fused, ctx.fusedg, ctx.is_map))
        return out
    monkeypatch.setattr(loop.UnrolledISTA, "forward", staticmethod(spy))
    torch.manual_seed(3)
    net = cva.CDLNet(K=3, M=32, P=7, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    y = cva.utils.synthetic_clip((2, 1, 48, 40), seed=1).cuda()
    assert ops.fused_supported(_geom(net, y, 1))
    per = torch.tensor([20.0, 30.0]).reshape(2, 1, 1, 1).cuda()
    with torch.no_grad():
        net(y, per)
        net(y, 25.0)
        net(y, per.expand(2, 1, 48, 40).contiguous())
    assert seen == [(True, False, False), (True, False, False), (False, False, True)]

    # generic backend, per-sample sigma: every new argument reaches the C sweeps as NULL
    calls = {}
    for name in ("ista_forward", "ista_backward"):
        orig = getattr(ops, name)

        def rec(*a, _orig=orig, _name=name, **k):
            calls[_name] = {q: k.get(q) for q in ("cmap", "tslope", "dcmap")}
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, rec)
    loop.set_backend("generic")
    try:
        sg = per.clone().requires_grad_(True)
        xhat, _ = net(y, sg)
        xhat.square().mean().backward()
    finally:
        loop.set_backend("auto")
    assert set(calls) == {"ista_forward", "ista_backward"}
    assert all(v is None for c in calls.values() for v in c.values()), calls
    assert sg.grad is not None and sg.grad.shape == per.shape


# ------------------------------------------------------------------------------------------ 6. the refusals
def test_refusals_and_adaptive_false():
    import cdlnet_video_amd as cva
    x = cva.utils.synthetic_clip((2, 1, 24, 26), seed=1).cuda()
    amap = smooth_map((2, 1, 24, 26), 2).cuda()
    torch.manual_seed(4)
    for cls in (cva.CDLNet_CSR, cva.CDLNet_CSRf2):
        csr = cls(K=2, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
        with torch.no_grad():
            _, zp = csr(x, sigma=25.0)
            with pytest.raises(NotImplementedError, match="map"):
                csr(x, sigma=amap)                                   # the no-neighbour branch too
            with pytest.raises(NotImplementedError, match="map"):
                csr(x, zp, sigma=amap)
    net = cva.CDLNet(K=2, M=8, P=5, s=2, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    with pytest.raises(ValueError, match="channel"):
        net(x, torch.rand(2, 8, 12, 13).cuda())
    with pytest.raises(ValueError, match=r"\(2, 1, 12, 13\)"):       # s = 2: the code grid, not the image's
        net(x, amap)
    with torch.no_grad():
        net(x, cva.utils.sigma_to_code_grid(amap, 2))                # ... which the helper produces
    # adaptive=False: the map is ignored and gets no gradient
    net.adaptive = False
    sg = amap.clone().requires_grad_(True)
    with torch.no_grad():
        ref, _ = net(x, None)
    xhat, _ = net(x, sg)
    assert torch.equal(xhat.detach(), ref)
    xhat.square().mean().backward()
    assert sg.grad is None
