"""Noise-level maps on the fused 2-D tier: `loop.set_map_tier("fused")` sends a map on a flagship
geometry through the map forms of cdl_fused2d.hip's stage kernel instead of the generic three-launch tier.

Against the per-sample fused call (a constant map: bit for bit where the sums are the same sums), against the generic
map route and the float64 oracle at identical supports (a map that varies inside every tile and differs per sample), the
route and its launches, the whole sweeps against the step-wise entry points, negative / NaN thresholds, net.jvp, windowed
inference, and guard-banded misaligned map buffers.

Shapes: the 64 x 16 tile gives (2,1,48,40) three tile rows and a ragged tile column, (1,1,33,130) three tile columns (the
last 2 pixels wide) and a last tile row of one image row; one shape has more tiles than the device has compute units, so
that persistent workgroups walk on to a second tile of another sample.  Tolerances are tests/test_gpu_sigmamap.py's.

Not here: the float64 arithmetic model of tests/fused2d_arith_restate.py takes one threshold per (sample, channel) row;
holding the map stage to its elementwise bound would need the model edited, so that check is left out."""
import contextlib

import pytest
import torch

from gpu_util import check, launch_sites, log
from oracle import cdl_oracle as O
from sigmamap_util import oracle_grads, smooth_map
from test_gpu_sigmamap import SPLIT_TOL, XTOL, _case, _geom, _run_all

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 48, 40), (1, 1, 33, 130)]
MP = [(32, 5), (32, 7), (64, 5), (64, 7)]
LAYOUTS = ["nchw", "blocked"]
GENERIC_KERNELS = ("k_ana_m", "k_synth_m")


@contextlib.contextmanager
def _layout(name):
    from cdlnet_video_amd import loop
    saved = loop.CODE_LAYOUT
    loop.set_code_layout(name)
    try:
        yield
    finally:
        loop.set_code_layout(saved)


def _fused_map(layout="blocked"):
    """The knob and the code layout of one test body."""
    from cdlnet_video_amd import loop
    stack = contextlib.ExitStack()
    stack.enter_context(_layout(layout))
    stack.enter_context(loop.map_tier_scope("fused"))
    return stack


def _varying_map(shape, seed):
    """Varies inside every tile (smooth_map plus a per-pixel random term) and differs per sample."""
    gen = torch.Generator().manual_seed(seed + 100)
    per_sample = 3.0 * torch.arange(shape[0], dtype=torch.float32).reshape(-1, 1, 1, 1)
    return smooth_map(shape, seed) + 4.0 * torch.rand(shape, generator=gen) + per_sample


def _big_shape():
    """More 64 x 16 tiles than compute units: (N,1,160,576) has 90 tiles per image."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (cus // 90 + 1, 1, 160, 576)


def _stage_modes(trace):
    return sorted({r.template()["MODE"] for k, v in launch_sites(trace).items()
                   if k.startswith("cdl_fused2d.hip:k_stage<") for r in v})


# ------------------------------------------------------------------------------------------ 1. a constant map
def _constant_map_case(shape, M, P, layout, K=3):
    from cdlnet_video_amd import ops
    net, sd, x, y, _, mask, w = _case("2d", 51, shape, 1, None, shape, K=K, M=M, P=P)
    assert ops.fused_supported(_geom(net, y, 1))
    N = shape[0]
    per = torch.linspace(15.0, 35.0, N).reshape(N, 1, 1, 1) if N > 1 else torch.full((1, 1, 1, 1), 25.0)
    dense = per.expand(shape).contiguous()
    with _layout(layout):
        a = _run_all(net, x, y, per, mask, w)                      # the per-sample fused route
        with _fused_map(layout), ops.trace() as t:
            b = _run_all(net, x, y, dense, mask, w)
            torch.cuda.synchronize()
    assert _stage_modes(t) == [4, 5, 6], _stage_modes(t)
    tag = f"fused map constant {shape} M{M}P{P} {layout}"
    assert torch.equal(a[0], b[0]), f"{tag}: xhat"
    assert torch.equal(a[1], b[1]), f"{tag}: z_K"
    assert len(a[6]) == K and all(torch.equal(ca, cb) for ca, cb in zip(a[6], b[6])), f"{tag}: codes"
    assert torch.equal(a[4], b[4]), f"{tag}: dL/dy"
    for name in a[3]:
        if name != "t":
            assert torch.equal(a[3][name], b[3][name]), f"{tag}: grad {name}"
    ta, tb = a[3]["t"].reshape(K, 2, M), b[3]["t"].reshape(K, 2, M)
    assert torch.equal(ta[:, 0], tb[:, 0]), f"{tag}: dt[:,0]"
    check(f"{tag} dt[:,1]", tb[:, 1], ta[:, 1], SPLIT_TOL)          # summation order only
    assert b[5].shape == dense.shape and a[5].shape == per.shape
    check(f"{tag} sum dL/dsigma", b[5].sum((2, 3), keepdim=True), a[5], SPLIT_TOL)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,P", MP)
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_map_equals_the_per_sample_fused_call(shape, M, P, layout):
    _constant_map_case(shape, M, P, layout)


def test_constant_map_with_more_tiles_than_compute_units():
    _constant_map_case(_big_shape(), 32, 7, "blocked", K=2)


# ------------------------------------------------------------------------------------------ 2. a varying map
def _varying_map_case(shape, M, P, layout, K=3, sigma_shape=None):
    from cdlnet_video_amd import ops
    net, sd, x, y, _, mask, w = _case("2d", 52, shape, 1, None, shape, K=K, M=M, P=P)
    assert ops.fused_supported(_geom(net, y, 1))
    amap = _varying_map(sigma_shape or shape, 53)
    a = _run_all(net, x, y, amap, mask, w)                          # the default: the generic map route
    with _fused_map(layout), ops.trace() as t:
        b = _run_all(net, x, y, amap, mask, w)
        torch.cuda.synchronize()
    sites = launch_sites(t)
    assert any(k.startswith("cdl_fused2d.hip:k_stage<") for k in sites)
    assert not [k for k in sites if any(name in k for name in GENERIC_KERNELS)], sorted(sites)
    tag = f"fused map varying {shape} sigma{tuple(amap.shape)} M{M}P{P} {layout}"
    check(f"{tag} xhat vs generic tier", b[0], a[0], XTOL)
    check(f"{tag} z_K vs generic tier", b[1], a[1], XTOL)
    xo, zo, lo, go, dyo, dso = oracle_grads(sd, x, y, w, amap, K=K, P=P, s=1, supports=b[6])
    check(f"{tag} xhat vs oracle", b[0], xo, XTOL)
    assert b[4].shape == y.shape and b[5].shape == amap.shape
    check(f"{tag} dL/dy", b[4], dyo, SPLIT_TOL)
    check(f"{tag} dL/dsigma", b[5], dso, SPLIT_TOL)
    seen = 0
    for name, ref in go.items():
        if name == "g" or ref is None:
            continue
        check(f"{tag} grad {name}", b[3][name], ref, SPLIT_TOL)
        seen += 1
    assert seen >= 1 + 2 * K


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,P", MP)
@pytest.mark.parametrize("shape", SHAPES)
def test_varying_map_vs_generic_tier_and_oracle(shape, M, P, layout):
    _varying_map_case(shape, M, P, layout)


def test_varying_map_with_more_tiles_than_compute_units():
    _varying_map_case(_big_shape(), 32, 7, "blocked", K=2)


def test_row_map_gradient_comes_back_in_the_shape_given():
    """An (N,1,H,1) map: dense on the device, its gradient summed back to the rows (the sum_to_size path)."""
    _varying_map_case((2, 1, 48, 40), 32, 7, "blocked", sigma_shape=(2, 1, 48, 1))


# ------------------------------------------------------------------------------------------ 3. the route
def test_route_and_launches(monkeypatch):
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
    amap = _varying_map((2, 1, 48, 40), 3).cuda()
    with torch.no_grad():
        with loop.map_tier_scope("fused"), ops.trace() as t:
            net(y, amap)
            torch.cuda.synchronize()
        with ops.trace() as t0:
            net(y, amap)
            torch.cuda.synchronize()
        with loop.map_tier_scope("fused"), loop.precision_scope("split4"):
            net(y, amap)                                            # no map form in this arithmetic: the generic tier
    assert seen == [(True, False, True), (False, False, True), (False, False, True)]
    sites, sites0 = launch_sites(t), launch_sites(t0)
    assert _stage_modes(t) == [4, 5] and not [k for k in sites if any(n in k for n in GENERIC_KERNELS)], sorted(sites)
    assert sites0 and not [k for k in sites0 if k.startswith("cdl_fused2d.hip:")], sorted(sites0)


@pytest.mark.parametrize("M,P", [(64, 7), (32, 5)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_c_sweeps_are_bit_identical_to_stepwise_launches_with_a_map(layout, M, P):
    """cdl_fused2d_forward / _backward with a map against ops.fused_iter / fused_stage_bwd / fused_dtau_reduce driven from
    Python (tests/test_gpu_fused.py's sweep-versus-loop test): stage outputs, dt, dL/dyp and dL/dcmap bit for bit; dA_k /
    dB_k at the 2e-6 of that test (the sweep's snake order regroups the filter gradients' partial sums)."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    torch.manual_seed(31)
    K, N, H, W = 3, 2, 40, 72
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    y = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    yp, mean, pads, _ = o.preprocess(y, 1, None)
    g = o.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1)
    t = net.t.detach()
    tau = o.thresholds(t, None, N)
    cmap, tslope = loop._map_args((_varying_map((N, 1, H, W), 4) / 255).cuda(), t)
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    mp = dict(cmap=cmap, tslope=tslope)
    with o.trace() as tr:
        xp1, z1, codes1, resid1, maps1 = loop._forward_fused(g, yp, None, tau, A, B, True, True, layout=layout, **mp)
        torch.cuda.synchronize()
    xp2, z2, codes2, resid2, maps2 = loop._forward_fused_stepwise(g, yp, None, tau, A, B, True, True, layout=layout, **mp)
    assert len(maps1) == K and len(codes1) == K and len(resid1) == K - 1
    assert all(torch.equal(a, b) for a, b in zip(maps1, maps2))
    assert torch.equal(xp1, xp2) and torch.equal(z1, z2)
    for k in range(K):
        lay = layout if k < K - 1 else "nchw"
        assert torch.equal(o.fused_to_nchw(g, codes1[k], lay), o.fused_to_nchw(g, codes2[k], lay))
    assert all(torch.equal(a, b) for a, b in zip(resid1, resid2))
    xp3, z3, codes3, resid3, maps3 = loop._forward_fused(g, yp, None, tau, A, B, False, False, layout=layout, **mp)   # ping-pong
    assert torch.equal(xp3, xp1) and torch.equal(z3, z1)
    g_xp = torch.randn(xp1.shape, generator=torch.Generator().manual_seed(2)).cuda()
    outs = []
    with o.trace() as tb:
        for sweep in (loop._backward_fused, loop._backward_fused_stepwise):
            dt = torch.zeros(K, 2, M, device="cuda")
            dyp, dcmap = torch.empty_like(yp), torch.full_like(cmap, float("nan"))
            dA, dB = sweep(g, K, yp, None, None, A, B, codes1, resid1, g_xp, None, dt, maps=maps1, layout=layout, dyp=dyp,
                           dcmap=dcmap, **mp)
            outs.append((dA, dB, dt, dyp, dcmap))
        torch.cuda.synchronize()
    for k in range(K):
        check(f"fused map snake dA[{k}]", outs[0][0][k], outs[1][0][k], 2e-6)
        check(f"fused map snake dB[{k}]", outs[0][1][k], outs[1][1][k], 2e-6)
    assert torch.equal(outs[0][2], outs[1][2]), "dt"
    assert torch.equal(outs[0][3], outs[1][3]), "dyp"
    assert torch.equal(outs[0][4], outs[1][4]) and bool(torch.isfinite(outs[0][4]).all()), "dcmap"
    assert _stage_modes(tr) == [4, 5] and _stage_modes(tb) == [6]
    ride = {",true," in k for k in launch_sites(tb) if k.startswith("cdl_fused2d.hip:k_stage<")}
    assert ride == {True, False}                                    # dA_k rides in the sweep's stages, not in the step-wise ones


# ------------------------------------------------------------------------------------------ 4. negative and NaN thresholds
def _forward_both(net, y, amap, layout="blocked"):
    with torch.no_grad():
        a = net(y, amap)
        with _fused_map(layout):
            b = net(y, amap)
    return a, b


@pytest.mark.parametrize("layout", LAYOUTS)
def test_negative_threshold_on_part_of_the_map(layout):
    """One slope t[1,1,m0] < 0, so large that channel m0's threshold of iteration 1 is negative where the map exceeds
    30 / 255 and positive elsewhere (the map spans 10..47): the reference's ST for t < 0, |u| - t > 0 everywhere."""
    net, sd, x, y, _, mask, w = _case("2d", 54, (2, 1, 48, 40), 1, None, (2, 1, 48, 40), K=3, M=32, P=7)
    amap = _varying_map((2, 1, 48, 40), 55)
    m0 = 5
    with torch.no_grad():
        t = net.t.reshape(3, 2, 32)
        t[1, 1, m0] = -t[1, 0, m0] * 255.0 / 30.0
        thr = float(t[1, 0, m0]) + (amap / 255) * float(t[1, 1, m0])
    frac = float((thr < 0).float().mean())
    assert 0.05 < frac < 0.95, frac
    (xa, za), (xb, zb) = _forward_both(net, y.cuda(), amap.cuda(), layout)
    assert bool(torch.isfinite(xb).all())
    check(f"fused map negative slope {layout} xhat", xb, xa, XTOL)
    check(f"fused map negative slope {layout} z_K", zb, za, XTOL)
    with torch.no_grad():
        xo, _ = O.ista(sd | {"t": net.t.detach().cpu()}, y, K=3, P=7, s=1, sigma=amap, adaptive=True)
    check(f"fused map negative slope {layout} xhat vs oracle", xb, xo, XTOL)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_region_and_a_nan_pixel_in_the_map(layout):
    """An exact-zero region (thresholds t0: the clamp form's ground) at K = 3, and one NaN pixel at K = 1.  The shrinkage is
    where a threshold acts, so the NaN comparison is made on its output, the code z_1: NaN at that pixel in every channel
    and nowhere else, on both tiers.  Further on the tiers differ by construction -- the matrix-core kernels multiply the
    zero weights of their padded 8 x 8 tap grid with the NaN, the generic ones never touch a tap outside P x P -- so xhat is
    compared outside the 17 x 17 neighbourhood both footprints stay inside."""
    net, sd, x, y, _, mask, w = _case("2d", 56, (2, 1, 48, 40), 1, None, (2, 1, 48, 40), K=3, M=32, P=7)
    amap = _varying_map((2, 1, 48, 40), 57)
    amap[0, 0, 10:30, 5:33] = 0.0
    (xa, za), (xb, zb) = _forward_both(net, y.cuda(), amap.cuda(), layout)
    check(f"fused map zero region {layout} xhat", xb, xa, XTOL)
    check(f"fused map zero region {layout} z_K", zb, za, XTOL)
    net1, sd1, x1, y1, _, _, _ = _case("2d", 58, (2, 1, 48, 40), 1, None, (2, 1, 48, 40), K=1, M=32, P=7)
    amap[1, 0, 20, 17] = float("nan")
    (xa, za), (xb, zb) = _forward_both(net1, y1.cuda(), amap.cuda(), layout)
    want = torch.zeros_like(za, dtype=torch.bool)
    want[1, :, 20, 17] = True
    assert torch.equal(torch.isnan(zb), want) and torch.equal(torch.isnan(za), want)
    check(f"fused map NaN pixel {layout} z_1 elsewhere", torch.nan_to_num(zb), torch.nan_to_num(za), XTOL)
    far = torch.ones_like(xa, dtype=torch.bool)
    far[1, :, 12:29, 9:26] = False
    assert bool(torch.isfinite(xb[far]).all()) and bool(torch.isfinite(xa[far]).all())
    assert bool(torch.isnan(xb[1, 0, 20, 17])) and bool(torch.isnan(xa[1, 0, 20, 17]))
    check(f"fused map NaN pixel {layout} xhat away from it", torch.where(far, xb, 0.0), torch.where(far, xa, 0.0), XTOL)


# ------------------------------------------------------------------------------------------ 5. net.jvp
def test_jvp_with_a_map_under_the_knob():
    """The primal takes the fused map route, the tangent the fused tangent sweep at the primal's bit maps.  Against the
    float64 oracle at the device's own supports (tests/test_gpu_tangent.py's check and tolerances: 1e-5 on xhat,
    SPLIT_TOL on xdot and the gradients) and against the default route: xhat within XTOL, xdot within SPLIT_TOL.  The
    tangent is taken at the primal's supports, so the two routes' xdot are comparable at a rounding tolerance only where
    their supports are the same sets: this net, input and map have no near-tie that falls differently on the two tiers
    (every kernel is order-fixed, so that does not change from run to run), which is asserted first."""
    from cdlnet_video_amd import ops
    from test_gpu_datagrad import _case as datagrad_case
    from test_gpu_tangent import _direction, _vs_oracle
    # the net, input and map of test_sigma_map_runs_the_generic_tangent_vs_oracle: its codes are 10-90 % dense
    net, sd, x, y, _, mask, w = datagrad_case("2d", 18, (2, 1, 48, 40), 1, False, K=4, M=32, P=7)
    amap = 15.0 + 20.0 * torch.rand((2, 1, 48, 40), generator=torch.Generator().manual_seed(5))
    v = _direction(y, None, 41)[0]
    with torch.no_grad():
        xh0, xd0 = net.jvp(y.cuda(), v.cuda(), amap.cuda())
        outs0 = net._run(y.cuda(), amap.cuda(), 1, True)
    with _fused_map("blocked"):
        with torch.no_grad():
            outs = net._run(y.cuda(), amap.cuda(), 1, True)
        supports = [c.cpu() for c in outs[2:]] + [outs[1].cpu()]
        with ops.trace() as t:
            xh1, xd1 = _vs_oracle("fused map", net, sd, x, y, amap, mask, SPLIT_TOL, supports=supports)
            torch.cuda.synchronize()
    assert 4 in _stage_modes(t) and 2 in _stage_modes(t)             # the map forward, the plain reverse stage as tangent
    assert not [k for k in launch_sites(t) if any(n in k for n in GENERIC_KERNELS)]
    check("fused map jvp xhat vs the default route", xh1, xh0, XTOL)
    flips = sum(int(((a != 0) != (b != 0)).sum()) for a, b in zip(outs[1:], outs0[1:]))
    log(f"fused map jvp: support flips between the two tiers: {flips}")
    assert flips == 0, f"{flips} code elements are in one tier's support and not in the other's"
    check("fused map jvp xdot vs the default route", xd1, xd0, SPLIT_TOL)


def test_sure_loss_with_a_map_under_the_knob():
    """train.sure_loss (the exact divergence through net.jvp) takes the same route, forward and backward.  Its value
    mean(d^2) + 2 mean(s2 b xdot), d = y - xhat, against the default route's, at the project's two tolerances: xhat within
    XTOL of its maximum moves the first mean by at most mean|d + d'| XTOL max|xhat|, xdot within SPLIT_TOL of its maximum
    the second by at most 2 mean(s2 |b|) SPLIT_TOL max|xdot|."""
    from cdlnet_video_amd import loop, ops, train
    net, sd, x, y, _, mask, w = _case("2d", 61, (2, 1, 48, 40), 1, None, (2, 1, 48, 40), K=3, M=32, P=7)
    amap = _varying_map((2, 1, 48, 40), 62).cuda()
    yd = y.cuda()
    b = torch.randn(yd.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    res = []
    for knob in ("generic", "fused"):
        net.zero_grad(set_to_none=True)
        with loop.map_tier_scope(knob), ops.trace() as t:
            loss, xhat = train.sure_loss(net, yd, amap, b=b)
            loss.backward()
            torch.cuda.synchronize()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in net.named_parameters() if n != "g")
        res.append((float(loss.detach()), xhat.detach(), _stage_modes(t)))
    log(f"fused map sure_loss: generic {res[0][0]:.8e} fused {res[1][0]:.8e}")
    assert 4 not in res[0][2] and 6 not in res[0][2] and 4 in res[1][2] and 6 in res[1][2], (res[0][2], res[1][2])
    check("fused map sure_loss xhat", res[1][1], res[0][1], XTOL)
    with torch.no_grad():
        xdot0 = net.jvp(yd, b, amap)[1]                              # the default route's
    s2 = (amap / 255.0) ** 2
    bound = float(((yd - res[0][1]) + (yd - res[1][1])).abs().mean() * XTOL * res[0][1].abs().max()
                  + 2.0 * (s2 * b.abs()).mean() * SPLIT_TOL * xdot0.abs().max())
    log(f"fused map sure_loss: |difference| {abs(res[0][0] - res[1][0]):.3e} bound {bound:.3e}")
    assert abs(res[0][0] - res[1][0]) <= bound, (res[0][0], res[1][0], bound)


# ------------------------------------------------------------------------------------------ 6. windowed inference
def test_windows_run_the_fused_map_stage():
    import cdlnet_video_amd as cva
    from test_gpu_windowed import case, stages
    net, y, _, _, _, _ = case(1)
    amap = smooth_map((2, 1, 96, 80), 7).cuda()
    with torch.no_grad(), _fused_map("blocked"):
        full = net(y, amap)[0]
        with cva.ops.trace() as t:
            got = cva.denoise_windowed(net, y, amap, window=(32, 32), halo=4)
            torch.cuda.synchronize()
    assert stages(t) == {"k_stage"} and _stage_modes(t) == [4, 5], sorted(launch_sites(t))
    check("fused map windowed vs net(y, map)", got, full, XTOL)


# ------------------------------------------------------------------------------------------ 7. misaligned map buffers
@pytest.mark.parametrize("layout", LAYOUTS)
def test_map_buffers_on_a_guard_banded_misaligned_base(layout):
    """cmap, tslope and dcmap need float alignment only: on a 4-byte aligned base between guard bands the stage forward
    (first and later) and reverse give the aligned run's results bit for bit and write nothing outside dcmap."""
    import cdlnet_video_amd as cva
    from arena_util import Arena
    o = cva.ops
    M, P, N, H, W = 64, 7, 2, 33, 70
    gen = torch.Generator().manual_seed(9)
    g = o.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1)
    wA, wB = (0.15 * torch.randn(M, 1, P, P, generator=gen)).cuda(), (0.15 * torch.randn(M, 1, P, P, generator=gen)).cuda()
    r0, r1 = torch.randn(N, 1, H, W, generator=gen).cuda(), torch.randn(N, 1, H, W, generator=gen).cuda()
    tau = (0.01 + 0.05 * torch.rand(1, M, generator=gen)).expand(N, M).contiguous().cuda()
    cmap_c, tslope_c = 0.04 + 0.12 * torch.rand(N, 1, H, W, generator=gen), 0.5 * torch.rand(M, generator=gen)
    gup = torch.randn(N, M, H, W, generator=gen).cuda()
    frags, patches = o.fused_prep(wA, wB), o.fused_patches(g, "cuda")

    def run(cmap, tslope, dcmap):
        bits = o.fused_map(g, "cuda")
        z1 = o.fused_iter(g, r0, None, tau, frags, 1.0, patches, lay_out=layout, cmap=cmap, tslope=tslope)
        z2 = o.fused_iter(g, r1, z1, tau, frags, -1.0, patches, map_out=bits, lay_in=layout, lay_out="nchw", cmap=cmap,
                          tslope=tslope)
        dtp = torch.empty(2 * o.fused_tiles(g), M, device="cuda")
        du = o.fused_stage_bwd(g, r0, gup, bits, frags, patches, dtp, True, lay_in="nchw", lay_out=layout, cmap=cmap,
                               tslope=tslope, dcmap=dcmap)
        o.fused_stage_bwd(g, r1, gup, bits, frags, patches, dtp, True, lay_in="nchw", lay_out=layout, cmap=cmap,
                          tslope=tslope, dcmap=dcmap, dcmap_add=True)
        torch.cuda.synchronize()                                   # (padding pixels of a blocked buffer are never written)
        return z2, bits, o.fused_to_nchw(g, du, layout), dtp.clone(), dcmap.clone()

    ref = run(cmap_c.cuda(), tslope_c.cuda(), torch.empty(N, 1, H, W, device="cuda"))
    arena = Arena("cuda")
    cmap, tslope = arena.put(cmap_c, 1, "cmap"), arena.put(tslope_c, 1, "tslope")
    dcmap = arena.out((N, 1, H, W), 1, name="dcmap")
    assert cmap.data_ptr() % 16 == 4 and tslope.data_ptr() % 16 == 4 and dcmap.data_ptr() % 16 == 4
    got = run(cmap, tslope, dcmap)
    arena.check()
    arena.assert_defined(dcmap)
    for name, a, b in zip(("z", "bit map", "du", "dtau partials", "dcmap"), ref, got):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(got[4]).all()) and float(got[4].abs().max()) > 0
