"""Per-frame noise levels on the fused generic tier: under `loop.set_frame_tier("fused")` a CDLNetVideo
call whose sigma holds one level per (sample, frame) stays on the tile kernel k_stage_g (or, with CDL_FUSEDG_STRIP=1, on
k_stripg), which then reads its thresholds from row n * D + zd of an (N*D, M) table.

1. equal levels on every frame of a sample against the per-sample fused call: the same launches with the same numbers, so
   bit for bit -- dt[:,1] included (the same partial rows, in the same order, with the same weights);
2. levels that differ for every (sample, frame) against the default (generic) route and against the oracle's autograd at
   identical supports; under the fp32 arithmetic the knob changes nothing;
3. one frame whose level makes its thresholds negative;
4. the launch trace with and without the knob;
5. one cell of each on k_stripg (the `kernel` parameter);
6. jvp, sure_loss, forward_generator, denoise_windowed and train_step under the knob against the same call without it.

The cases, and why their levels tell a wrong row index apart, are in tests/frame_levels_util.py and
tests/test_frame_levels_cpu.py.  Tolerances are tests/test_gpu_sigmamap.py's."""
import copy
import functools

import pytest
import torch

from frame_levels_util import CASES, REFUSED, TANGENT_CASE, build
from gpu_util import check, launch_sites, log
from sigmamap_util import oracle_grads
from test_gpu_sigmamap import SPLIT_TOL, XTOL, _run_all

pytestmark = pytest.mark.gpu

STAGE = {"tile": "cdl_fusedg.hip:k_stage_g<", "stripg": "cdl_stripg.hip:k_stripg<"}
GENERIC_KERNELS = ("k_ana_m", "k_synth_m")
FUSED_FILES = {"cdl_fusedg.hip", "cdl_stripg.hip", "cdl_strip.hip", "cdl_fused2d.hip"}
CELLS = [(label, "tile") for label in sorted(CASES)] + [("A", "stripg")]
IDS = [f"{label}-{kernel}" for label, kernel in CELLS]
SMALL = [("A", "tile"), ("A", "stripg")]
LOSS_ATOL = 1e-5     # a loss of xhat (and xdot) that moved by XTOL: worked out where it is used
TANGENT_SEED = 71


@functools.lru_cache(maxsize=None)
def case(label):
    net, sd, x, y, mask, w, lev = build(label)
    return net.cuda(), sd, x, y, mask, w, lev


@pytest.fixture
def select(hip_env):
    """The kernel behind the cdl_fusedg_* entry points, chosen the way tests/test_gpu_fusedg_cells.py chooses it."""
    def choose(kernel):
        if kernel == "stripg":
            hip_env("CDL_FUSEDG_STRIP", "1")
    return choose


def knob():
    from cdlnet_video_amd import loop
    return loop.frame_tier_scope("fused")


def stage_records(trace, kernel):
    return [r for k, v in launch_sites(trace).items() if k.startswith(STAGE[kernel]) for r in v]


def takes(label):
    """Whether the fused generic tier has a plan for the case; C has none (tests/frame_levels_util.py REFUSED)."""
    from cdlnet_video_amd import ops
    cfg = CASES[label]
    N, C = cfg["shape"][:2]
    P = tuple(cfg["P"])
    ok = ops.fusedg_supported(ops.Geometry.make(N, C, cfg["M"], cfg["shape"][2:], P, tuple(p // 2 for p in P), 1))
    assert ok == (label not in REFUSED), label
    return ok


def assert_same_run(a, b, tag):
    """Two _run_all results of the same launches: every output and gradient bit for bit."""
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]), tag
    assert all(torch.equal(ca, cb) for ca, cb in zip(a[6], b[6])) and all(torch.equal(a[3][n], b[3][n]) for n in a[3]), tag


def assert_on_the_fused_tier(trace, kernel, tag):
    sites = launch_sites(trace)
    assert stage_records(trace, kernel), (tag, sorted(sites))
    other = STAGE["stripg" if kernel == "tile" else "tile"]
    assert not [k for k in sites if k.startswith(other) or any(name in k for name in GENERIC_KERNELS)], (tag, sorted(sites))


# ------------------------------------------------------------------------------------------ 1. equal levels on every frame
@pytest.mark.parametrize("label,kernel", CELLS, ids=IDS)
def test_equal_levels_equal_the_per_sample_fused_call(label, kernel, select):
    from cdlnet_video_amd import ops
    select(kernel)
    net, sd, x, y, mask, w, _ = case(label)
    N, D, K, M = y.shape[0], y.shape[2], CASES[label]["K"], CASES[label]["M"]
    per = (torch.linspace(15.0, 35.0, N) if N > 1 else torch.full((1,), 25.0)).reshape(N, 1, 1, 1, 1)
    frame = per.expand(N, 1, D, 1, 1).contiguous()
    with knob():
        with ops.trace() as ta:
            a = _run_all(net, x, y, per, mask, w)                 # one level per sample: the fused generic tier, as ever
            torch.cuda.synchronize()
        with ops.trace() as tb:
            b = _run_all(net, x, y, frame, mask, w)
            torch.cuda.synchronize()
    tag = f"frame levels equal {label} [{kernel}]"
    if not takes(label):
        # no fused plan takes the geometry: the knob changes nothing -- per-sample levels run the generic tier as ever, the
        # frame form its dense map (tests/test_gpu_sigmamap.py test_constant_map_equals_per_sample_path's comparison)
        assert not ((ta.files() | tb.files()) & FUSED_FILES)
        assert_same_run(_run_all(net, x, y, frame, mask, w), b, tag)
        check(f"{tag} xhat", b[0], a[0], XTOL)
        check(f"{tag} dL/dy", b[4], a[4], SPLIT_TOL)
        check(f"{tag} sum over frames of dL/dsigma", b[5].sum(2, keepdim=True), a[5], SPLIT_TOL)
        for name in a[3]:
            check(f"{tag} grad {name}", b[3][name], a[3][name], SPLIT_TOL)
        return
    assert_on_the_fused_tier(ta, kernel, tag)
    assert_on_the_fused_tier(tb, kernel, tag)
    assert len(stage_records(ta, kernel)) == len(stage_records(tb, kernel)) == 3 * K        # forward, reverse, the codes' forward
    assert torch.equal(a[0], b[0]), f"{tag}: xhat"
    assert torch.equal(a[1], b[1]), f"{tag}: z_K"
    assert len(a[6]) == len(b[6]) == K and all(torch.equal(ca, cb) for ca, cb in zip(a[6], b[6])), f"{tag}: codes"
    assert torch.equal(a[4], b[4]), f"{tag}: dL/dy"
    assert set(a[3]) == set(b[3]) and len(a[3]) == 2 * K + 1    # t, A_k, B_k (D is B_0)
    for name in a[3]:
        if name != "t":
            assert torch.equal(a[3][name], b[3][name]), f"{tag}: grad {name}"
    ta_, tb_ = a[3]["t"].reshape(K, 2, M), b[3]["t"].reshape(K, 2, M)
    assert torch.equal(ta_[:, 0], tb_[:, 0]), f"{tag}: dt[:,0]"
    assert torch.equal(ta_[:, 1], tb_[:, 1]), f"{tag}: dt[:,1]"  # the same rows and weights in the same order
    assert a[5].shape == per.shape and b[5].shape == frame.shape
    check(f"{tag} sum over frames of dL/dsigma", b[5].sum(2, keepdim=True), a[5], SPLIT_TOL)


# ------------------------------------------------------------------------------------------ 2. a level per (sample, frame)
@pytest.mark.parametrize("label,kernel", CELLS, ids=IDS)
def test_varying_levels_against_the_generic_route_and_the_oracle(label, kernel, select):
    from cdlnet_video_amd import ops
    select(kernel)
    net, sd, x, y, mask, w, lev = case(label)
    cfg = CASES[label]
    K = cfg["K"]
    with ops.trace() as ta:
        a = _run_all(net, x, y, lev, mask, w)                     # the default: expanded, the generic map route
        torch.cuda.synchronize()
    assert not (ta.files() & FUSED_FILES), ta.files()
    with knob(), ops.trace() as tb:
        b = _run_all(net, x, y, lev, mask, w)
        torch.cuda.synchronize()
    tag = f"frame levels varying {label} [{kernel}]"
    if takes(label):
        assert_on_the_fused_tier(tb, kernel, tag)
    else:                                                         # no fused plan: the same launches with and without the knob
        assert not (tb.files() & FUSED_FILES)
        assert_same_run(a, b, tag)
    check(f"{tag} xhat vs generic route", b[0], a[0], XTOL)
    check(f"{tag} z_K vs generic route", b[1], a[1], XTOL)
    dense = lev.expand((y.shape[0], 1) + tuple(y.shape[2:])).contiguous()
    xo, zo, lo, go, dyo, dso = oracle_grads(sd, x, y, w, dense, K=K, P=tuple(cfg["P"]), s=1, mask=mask, ndim=3, supports=b[6])
    check(f"{tag} xhat vs oracle", b[0], xo, XTOL)
    check(f"{tag} z_K vs oracle", b[1], zo, XTOL)
    assert b[4].shape == y.shape and b[5].shape == lev.shape and a[5].shape == lev.shape
    check(f"{tag} dL/dy", b[4], dyo, SPLIT_TOL)
    check(f"{tag} dL/dsigma", b[5], dso.double().sum_to_size(lev.shape).float(), SPLIT_TOL)
    seen = 0
    for name, ref in go.items():
        if name == "g" or ref is None:
            continue
        check(f"{tag} grad {name}", b[3][name], ref, SPLIT_TOL)
        seen += 1
    assert seen >= 1 + 2 * K


@pytest.mark.parametrize("label", ["A", "D"])
def test_fp32_arithmetic_ignores_the_knob(label):
    from cdlnet_video_amd import loop, ops
    net, sd, x, y, mask, w, lev = case(label)
    with loop.precision_scope("fp32"):
        a = _run_all(net, x, y, lev, mask, w)
        with knob(), ops.trace() as t:
            b = _run_all(net, x, y, lev, mask, w)
            torch.cuda.synchronize()
    assert t and not (t.files() & FUSED_FILES), t.files()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    assert all(torch.equal(a[3][n], b[3][n]) for n in a[3])
    assert b[5].shape == lev.shape


# ------------------------------------------------------------------------------------------ 3. a frame with negative thresholds
@pytest.mark.parametrize("label,kernel", SMALL + [("E", "tile")], ids=["A-tile", "A-stripg", "E-tile"])
def test_a_frame_with_negative_thresholds(label, kernel, select):
    from cdlnet_video_amd import ops
    select(kernel)
    net, sd, x, y, mask, w, lev = case(label)
    lev = lev.clone()
    lev[-1, 0, 1] = -300.0                                        # tau = t0 (1 + sigma / 255) < 0 on that frame, for every k and m
    with torch.no_grad():
        xa, za = net(y.cuda(), lev.cuda())
        with knob(), ops.trace() as t:
            xb, zb = net(y.cuda(), lev.cuda())
            torch.cuda.synchronize()
    tag = f"frame levels negative frame {label} [{kernel}]"
    assert_on_the_fused_tier(t, kernel, tag)
    check(f"{tag} xhat vs generic route", xb, xa, XTOL)
    check(f"{tag} z_K vs generic route", zb, za, XTOL)


@pytest.mark.parametrize("kernel", ["tile", "stripg"])
def test_only_the_negative_frame_takes_the_general_shrinkage(kernel, select):
    """One stage, thresholds per plane: a negative row changes its own plane's result -- there to the general form
    sign(u) max(|u| - tau, 0) -- and no other plane's by a bit."""
    import cdlnet_video_amd as cva
    o = cva.ops
    select(kernel)
    N, C, M, sp, P = 2, 1, 16, (4, 20, 70), (3, 3, 3)
    g = o.Geometry.make(N, C, M, sp, P, tuple(p // 2 for p in P), 1)
    D = sp[0]
    gen = torch.Generator().manual_seed(5)
    r = torch.randn(g.image_shape(), generator=gen).cuda()
    zin = (torch.randn(g.code_shape(), generator=gen) * (torch.rand(g.code_shape(), generator=gen) < 0.3)).cuda()
    wA = (torch.randn(g.filter_shape(), generator=gen) * 0.1).cuda()
    frags = o.fusedg_prep(g, wA, wA)
    patches = o.fusedg_patches(g, "cuda")
    tau = (torch.rand(N * D, M, generator=gen) * 0.6 + 0.01).cuda()
    row = 1 * D + 2                                              # sample 1, frame 2
    neg, zero = tau.clone(), tau.clone()
    neg[row], zero[row] = -0.05, 0.0
    with o.trace() as t:
        z_pos = o.fusedg_iter(g, r, zin, tau, frags, -1.0, patches, planes=True)
    assert stage_records(t, kernel)
    z_neg = o.fusedg_iter(g, r, zin, neg, frags, -1.0, patches, planes=True)
    u = o.fusedg_iter(g, r, zin, zero, frags, -1.0, patches, planes=True)[1, :, 2]        # ST(u, 0) = u
    others = torch.ones(N, D, dtype=torch.bool)
    others[1, 2] = False
    pick = lambda z: z.permute(0, 2, 1, 3, 4)[others.cuda()]
    assert torch.equal(pick(z_neg), pick(z_pos))
    want = torch.sign(u) * (u.abs() + 0.05)
    assert float((z_neg[1, :, 2] - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert not torch.equal(z_neg[1, :, 2], z_pos[1, :, 2])
    # and the refusal: per-plane thresholds are the tile / grouped strip kernels'; a row count that is not N * D is an error
    with pytest.raises(ValueError):
        o.fusedg_iter(g, r, zin, tau[:N], frags, -1.0, patches, planes=True)


def test_the_strip_kernel_refuses_the_flag():
    """k_strip (2-D, D == 1; here the stride-2 shape of the shipped checkpoints) has no per-plane form: CDL_EINVAL."""
    import cdlnet_video_amd as cva
    o = cva.ops
    g = o.Geometry.make(2, 1, 169, (50, 78), (7, 7), (3, 3), 2)
    assert o.fusedg_supported(g) and not o.fused_supported(g)
    gen = torch.Generator().manual_seed(6)
    r = torch.randn(g.image_shape(), generator=gen).cuda()
    wA = (torch.randn(g.filter_shape(), generator=gen) * 0.1).cuda()
    frags = o.fusedg_prep(g, wA, wA)
    patches = o.fusedg_patches(g, "cuda")
    tau = torch.full((2, 169), 0.1).cuda()
    o.fusedg_iter(g, r, None, tau, frags, 1.0, patches)
    with pytest.raises(cva._lib.HipKernelError, match="CDL_EINVAL"):
        o.fusedg_iter(g, r, None, tau, frags, 1.0, patches, planes=True)
    dt = torch.zeros(2, 169).cuda()
    partial = torch.zeros(o._fusedg_sizes(g)[2], 169).cuda()
    o.fusedg_dtau_reduce(g, partial, tau[:, 0].contiguous(), dt)
    with pytest.raises(cva._lib.HipKernelError, match="CDL_EINVAL"):
        o.fusedg_dtau_reduce(g, partial, tau[:, 0].contiguous(), dt, planes=True)


# ------------------------------------------------------------------------------------------ 4. the launch trace
@pytest.mark.parametrize("label,kernel", SMALL, ids=["A-tile", "A-stripg"])
def test_launch_trace_with_and_without_the_knob(label, kernel, select):
    from cdlnet_video_amd import ops
    select(kernel)
    net, sd, x, y, mask, w, lev = case(label)
    K = CASES[label]["K"]
    dense = lev.expand((y.shape[0], 1) + tuple(y.shape[2:])).contiguous()

    def run(sigma):
        for p in net.parameters():
            p.grad = None
        with ops.trace() as t:
            xhat, _ = net(y.cuda(), sigma.cuda())
            xhat.square().mean().backward()
            torch.cuda.synchronize()
        return t

    off, today = run(lev), run(dense)                             # without the knob: the launches of the dense map, today's
    assert [(r.file, r.func, r.note) for r in off] == [(r.file, r.func, r.note) for r in today]
    assert off and not (off.files() & FUSED_FILES), off.files()
    with knob():
        on = run(lev)
        on_dense = run(dense)                                     # a dense map is no frame level: the knob leaves it alone
    assert_on_the_fused_tier(on, kernel, f"frame levels trace {label} [{kernel}]")
    assert len(stage_records(on, kernel)) == 2 * K                # K forward stages, K reverse stages
    assert [(r.file, r.func, r.note) for r in on_dense] == [(r.file, r.func, r.note) for r in today]


# ------------------------------------------------------------------------------------------ 6. what depends on the sweep
def _both(fn, kernel, tag):
    """fn() without the knob and under it (there on the fused tier, by its launch trace)."""
    from cdlnet_video_amd import ops
    off = fn()
    with knob(), ops.trace() as t:
        on = fn()
        torch.cuda.synchronize()
    assert_on_the_fused_tier(t, kernel, tag)
    return off, on


@functools.lru_cache(maxsize=None)
def tangent_case():
    net, sd, x, y, mask, w, lev = build(TANGENT_CASE, TANGENT_SEED)
    return net.cuda(), y.cuda(), lev.cuda()


@pytest.mark.parametrize("kernel", ["tile", "stripg"])
def test_jvp_and_sure_loss_follow_the_route(kernel, select):
    """xdot is the derivative at the primal's supports, so the two routes are compared where their supports coincide
    (asserted first: tests/frame_levels_util.py TANGENT_CASE)."""
    import cdlnet_video_amd as cva
    select(kernel)
    net, yd, ld = tangent_case()
    tag = f"frame levels tangent [{kernel}]"
    v = torch.randn(yd.shape, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        ga, gb = _both(lambda: list(net.forward_generator(yd, ld)), kernel, tag)
        flips = sum(int(((p != 0) != (q != 0)).sum()) for p, q in zip(ga[:-1], gb[:-1]))
        assert flips == 0, f"{tag}: {flips} supports differ between the routes: xdot is not comparable on this clip"
        (xa, da), (xb, db) = _both(lambda: net.jvp(yd, v, ld), kernel, tag)
        check(f"{tag} jvp xhat", xb, xa, XTOL)
        check(f"{tag} jvp xdot", db, da, XTOL)
        sure = lambda: cva.train.sure_loss(net, yd, ld, generator=torch.Generator().manual_seed(4))
        (la, xa), (lb, xb) = _both(sure, kernel, tag)
        check(f"{tag} sure_loss xhat", xb, xa, XTOL)
        # the scalar: |d mean((y - xhat)^2)| <= 2 XTOL max|xhat| sqrt(mse) (about 2e-5 x 0.1) and the divergence term moves by
        # at most 2 max(sigma/255)^2 mean|b| XTOL max|xdot| (about 2 x 0.055 x 0.8 x 1e-5): together below 1e-5 absolute
        log(f"{tag} sure_loss generic {float(la):.8e} fused {float(lb):.8e}")
        assert abs(float(lb) - float(la)) <= LOSS_ATOL, (float(la), float(lb))

    def sure_grads():                                            # and its reverse sweeps run
        for p in net.parameters():
            p.grad = None
        loss, _ = cva.train.sure_loss(net, yd, ld, generator=torch.Generator().manual_seed(4))
        loss.backward()
        return {n: p.grad.clone() for n, p in net.named_parameters()}
    ga, gb = _both(sure_grads, kernel, tag)
    for name in ga:
        check(f"{tag} sure_loss grad {name}", gb[name], ga[name], SPLIT_TOL)


@pytest.mark.parametrize("label,kernel", SMALL, ids=["A-tile", "A-stripg"])
def test_generator_windows_and_training_step_follow_the_route(label, kernel, select):
    import cdlnet_video_amd as cva
    select(kernel)
    net, sd, x, y, mask, w, lev = case(label)
    tag = f"frame levels {label} [{kernel}]"
    yd, ld = y.cuda(), lev.cuda()
    with torch.no_grad():
        ga, gb = _both(lambda: list(net.forward_generator(yd, ld)), kernel, tag)
        assert len(ga) == len(gb) == CASES[label]["K"] + 1
        for i, (ca, cb) in enumerate(zip(ga, gb)):
            check(f"{tag} forward_generator item {i}", cb, ca, XTOL)
        # two windows along depth with an integer halo: the levels are cropped with their window
        y2 = torch.cat([yd, yd.flip(2)], 2)
        l2 = torch.cat([ld, ld.flip(2) + 1.5], 2)
        win = lambda: cva.denoise_windowed(net, y2, l2, window=(4, None, None), halo=(1, 0, 0))
        wa, wb = _both(win, kernel, tag)
        check(f"{tag} denoise_windowed", wb, wa, XTOL)
        whole = net(y2, l2)[0]
        assert float((wa - whole).abs().max()) > 0               # the windows were really cut (an approximate halo)

    # a training step with the levels awgn3d draws per frame
    batch = x.cuda()
    _, noise_std = cva.utils.awgn3d(batch, (10, 40), torch.Generator().manual_seed(8), per_frame=True)
    assert tuple(noise_std.shape) == (y.shape[0], 1, y.shape[2], 1, 1)

    def step():
        model = copy.deepcopy(net)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        loss, level = cva.train.train_step(model, opt, batch, noise_std, generator=torch.Generator().manual_seed(9))
        assert level is noise_std
        return loss
    la, lb = _both(step, kernel, tag)
    log(f"{tag} train_step loss generic {float(la):.8e} fused {float(lb):.8e}")
    # |d mean((x - xhat)^2)| <= 2 XTOL max|xhat| sqrt(mse), about 2e-5 x 0.1
    assert abs(float(lb) - float(la)) <= LOSS_ATOL, (float(la), float(lb))
