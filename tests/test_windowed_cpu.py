"""Windowed inference on the host side: the planner's invariants, the assembly as a partition of
unity, exact halos against the untiled float64 restatement of the loop (tests/windowed_restate.py) through
loop.run_windows(sweep=...), the automatic plan at a user's frame and clip size (geometry only: the fused tiers' admission
rules are host functions), the refusals and the export."""
import pytest
import torch

from windowed_restate import make_sweep, random_net

EXACT = 1e-12        # halo R: the windowed float64 result against the untiled one
SEAM = 1e-3          # halo one stride short: must differ by more than this


def W():
    import cdlnet_video_amd as cva
    return cva.windowed


# ------------------------------------------------------------------------------------------ planner
AXIS_CASES = [(L, c, h, s) for s in (1, 2, 3) for L in (s, 12 * s, 37 * s, 96 * s)
              for c in (s, 5 * s, 16 * s, 96 * s, None) for h in (0, s, 4 * s, 20 * s)]


@pytest.mark.parametrize("L,c,h,s", AXIS_CASES)
def test_plan_axis_invariants(L, c, h, s):
    axis = W().plan_axis(L, c, h, s)
    # cores partition the axis exactly once
    assert axis[0].c0 == 0 and axis[-1].c1 == L
    assert all(a.c1 == b.c0 for a, b in zip(axis, axis[1:])) and all(a.c0 < a.c1 for a in axis)
    for a in axis:
        assert 0 <= a.w0 <= a.c0 and a.c1 <= a.w1 <= L                    # inside the padded frame, around the core
        assert all(v % s == 0 for v in (a.w0, a.w1, a.c0, a.c1))          # origins and extents on the stride
        assert a.w0 == 0 or a.c0 - a.w0 >= h                             # the requested halo, except at a frame border
        assert a.w1 == L or a.w1 - a.c1 >= h
    assert len({a.w1 - a.w0 for a in axis}) == 1                          # one shape per plan
    want = L if c is None else min(c + 2 * h, L)
    assert axis[0].w1 - axis[0].w0 == want
    if want == L:
        assert len(axis) == 1


def test_plan_windows_is_the_product_of_its_axes():
    w = W()
    plan = w.plan_windows((20, 48, 40), 2, (8, 16, None), (2, 4, 4))
    assert plan.counts == (3, 3, 1) and plan.shape == (12, 24, 40) and len(plan.windows) == 9
    assert plan.windows[0] == (0, 0, 0) and plan.windows[1] == (0, 1, 0)
    owned = torch.zeros(plan.dims)
    for idx in plan.windows:
        owned[tuple(slice(a[i].c0, a[i].c1) for a, i in zip(plan.axes, idx))] += 1
    assert bool((owned == 1).all())
    assert plan.overhead == pytest.approx(3 * 12 / 20 * 3 * 24 / 48)
    assert plan.slices(4) == (slice(6, 18), slice(12, 36), slice(0, 40))                 # cores [8, 16) x [16, 32)
    assert plan.slices(4, scale=2) == (slice(3, 9), slice(6, 18), slice(0, 20))          # the same window on the code grid


@pytest.mark.parametrize("bad", [dict(core=5, halo=2, s=2), dict(core=4, halo=3, s=2), dict(core=0, halo=0, s=1),
                                 dict(core=4, halo=-1, s=1)])
def test_plan_axis_refuses_what_is_off_the_stride(bad):
    with pytest.raises(ValueError):
        W().plan_axis(24, bad["core"], bad["halo"], bad["s"])


def test_exact_halo():
    w = W()
    assert w.exact_halo(30, (7, 7), 1) == (180, 180) and w.exact_halo(20, (5, 5, 5), 1) == (80, 80, 80)
    assert w.exact_halo(2, (3, 3), 2) == (4, 4) and w.exact_halo(3, (3, 5), 4) == (8, 12) and w.exact_halo(1, (3, 1), 3) == (3, 0)


# ------------------------------------------------------------------------------------------ partition of unity
@pytest.mark.parametrize("blend", ["crop", "ramp"])
@pytest.mark.parametrize("dims,s,cores,halo", [
    ((48, 40), 1, (16, 16), (4, 4)), ((48, 40), 2, (16, 12), (4, 6)), ((37, 29), 1, (5, 7), (3, 0)),
    ((30, 26), 1, (4, 6), (9, 8)),                    # halos wider than the cores: three windows overlap
    ((20, 24, 20), 1, (8, 8, None), (1, 4, 4)), ((12, 16, 20), 2, (4, 8, 8), (2, 2, 4)),
])
def test_identity_sweep_returns_the_frame_bit_for_bit(dims, s, cores, halo, blend):
    from cdlnet_video_amd import loop
    plan = W().plan_windows(dims, s, cores, halo)
    assert len(plan.windows) > 1
    yp = torch.randn((2, 3) + dims, generator=torch.Generator().manual_seed(1))
    for mb in (None, 1, 5):
        out = loop.run_windows(yp, None, None, None, None, None, s, plan, blend=blend, max_batch=mb,
                               sweep=lambda yp_w, mask_w, c_w: yp_w)
        assert out.shape == yp.shape and torch.equal(out, yp)


def test_ramp_weights_are_the_analytic_cross_fade():
    """Window i contributes the constant i: across an overlap the result climbs linearly from i to i + 1."""
    w = W()
    axis = w.plan_axis(40, 16, 4)
    pieces = [torch.full((1, 1, a.w1 - a.w0), float(i), dtype=torch.float64) for i, a in enumerate(axis)]
    out = w.Plan((40,), 1, (axis,), (4,)).assemble(pieces, "ramp")[0, 0]
    want = torch.zeros(40, dtype=torch.float64)
    want[12:24] = torch.arange(1, 13, dtype=torch.float64) / 13         # windows 0 | 1 overlap on [12, 24)
    want[24:36] = 1.0 + torch.arange(1, 13, dtype=torch.float64) / 13   # the last window, shifted inward to [16, 40), overlaps
    want[36:] = 2.0                                                      # on [16, 36): clipped to the cores' centres 24, 36
    assert [(a.w0, a.w1) for a in axis] == [(0, 24), (12, 36), (16, 40)]
    assert torch.allclose(out, want, atol=1e-15, rtol=0)


# ------------------------------------------------------------------------------------------ exact halos
def _frame(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64)


EXACT_CASES = [
    # label, (N, C, *padded dims), s, K, P, M, cores, masked, sigma form
    ("2-D s1", (2, 1, 48, 40), 1, 2, (3, 3), 4, (16, 16), False, "per-sample"),
    ("2-D s2", (1, 1, 48, 40), 2, 2, (3, 3), 4, (16, 16), False, "map"),
    ("2-D s1 K3 P5 C3 mask", (1, 3, 64, 44), 1, 3, (5, 5), 4, (16, None), True, None),
    ("3-D s1", (1, 1, 20, 24, 20), 1, 2, (3, 3, 3), 3, (8, 8, None), False, "per-sample"),
    ("3-D s2", (1, 1, 24, 24, 16), 2, 2, (3, 3, 3), 3, (8, 8, None), False, None),
]


@pytest.mark.parametrize("label,shape,s,K,P,M,cores,masked,sform", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_halo_reproduces_the_untiled_restatement(label, shape, s, K, P, M, cores, masked, sform):
    from cdlnet_video_amd import loop
    w = W()
    N, C, dims = shape[0], shape[1], shape[2:]
    A, B, t = random_net(K, M, C, P, seed=11)
    sweep = make_sweep(A, B, t, s)
    yp = _frame(shape, 12)
    mask_p = (torch.rand(shape, generator=torch.Generator().manual_seed(13)) < 0.6).double() if masked else None
    grid = tuple(d // s for d in dims)
    c = {None: None, "per-sample": 0.05 + 0.1 * torch.arange(N, dtype=torch.float64),
         "map": 0.05 + 0.1 * torch.rand((N, 1) + grid, generator=torch.Generator().manual_seed(14), dtype=torch.float64)}[sform]
    full = sweep(yp, mask_p, c)
    R = w.exact_halo(K, P, s)
    assert R == tuple(-(-2 * K * (p // 2) // s) * s for p in P)
    plan = w.plan_windows(dims, s, cores, R)
    assert len(plan.windows) > 1
    for mb in (None, 2):                               # "crop": a window is exact on its core, not in its halo
        got = loop.run_windows(yp, mask_p, c, None, None, None, s, plan, blend="crop", max_batch=mb, sweep=sweep)
        err = float((got - full).abs().max())
        assert err <= EXACT, (label, mb, err)
    # one stride short on the axes that are cut: a seam the comparison sees
    short = tuple(r - s if cr is not None else r for r, cr in zip(R, cores))
    got = loop.run_windows(yp, mask_p, c, None, None, None, s, w.plan_windows(dims, s, cores, short), sweep=sweep)
    seam = float((got - full).abs().max())
    print(f"windowed {label}: halo one stride short differs by {seam:.3e}")
    assert seam > SEAM, (label, seam)


# ------------------------------------------------------------------------------------------ the automatic plan
@pytest.mark.parametrize("label,C,M,P,K,dims,cut", [
    ("flagship 2160 x 4096", 1, 64, (7, 7), 30, (2160, 4096), 0),
    ("cfg3 clip 16 x 1080 x 1920", 1, 48, (5, 5, 5), 20, (16, 1080, 1920), 1),       # exact temporal halo: depth stays whole
])
def test_auto_plan_on_real_sizes(label, C, M, P, K, dims, cut):
    w = W()
    accepts = w.fused_accepts(C, M, P, 1)
    assert not accepts(dims)                                            # the whole sample is refused by the fused tiers
    halo = w.exact_halo(K, P, 1)
    cores = w.auto_cores(dims, 1, halo, accepts)
    plan = w.plan_windows(dims, 1, cores, halo)
    print(f"windowed auto plan {label}: {plan.describe()}")
    assert len(plan.windows) > 1 and accepts(plan.shape)                # every window (one shape) is accepted
    assert [i for i, c in enumerate(cores) if c is not None] == [cut]   # the first axis that can be cut, and only it
    # the fewest windows that admit: one window fewer on that axis is refused
    n = plan.counts[cut]
    fewer = -(-dims[cut] // (n - 1)) + 2 * halo[cut]
    assert n == 2 or not accepts(tuple(fewer if a == cut else d for a, d in enumerate(dims)))
    assert w.auto_cores(dims, 1, halo, accepts) == cores                # deterministic


def test_auto_plan_order_of_the_axes():
    w = W()
    accepts = w.fused_accepts(1, 48, (5, 5, 5), 1)
    shape = lambda dims, cores, halo: w.plan_windows(dims, 1, cores, halo).shape
    # depth first: five frames of 1080p fit, so four windows of four
    dims, halo = (16, 1080, 1920), (0, 80, 80)
    cores = w.auto_cores(dims, 1, halo, accepts)
    assert cores == (4, None, None) and accepts(shape(dims, cores, halo)) and not accepts((6,) + dims[1:])
    # a temporal halo of 2 leaves depth a core of one frame, less than twice the halo: the height is cut instead
    halo = (2, 80, 80)
    assert w.largest_core(dims, 1, halo, accepts, 0, (None,) * 3) == 1
    assert w.auto_cores(dims, 1, halo, accepts) == (None, 180, None)
    # ... unless nothing else can be cut
    assert w.auto_cores((16, 1080, 1920), 1, (2, 540, 960), accepts) == (1, None, None)
    # no axis settles it alone: depth stays at twice its halo and the height is cut as well
    dims, halo = (64, 4096, 4096), (4, 80, 80)
    cores = w.auto_cores(dims, 1, halo, accepts)
    assert cores[0] == 8 and cores[1] is not None and cores[2] is None and accepts(shape(dims, cores, halo))
    # not even that: one core for all three axes
    dims, halo = (2048, 2048, 2048), (80, 80, 80)
    cores = w.auto_cores(dims, 1, halo, accepts)
    assert len(set(cores)) == 1 and accepts(shape(dims, cores, halo))
    assert not accepts(tuple(c + 1 + 2 * h for c, h in zip(cores, halo)))


def test_auto_plan_last_axis_core_is_a_multiple_of_32_code_pixels():
    w = W()
    # a single row of blocks: height cannot be cut (the halo leaves no room), so the width is
    dims, halo = (300, 40000), (180, 180)
    accepts = w.fused_accepts(1, 64, (7, 7), 1)
    assert not accepts(dims)
    cores = w.auto_cores(dims, 1, halo, accepts)
    assert cores[0] is None and cores[1] % 32 == 0
    assert accepts(w.plan_windows(dims, 1, cores, halo).shape)


def test_small_frame_and_unsupported_net_plan_as_one_window():
    w = W()
    assert w.auto_cores((256, 256), 1, (180, 180), w.fused_accepts(1, 64, (7, 7), 1)) == (None, None)
    assert len(w.plan_windows((256, 256), 1, (None, None), (180, 180)).windows) == 1
    # 9 x 9 filters: no fused tier at any size -- the route of net(y)
    acc = w.fused_accepts(1, 64, (9, 9), 1)
    assert not acc((64, 64)) and w.auto_cores((4096, 4096), 1, (16, 16), acc) == (None, None)


# ------------------------------------------------------------------------------------------ refusals, export
def test_refusals_come_before_any_device_use():
    import cdlnet_video_amd as cva
    y = torch.rand(1, 1, 32, 32)
    kw = dict(K=2, M=8, P=5, s=1, C=1, init=False)
    for cls in (cva.CDLNet_CSR, cva.CDLNet_CSRf2):
        with pytest.raises(NotImplementedError, match="frame to frame"), torch.no_grad():
            cva.denoise_windowed(cls(**kw), y)
    vid = cva.CDLNetVideo(K=2, M=8, P=[3, 3, 3], init=False, residual=True)
    with pytest.raises(NotImplementedError, match="residual"), torch.no_grad():
        cva.denoise_windowed(vid, torch.rand(1, 1, 4, 16, 16))
    net = cva.CDLNet(**kw)
    with pytest.raises(NotImplementedError, match="`y` requires grad"):
        cva.denoise_windowed(net, y.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="`sigma` requires grad"):
        cva.denoise_windowed(net, y, torch.tensor([25.0], requires_grad=True))
    with pytest.raises(NotImplementedError, match="parameters require grad"):
        cva.denoise_windowed(net, y)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU"):
            cva.denoise_windowed(net, y)
        for bad in (dict(window=(16,)), dict(window=(16, 16, 16)), dict(window=0), dict(window=-8), dict(window=2.5),
                    dict(window="big"), dict(halo="none"), dict(halo=-1), dict(halo=(4,)), dict(halo=1.5),
                    dict(blend="feather"), dict(max_batch=0)):
            with pytest.raises(ValueError):
                cva.denoise_windowed(net, y, **bad)
        net2 = cva.CDLNet(K=2, M=8, P=5, s=2, C=1, init=False)
        for bad in (dict(window=7), dict(halo=3)):                      # off the stride
            with pytest.raises(ValueError):
                cva.denoise_windowed(net2, y, **bad)


def test_export():
    import cdlnet_video_amd as cva
    assert cva.denoise_windowed is cva.windowed.denoise
    assert "denoise_windowed" in cva.__all__ and "windowed" in cva.__all__
    from cdlnet_video_amd import loop
    assert callable(loop.run_windows) and callable(loop._forward_sweep)
