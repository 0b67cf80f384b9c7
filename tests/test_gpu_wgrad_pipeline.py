"""The software-pipelined filter-gradient kernel (k_wgrad2d: fat operand one row block ahead, across tile and image
boundaries; one persistent workgroup per CU) and the reverse sweep's one reduction launch per iteration (k_sweep_reduce)."""
import pytest
import torch

from gpu_util import check

pytestmark = pytest.mark.gpu

LAYOUTS = ["nchw", "blocked", "blocked_bf16"]

# (N, M, P, H, W): one tile, N = 1 | 3 tiles | 9 tiles, one wave row half empty | H, W off 16 / 64 / 128, partial tiles
# on both edges | 1088 tiles: several per workgroup in both modes, so the prefetch crosses tile and image boundaries and
# the last round of the persistent grid is partly idle
WGRAD_SHAPES = [(1, 64, 7, 16, 64), (1, 64, 7, 40, 64), (3, 32, 5, 41, 50), (2, 64, 7, 50, 200), (1, 64, 3, 23, 130),
                (17, 32, 5, 250, 250)]


def _operands(o, N, M, P, H, W, layout):
    gen = torch.Generator().manual_seed(13 * H + W + M)
    geom = o.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1)
    X = torch.randn(N, M, H, W, generator=gen) * (torch.rand(N, M, H, W, generator=gen) < 0.5)
    if layout == "blocked_bf16":
        X = X.bfloat16().float()          # what that storage can hold: the generic reference sees the same values
    X = X.cuda()
    T = torch.randn(N, 1, H, W, generator=gen).cuda()
    X2 = torch.randn(N, M, H, W, generator=gen).bfloat16().float().cuda()
    T2 = torch.randn(N, 1, H, W, generator=gen).cuda()
    return geom, X, T, X2, T2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N,M,P,H,W", WGRAD_SHAPES)
@pytest.mark.parametrize("precision,tol", [("split3", 2e-5), ("bf16", 3e-2)])    # test_fused_filter_gradients_vs_generic's
def test_single_operator_wgrad_vs_generic(N, M, P, H, W, layout, precision, tol):
    import cdlnet_video_amd as cva
    o = cva.ops
    geom, X, T, X2, T2 = _operands(o, N, M, P, H, W, layout)
    ws = o.fused_wgrad_workspace(geom, "cuda")
    ref = o.wgrad(geom, X, T, 1.0)
    Xl, X2l = o.fused_from_nchw(geom, X, layout), o.fused_from_nchw(geom, X2, layout)
    tag = f"wgrad-pipeline[{precision},{layout}] N{N}M{M}P{P} {H}x{W}"
    for rev in (False, True):
        (single, none) = o.fused_wgrad(geom, ws, Xl, T, 1.0, precision=precision, layout=layout, tiles_reversed=rev)
        assert none is None
        check(f"{tag} rev={int(rev)} single", single, ref, tol)
        # the same gradient through either slot of the two-operator launch: other tiles per wave group, so another
        # grouping of the fp32 partial sums -- the tolerance against the reference holds between the two as well
        pair0, other = o.fused_wgrad(geom, ws, Xl, T, 1.0, X2l, T2, -1.0, precision, layout=layout, tiles_reversed=rev)
        other_b, pair1 = o.fused_wgrad(geom, ws, X2l, T2, -1.0, Xl, T, 1.0, precision, layout=layout, tiles_reversed=rev)
        check(f"{tag} rev={int(rev)} pair slot 0", pair0, ref, tol)
        check(f"{tag} rev={int(rev)} pair slot 1", pair1, ref, tol)
        check(f"{tag} rev={int(rev)} single vs slot 0", single, pair0, tol)
        check(f"{tag} rev={int(rev)} single vs slot 1", single, pair1, tol)
        check(f"{tag} rev={int(rev)} second operator", other, o.wgrad(geom, X2, T2, -1.0), tol)
        assert torch.equal(other, other_b)                    # the two slots run the same code on the same tiles
        (again, _) = o.fused_wgrad(geom, ws, Xl, T, 1.0, precision=precision, layout=layout, tiles_reversed=rev)
        assert torch.equal(single, again)                                     # deterministic


def _net_and_forward(cva, K, M, P, N, H, W, layout):
    from cdlnet_video_amd import loop
    o = cva.ops
    torch.manual_seed(41)
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=1, t0=5e-3, adaptive=True, init=True).cuda()
    y = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    yp, _, _, _ = o.preprocess(y, 1, None)
    g = o.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1)
    c = torch.linspace(0.07, 0.12, N).cuda()
    tau = o.thresholds(net.t.detach(), c, N)
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    xp, _, codes, resid, maps = loop._forward_fused(g, yp, None, tau, A, B, True, True, layout=layout)
    g_xp = torch.randn(xp.shape, generator=torch.Generator().manual_seed(4)).cuda()
    return g, yp, c, A, B, codes, resid, maps, g_xp


def _stepwise_reverse(o, g, K, yp, c, A, B, codes, resid, maps, g_xp, layout, dt, dyp, dtau):
    """The launches of cdl_fused2d_backward through the stand-alone entry points, each with its own reduction kernel:
    dA_k from the reverse stage, dB_k from the single-operator k_wgrad2d, the thresholds from k_dtau_reduce."""
    dev = yp.device
    dA, dB = [None] * K, [None] * K
    patches = o.fused_patches(g, dev)
    ws = o.fused_wgrad_workspace(g, dev)
    dtp = torch.empty((o.fused_tiles(g), g.M), device=dev, dtype=torch.float32)
    thin, du_next = g_xp, None
    (dB[0],) = o.fused_wgrad(g, ws, codes[K - 1], g_xp, 1.0)[:1]
    for k in range(K - 1, -1, -1):
        frags = o.fused_prep(B[(k + 1) % K], A[k])
        du, dA[k] = o.fused_stage_bwd(g, thin, du_next, maps[k], frags, patches, dtp, k >= 1 or dyp is not None, "split3",
                                      lay_in="nchw" if k == K - 1 else layout, lay_out=layout,
                                      r2=resid[k - 1] if k >= 1 else yp, alpha=-1.0 if k >= 1 else 1.0, workspace=ws)
        o.fused_dtau_reduce(g, dtp, c, dt[k], dtau[k] if dtau is not None else None)
        if k == 0 and dyp is not None:
            o.fused_assemble(g, patches, acc=dyp, acc_add=K > 1, write_out=False)
        if k >= 1:
            q = o.fused_assemble(g, patches, None, None, -1.0, acc=dyp, acc_add=k < K - 1)
            (dB[k],) = o.fused_wgrad(g, ws, codes[k - 1], q, 1.0, layout=layout)[:1]
            thin = q
        du_next = du
    return dA, dB


@pytest.mark.parametrize("layout", ["nchw", "blocked"])
@pytest.mark.parametrize("K,with_data_grads", [(4, False), (4, True), (1, True), (2, False)])
def test_merged_reduction_is_bit_identical_to_the_standalone_reductions(hip_env, layout, K, with_data_grads):
    """One tile direction for every launch (CDL_FUSED_SNAKE=0), so the sweep and the step-wise launches group their
    partial sums alike: dA_k, dB_k, dt and the per-image dtau are the same bits.  40 x 72: partial tiles, 6 per image."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    M, P, N, H, W = 64, 7, 3, 40, 72
    g, yp, c, A, B, codes, resid, maps, g_xp = _net_and_forward(cva, K, M, P, N, H, W, layout)
    hip_env("CDL_FUSED_SNAKE", "0")
    outs = []
    for sweep in ("c", "stepwise"):
        dt = torch.zeros(K, 2, M, device="cuda")
        dyp = torch.full_like(yp, float("nan")) if with_data_grads else None
        dtau = torch.full((K, N, M), float("nan"), device="cuda") if with_data_grads else None
        if sweep == "c":
            dA, dB = loop._backward_fused(g, K, yp, None, c, A, B, codes, resid, g_xp, None, dt, maps=maps, layout=layout,
                                          dyp=dyp, dtau=dtau)
        else:
            dA, dB = _stepwise_reverse(o, g, K, yp, c, A, B, codes, resid, maps, g_xp, layout, dt, dyp, dtau)
        outs.append((dA, dB, dt, dyp, dtau))
    for k in range(K):
        assert torch.equal(outs[0][0][k], outs[1][0][k]), f"dA[{k}]"
        assert torch.equal(outs[0][1][k], outs[1][1][k]), f"dB[{k}]"
    assert torch.equal(outs[0][2], outs[1][2])
    assert bool(outs[0][2].abs().sum() > 0) and all(bool(w.abs().sum() > 0) for w in outs[0][0] + outs[0][1])
    if with_data_grads:
        assert torch.equal(outs[0][3], outs[1][3]) and torch.equal(outs[0][4], outs[1][4])
        assert bool(torch.isfinite(outs[0][3]).all()) and bool(torch.isfinite(outs[0][4]).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K", [1, 3])
def test_reverse_sweep_is_bit_reproducible(layout, K):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    M, P, N, H, W = 64, 7, 2, 56, 136
    g, yp, c, A, B, codes, resid, maps, g_xp = _net_and_forward(cva, K, M, P, N, H, W, layout)
    runs = []
    for _ in range(2):
        dt = torch.zeros(K, 2, M, device="cuda")
        dyp = torch.empty_like(yp)
        dtau = torch.empty((K, N, M), device="cuda")
        dA, dB = loop._backward_fused(g, K, yp, None, c, A, B, codes, resid, g_xp, None, dt, maps=maps, layout=layout,
                                      dyp=dyp, dtau=dtau)
        runs.append([t.clone() for t in dA + dB + [dt, dyp, dtau]])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
