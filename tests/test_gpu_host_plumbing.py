"""The host plumbing on the device: a bad caller-provided buffer is refused without a launch, and the buffer tables of
every one-call sweep (ops._sweep_tables) give the same bits whether every code keeps its own buffer or two ping-pong --
at K = 1, 2, 3, where the tables have their edge cases (no residual, one buffer, the modulo).  Shapes: N = 2 and the
smallest extents that leave a partial tile in both axes of the tier's kernel."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [1, 2, 3]
# tier -> (C, M, spatial, P, stride)
GEOMS = {
    "generic": (2, 5, (13, 11), (3, 3), 1),           # no fused kernel takes it (M = 5)
    "fused": (1, 32, (20, 70), (5, 5), 1),            # 64 x 16 tiles: 2 x 2 of them, the last row and column partial
    "tile": (1, 24, (3, 17, 33), (3, 3, 3), 1),       # cdl_fusedg.hip's tile kernel, ragged tiles, M no multiple of 16
    "strip": (1, 24, (20, 36), (3, 3), 2),            # cdl_strip.hip: a 10 x 18 code plane, less than one 32-column strip
}


def _geom(tier):
    from cdlnet_video_amd import ops
    C, M, sp, P, s = GEOMS[tier]
    return ops.Geometry.make(2, C, M, sp, P, tuple(p // 2 for p in P), s)


@functools.lru_cache(maxsize=None)
def _inputs(tier, K):
    """Random operands of a K-iteration sweep on `tier`'s geometry (made once per case, never written)."""
    from cdlnet_video_amd import ops
    g = _geom(tier)
    gen = torch.Generator().manual_seed(100 * K + len(tier))
    rnd = lambda shape, sc=1.0: (sc * torch.randn(shape, generator=gen)).cuda()
    d = dict(g=g, yp=rnd(g.image_shape()), vp=rnd(g.image_shape()),
             mask=(torch.rand(g.image_shape(), generator=gen) > 0.3).float().cuda(),
             A=[rnd(g.filter_shape(), 0.1) for _ in range(K)], B=[rnd(g.filter_shape(), 0.1) for _ in range(K)])
    c = torch.rand(g.N, generator=gen).cuda()
    t, g1, g2 = ((torch.rand(K, 2, g.M, 1, 1, generator=gen) * sc).cuda() for sc in (0.05, 1.0, 1.0))
    d["tau"], d["gam1"], d["gam2"] = (ops.thresholds(p, c, g.N) for p in (t, g1, g2))
    for name in ("zp", "za", "zdp", "zda"):
        d[name] = rnd(g.code_shape(), 0.2)
    return d


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_tiers_are_the_ones_named():
    from cdlnet_video_amd import ops
    want = {"generic": (False, False), "fused": (True, False), "tile": (False, True), "strip": (False, True)}
    for tier, (fused, fusedg) in want.items():
        g = _geom(tier)
        assert (ops.fused_supported(g), ops.fusedg_supported(g) and not ops.fused_supported(g)) == (fused, fusedg), tier


# ------------------------------------------------------------------------------------------ refused without a launch
def test_strided_dt_k_is_refused_without_a_launch():
    from cdlnet_video_amd import ops
    g = _geom("generic")
    gk, z = torch.randn(g.code_shape(), device="cuda"), torch.randn(g.code_shape(), device="cuda")
    dt_k = torch.zeros(2, 2 * g.M, device="cuda")[:, ::2]                # (2, M), every second column
    with ops.trace() as t:
        with pytest.raises(ValueError, match="dt_k"):
            ops.tau_grad(g, gk, z, None, dt_k)
        torch.cuda.synchronize()
    assert list(t) == []


def test_float64_dyp_is_refused_without_a_launch():
    from cdlnet_video_amd import ops
    g = _geom("generic")
    q = torch.randn(g.image_shape(), device="cuda")
    dyp = torch.zeros(g.image_shape(), device="cuda", dtype=torch.float64)
    with ops.trace() as t:
        with pytest.raises(TypeError, match="dyp"):
            ops.dyp_split(g, q, None, dyp, False)
        torch.cuda.synchronize()
    assert list(t) == []


# ------------------------------------------------------------------------------------------ buffer tables
@pytest.mark.parametrize("csr", [False, True])
@pytest.mark.parametrize("K", KS)
def test_generic_forward_tables(K, csr):
    from cdlnet_video_amd import loop, ops
    d = _inputs("generic", K)
    g, yp, mask, A, B = d["g"], d["yp"], d["mask"], d["A"], d["B"]
    nb = (d["zp"], d["za"], d["gam1"], d["gam2"]) if csr else ()
    kept = ops.ista_forward(g, yp, mask, d["tau"], A, B, True, *nb)
    pong = ops.ista_forward(g, yp, mask, d["tau"], A, B, False, *nb)
    assert len(kept[2]) == K and len(kept[3]) == K - 1 and len(pong[2]) == 1 and pong[3] == []
    assert _same(kept[:2], pong[:2])
    if csr:
        step = loop._forward_csr_stepwise(g, yp, mask, d["tau"], d["gam1"], d["gam2"], d["zp"], d["za"], A, B, True)
        assert _same(kept[:2], step[:2]) and _same(kept[4], step[2]) and _same(kept[2], step[3]) and _same(kept[3], step[4])
    else:
        step = loop._forward_generic_stepwise(g, yp, mask, d["tau"], A, B, True, True)
        assert _same(kept[:2], step[:2]) and _same(kept[2], step[2]) and _same(kept[3], step[3])


@pytest.mark.parametrize("csr", [False, True])
@pytest.mark.parametrize("K", KS)
def test_generic_tangent_tables(K, csr):
    from cdlnet_video_amd import loop, ops
    d = _inputs("generic", K)
    g, vp, mask, A, B = d["g"], d["vp"], d["mask"], d["A"], d["B"]
    if csr:
        args = (g, vp, mask, d["tau"], d["gam1"], d["gam2"], d["zp"], d["za"], d["zdp"], d["zda"], A, B)
        us = ops.ista_forward(g, d["yp"], mask, d["tau"], A, B, True, d["zp"], d["za"], d["gam1"], d["gam2"])[4]
        kept = ops.csr_tangent_forward(*args, us, True)
        pong = ops.csr_tangent_forward(*args, us, False)
        step = loop._tangent_csr_stepwise(*args, us, True)
        assert len(kept[2]) == K and len(kept[3]) == K - 1 and pong[2] == [] and pong[3] == []
        assert _same(kept[:2], pong[:2]) and _same(kept[:2], step[:2])
        assert _same(kept[2], step[2]) and _same(kept[3], step[3])
    else:
        gates = ops.ista_forward(g, d["yp"], mask, d["tau"], A, B, True)[2]
        kept = ops.tangent_forward(g, vp, mask, A, B, gates, True)
        pong = ops.tangent_forward(g, vp, mask, A, B, gates, False, last=True)
        step = loop._tangent_generic_stepwise(g, vp, mask, A, B, gates, True)
        assert len(kept[1]) == K and len(kept[2]) == K - 1 and len(pong[1]) == 1 and pong[2] == []
        assert torch.equal(kept[0], pong[0]) and torch.equal(kept[1][-1], pong[1][0])
        assert torch.equal(kept[0], step[0]) and _same(kept[1], step[1]) and _same(kept[2], step[2])


@pytest.mark.parametrize("K", KS)
def test_fused_2d_tables(K):
    from cdlnet_video_amd import loop, ops
    d = _inputs("fused", K)
    g, yp, vp, mask, A, B, lay = d["g"], d["yp"], d["vp"], d["mask"], d["A"], d["B"], "blocked"
    kept = ops.fused_forward(g, yp, mask, d["tau"], A, B, True, "split3", lay)
    pong = ops.fused_forward(g, yp, mask, d["tau"], A, B, False, "split3", lay, keep_maps=True)
    assert len(kept[2]) == K and len(kept[3]) == K - 1 and len(pong[2]) == 1 and pong[3] == []
    assert _same(kept[:2], pong[:2]) and _same(kept[4], pong[4])
    with loop.precision_scope("split3"):
        step = loop._forward_fused_stepwise(g, yp, mask, d["tau"], A, B, True, True, layout=lay)
        assert _same(kept[:2], step[:2]) and _same(kept[3], step[3]) and _same(kept[4], step[4])
        maps = kept[4]
        tk = ops.fused_tangent(g, vp, mask, A, B, maps, True, "split3", lay)
        tp = ops.fused_tangent(g, vp, mask, A, B, maps, False, "split3", lay, last=True)
        ts = loop._tangent_fused_stepwise(g, vp, mask, A, B, maps, True, layout=lay, precision="split3")
    assert len(tk[1]) == K and len(tk[2]) == K - 1 and len(tp[1]) == 1 and tp[2] == []
    assert torch.equal(tk[0], tp[0]) and torch.equal(tk[1][-1], tp[1][0])
    assert torch.equal(tk[0], ts[0]) and torch.equal(tk[1][-1], ts[1][-1]) and _same(tk[2], ts[2])


@pytest.mark.parametrize("tier", ["tile", "strip"])
@pytest.mark.parametrize("K", KS)
def test_fused_generic_tables(K, tier):
    from cdlnet_video_amd import ops
    d = _inputs(tier, K)
    g, yp, vp, mask, A, B = d["g"], d["yp"], d["vp"], d["mask"], d["A"], d["B"]
    kept = ops.fusedg_forward(g, yp, mask, d["tau"], A, B, True)
    pong = ops.fusedg_forward(g, yp, mask, d["tau"], A, B, False, keep_maps=True)
    assert len(kept[2]) == K and len(kept[3]) == K - 1 and len(pong[2]) == 1 and pong[3] == []
    assert _same(kept[:2], pong[:2]) and _same(kept[4], pong[4])
    tk = ops.fusedg_tangent(g, vp, mask, A, B, kept[4], True)
    tp = ops.fusedg_tangent(g, vp, mask, A, B, kept[4], False, last=True)
    assert len(tk[1]) == K and len(tk[2]) == K - 1 and len(tp[1]) == 1 and tp[2] == []
    assert torch.equal(tk[0], tp[0]) and torch.equal(tk[1][-1], tp[1][0])
