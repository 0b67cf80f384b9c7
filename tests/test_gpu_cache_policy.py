"""Cache policy of the fused 2-D kernels' streams (cdl_fused2d.hip, struct CachePolicy).

A policy decides where a cache line is kept, never a value -- but a load that goes past a cache, or a store that writes
through one, could hand a consumer in the NEXT launch stale bytes, and a store form could stop dropping the lanes whose
offset lies beyond the descriptor.  So: producer -> consumer across a launch boundary on every stream that carries a policy
(the stages' fat loads and stores, k_wgrad2d's fat load), at the smallest shapes with partial tiles in both axes, more
than one tile per axis and both tile directions (the sweeps walk the tiles in snake order).

The tests hold under every policy and are meant to be run under the -DCDL_POL_* A/B builds as well.
"""
import pytest
import torch

from arena_util import Arena
from gpu_util import launch_sites

pytestmark = pytest.mark.gpu

N, K = 2, 3
SHAPES = [(20, 70, 5), (33, 65, 7)]          # (H, W, P): 64 x 16 tiles, partial in both axes, 2 x 2 and 2 x 3 of them


def _net(cva, M, P):
    torch.manual_seed(7)
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=1, t0=5e-3, adaptive=True, init=True)
    with torch.no_grad():                    # K identical iterations would hide a stage that read the wrong launch's bytes
        for n, p in net.named_parameters():
            if n == "t":
                p.uniform_(2e-3, 2e-2)
            elif n != "g":
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net.cuda()


def _data(cva, H, W):
    x = cva.utils.synthetic_clip((N, 1, H, W), seed=3)
    y, sigma = cva.awgn(x, (20, 30), torch.Generator().manual_seed(4))
    return x.cuda(), y.cuda(), sigma.cuda()


def _train_step(net, x, y, sigma):
    """One training step through the public net call; every output and every parameter gradient, cloned."""
    for p in net.parameters():
        p.grad = None
    xhat, z = net(y, sigma)
    torch.mean((x - xhat) ** 2).backward()
    torch.cuda.synchronize()
    out = {"xhat": xhat.detach().clone(), "z_K": z.detach().clone()}
    out.update({f"d{n}": p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    assert any(k.startswith("dA") for k in out) and any(k.startswith("dB") for k in out) and "dt" in out, sorted(out)
    return out


def _stepwise(monkeypatch, loop):
    """Route the fused tier's sweeps through the launch-by-launch drivers."""
    monkeypatch.setattr(loop, "_forward_fused", lambda g, yp, mask_p, tau, A, B, keep_codes, keep_resid, layout=None, *, keep_maps=False:
                        loop._forward_fused_stepwise(g, yp, mask_p, tau, A, B, keep_codes, keep_resid, layout=layout or loop.CODE_LAYOUT))
    monkeypatch.setattr(loop, "_backward_fused", lambda g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=None, layout=None,
                        precision=None, dyp=None, dtau=None:
                        loop._backward_fused_stepwise(g, K, yp, mask_p, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps,
                                                      layout=layout or loop.CODE_LAYOUT, dyp=dyp, dtau=dtau))


def _same(tag, a, b, keys=None):
    assert sorted(a) == sorted(b)
    bad = [k for k in (keys or a) if not torch.equal(a[k], b[k])]
    assert not bad, f"{tag}: not bit-identical: {bad}"


def _order_fixed(out):
    """What does not depend on how the filter gradients' partial sums are grouped: outputs and threshold gradients."""
    return [k for k in out if not (k.startswith("dA") or k.startswith("dB"))]


@pytest.mark.parametrize("layout", ["blocked", "nchw"])
@pytest.mark.parametrize("H,W,P", SHAPES)
@pytest.mark.parametrize("M", [32, 64])
def test_training_step_twice_equals_the_stepwise_drivers(M, H, W, P, layout, monkeypatch, hip_env):
    """Two training steps in a row through net(y, sigma) -- the second finds the code buffers, patches and partial
    workspace of the first still in cache -- against each other and against the step-wise drivers, bit for bit.

    The sweeps walk the tiles in snake order and compute dA_k inside the reverse stage; the step-wise drivers walk them
    forwards and compute dA_k in k_wgrad2d.  That regroups the filter gradients' partial sums (tests/test_gpu_fused.py:
    2e-6), so against the step-wise drivers the snake-order step is compared in everything else -- xhat, z_K, dt -- and the
    filter gradients in a step with CDL_FUSED_SNAKE=0 and CDL_FUSED_DA=0, which enqueues the step-wise launches exactly.
    """
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    monkeypatch.setattr(loop, "CODE_LAYOUT", layout)
    net = _net(cva, M, P)
    x, y, sigma = _data(cva, H, W)
    assert cva.ops.fused_supported(cva.ops.Geometry.make(N, 1, M, (H, W), (P, P), (P // 2, P // 2), 1))
    with cva.ops.trace() as t:
        first = _train_step(net, x, y, sigma)
    sites = sorted(launch_sites(t))
    assert all(any(s.startswith("cdl_fused2d.hip:" + k) for s in sites) for k in ("k_stage<", "k_wgrad2d<", "k_assemble")), sites
    second = _train_step(net, x, y, sigma)
    _same("second step vs first", first, second)
    hip_env("CDL_FUSED_SNAKE", "0")
    hip_env("CDL_FUSED_DA", "0")
    plain = [_train_step(net, x, y, sigma) for _ in range(2)]
    _same("forward-order step, second vs first", plain[0], plain[1])
    _stepwise(monkeypatch, loop)
    ref = _train_step(net, x, y, sigma)
    _same("forward-order step vs step-wise drivers", plain[1], ref)
    for tag, got in (("first", first), ("second", second)):
        _same(f"snake-order step ({tag}) vs step-wise drivers", got, ref, _order_fixed(ref))


@pytest.mark.parametrize("layout", ["blocked", "nchw"])
def test_training_step_inside_guard_bands(layout, monkeypatch):
    """The same step with every sweep buffer -- codes, du ping-pong, thin tensors, patches, partial banks -- carved out of
    a guard-banded arena: lanes outside the image carry an out-of-range offset and must be dropped
    under every store policy, so no guard word changes, and the results are those of ordinary allocations bit for bit."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    o = cva.ops
    M, (H, W, P) = 64, SHAPES[1]
    monkeypatch.setattr(loop, "CODE_LAYOUT", layout)
    net = _net(cva, M, P)
    x, y, sigma = _data(cva, H, W)
    ref = _train_step(net, x, y, sigma)
    arena = Arena("cuda")
    code_buffer, wgrad_ws = o.fused_code_buffer, o.fused_wgrad_workspace

    def like(t, name):                       # offset 0: library-sized buffers are 16-byte aligned (include/cdlnet_hip.h)
        return arena.out(t.shape, 0, name=f"{name}{len(arena.bufs)}")

    monkeypatch.setattr(o, "_new", lambda shape, device: arena.out(shape, 0, name=f"new{len(arena.bufs)}"))
    monkeypatch.setattr(o, "_thin", lambda g, device, count: arena.out((count,) + g.image_shape(), 0, name=f"thin{len(arena.bufs)}"))
    monkeypatch.setattr(o, "_FUSED2D", o._FUSED2D._replace(
        code_buffers=lambda g, lay, device, count=1: like(code_buffer(g, lay, device, count), "codes"),
        reverse_ws=lambda g, device: (like(wgrad_ws(g, device), "wgrad_ws"),)))
    for _ in range(2):
        got = _train_step(net, x, y, sigma)
        arena.check()
        _same("step inside guard bands vs ordinary allocations", got, ref)
    assert len(arena.bufs) >= 2 * 8, [b.name for b in arena.bufs]
