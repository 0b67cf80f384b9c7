"""The perceptual term on the device (cdl_vgg_forward / cdl_vgg_backward) against the float64 restatement
(tests/perceptual_restate.py), CombinedLossWithSSIM as a whole, and the trainer with `loss_fn` / `combmse`.

Gates: max(floor, 2 x the error the same restatement makes in fp32).  The floor is the dense tier's: its operands are
split-bf16 pairs (16-17 significant bits), 5e-5 after the six dense layers for features and
values, 1e-4 for gradients; the measured values are logged.  Against the restatement's own ReLU gates a gradient can
differ where a pre-activation sits within rounding of 0 (a gate flips); the comparison with the product's own gates
and argmax codes, where the map is linear, is the exact one."""
import math

import pytest
import torch

import perceptual_restate as R
from gpu_util import check, log
from vgg_scratch_util import scratch_views as _scratch_views

pytestmark = pytest.mark.gpu

FLOOR_F, FLOOR_G = 5e-5, 1e-4


def _cva():
    import cdlnet_video_amd as cva
    return cva


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _gate(name, got, r64, r32, floor):
    return check(name, got.double(), r64, max(floor, 2 * _err(r32, r64)))


def _clips(shape, seed):
    cva = _cva()
    x = cva.utils.synthetic_clip(shape, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    y = (x + 0.1 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    return y, x                                     # (output, target)


SHAPES = [(1, 1, 2, 128, 128), (1, 1, 3, 37, 50), (2, 1, 15, 32, 40)]


@pytest.mark.parametrize("shape", SHAPES)
def test_features_match_restatement(shape):
    cva = _cva()
    sd = R.random_weights(shape[-1])
    o, _ = _clips(shape, seed=sum(shape))
    P = shape[0] * shape[2]
    planes = o.reshape(P, 1, *shape[-2:])
    got = cva.metrics.vgg16_features(o.cuda().reshape(P, *shape[-2:]), sd)
    r64 = R.features(planes.double(), {k: v.double() for k, v in sd.items()})
    r32 = R.features(planes, sd)
    assert got.shape == r64.shape
    _gate(f"relu3_3 {shape}", got.cpu(), r64, r32, FLOOR_F)


@pytest.mark.parametrize("shape", SHAPES)
def test_value_and_gradients(shape):
    cva = _cva()
    sd = R.random_weights(shape[-2])
    o, t = _clips(shape, seed=sum(shape) + 7)
    oc, tc = o.cuda().requires_grad_(), t.cuda().requires_grad_()
    val = cva.metrics.perceptual_frames(oc, tc, sd)
    val.backward(torch.tensor(0.7, device="cuda"))
    sd64 = {k: v.double() for k, v in sd.items()}
    o64, t64 = o.double().requires_grad_(), t.double().requires_grad_()
    r64 = R.perceptual(o64, t64, sd64)
    (0.7 * r64).backward()
    o32, t32 = o.clone().requires_grad_(), t.clone().requires_grad_()
    r32 = R.perceptual(o32, t32, sd)
    (0.7 * r32).backward()
    _gate(f"perceptual value {shape}", val.detach().cpu().reshape(1), r64.detach().reshape(1),
          r32.detach().reshape(1), FLOOR_F)
    # the restatement's own gates and argmaxes: a ReLU gate or a near-tied pool window that rounds the other way moves
    # a few elements by a whole contribution (smooth frames have many near-tied windows), so the max-norm error is
    # logged and the l2 error is gated; test_gradients_with_product_gates is the exact comparison
    e_dx, e_dy = _err(oc.grad, o64.grad), _err(tc.grad, t64.grad)
    l_dx, l_dy = _l2(oc.grad, o64.grad), _l2(tc.grad, t64.grad)
    log(f"perceptual dx / dy {shape} vs free restatement: max {e_dx:.3e} / {e_dy:.3e}, l2 {l_dx:.3e} / {l_dy:.3e}")
    assert l_dx < 5e-2 and l_dy < 5e-2


def _gates_of(v, f):
    """Restatement gates / argmax codes from the kept activations: a pooled layer's gate is its pooled value's
    (only the argmax position is gathered)."""
    up2 = lambda p, like: torch.nn.functional.pad(                              # noqa: E731
        p.repeat_interleave(2, -2).repeat_interleave(2, -1),
        (0, like[-1] - 2 * p.shape[-1], 0, like[-2] - 2 * p.shape[-2]))
    a1 = v["a1"]
    gates = [a1 > 0, up2(v["p1"] > 0, a1.shape), v["a3"] > 0, up2(v["p2"] > 0, v["a3"].shape), v["a5"] > 0,
             v["a6"] > 0, f > 0]
    return [g.double().cpu() for g in gates], [v["am1"].long().cpu(), v["am2"].long().cpu()]


@pytest.mark.parametrize("shape", [(1, 1, 2, 64, 64), (1, 1, 3, 37, 50)])
def test_gradients_with_product_gates(shape):
    cva = _cva()
    lib = cva._lib.lib()
    ops = cva.ops
    sd = R.random_weights(11)
    o, t = _clips(shape, seed=3)
    P, (H, W) = shape[0] * shape[2], shape[-2:]
    x, y = o.cuda().reshape(P, H, W).contiguous(), t.cuda().reshape(P, H, W).contiguous()
    ws, bs = cva.metrics._vgg_tables(sd, x.device)
    n = int(lib.cdl_vgg_scratch_floats(P, H, W, 3))
    scr = torch.zeros(n, device="cuda")
    loss = torch.empty((), device="cuda")
    wt, bt = ops._ptr_table(ws), ops._ptr_table(bs)
    cva._lib.check(lib.cdl_vgg_forward(ops._ptr(x), ops._ptr(y), P, H, W, wt, bt, 3, None, ops._ptr(loss),
                                       ops._ptr(scr), n, ops._stream()), "cdl_vgg_forward")
    s0, s1, fy = _scratch_views(scr, P, H, W, 3)
    fx = cva.metrics.vgg16_features(x, sd)                    # conv3_3's ReLU gate of the output (same kernels)
    gx, cx = _gates_of(s0, fx)
    gy, cy = _gates_of(s1, fy)
    g1 = torch.ones((), device="cuda")
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    cva._lib.check(lib.cdl_vgg_backward(P, H, W, wt, bt, 3, ops._ptr(g1), ops._ptr(dx), ops._ptr(dy), ops._ptr(scr),
                                        n, ops._stream()), "cdl_vgg_backward")

    def restated(dt):
        sdd = {k: v.to(dt) for k, v in sd.items()}
        a = o.reshape(P, 1, H, W).to(dt).requires_grad_()
        b = t.reshape(P, 1, H, W).to(dt).requires_grad_()
        fa = R.features(a, sdd, gates=gx, codes=cx)
        fb = R.features(b, sdd, gates=gy, codes=cy)
        val = torch.mean((fa - fb) ** 2)
        val.backward()
        return val.detach(), a.grad.reshape(P, H, W), b.grad.reshape(P, H, W)

    v64, dx64, dy64 = restated(torch.float64)
    v32, dx32, dy32 = restated(torch.float32)
    _gate(f"perceptual value, product gates {shape}", loss.cpu().reshape(1), v64.reshape(1), v32.reshape(1), FLOOR_F)
    _gate(f"perceptual dx, product gates {shape}", dx.cpu(), dx64, dx32, FLOOR_G)
    _gate(f"perceptual dy, product gates {shape}", dy.cpu(), dy64, dy32, FLOOR_G)


def _first_max_codes(h, rel=1e-9):
    """argmax codes of the 2x2 windows of h (P, C, H, W) by the first-maximum rule, values within rel of the maximum
    counted as ties (the float64 restatement may round tied positions differently); also the number of tied windows
    at positive values."""
    P, C, H, W = h.shape
    Hp, Wp = H // 2, W // 2
    v = h[..., :2 * Hp, :2 * Wp].reshape(P, C, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(P, C, Hp, Wp, 4)
    m = v.max(-1, keepdim=True).values
    ok = v >= m - rel * m.abs()
    ties = int(((ok.sum(-1) > 1) & (m.squeeze(-1) > 0)).sum())
    return ok.to(torch.int8).argmax(-1), ties


def test_pool_ties_go_to_the_first_maximum():
    """A piecewise-constant image (constant 32 x 32 blocks): interior pool windows tie exactly at positive values, so
    the gradient of every tied window must reach its first (row-major) element only."""
    cva = _cva()
    sd = R.random_weights(12)
    for k in list(sd):                               # positive biases: the ties sit at positive values
        if k.endswith("bias"):
            sd[k] = sd[k].abs() + 0.05
    g = torch.Generator().manual_seed(13)
    blocks = torch.rand((1, 1, 2, 2, 2), generator=g)
    o = blocks.repeat_interleave(32, -2).repeat_interleave(32, -1)        # (1, 1, 2, 64, 64)
    t = torch.zeros_like(o)
    oc = o.cuda().requires_grad_()
    cva.metrics.perceptual_frames(oc, t.cuda(), sd).backward()
    sd64 = {k: v.double() for k, v in sd.items()}
    planes = o.reshape(2, 1, 64, 64).double()
    trace = []
    R.features(planes, sd64, trace=trace)
    pre = [tr for tr in trace if tr.dtype == torch.float64]
    c1, n1 = _first_max_codes(torch.relu(pre[1]))
    c2, n2 = _first_max_codes(torch.relu(pre[3]))
    log(f"tied pool windows at positive values: {n1} (pool 1), {n2} (pool 2)")
    assert n1 > 0 and n2 > 0
    gates = [(p_ > 0).double() for p_ in pre]
    a = planes.clone().requires_grad_()
    fa = R.features(a, sd64, gates=gates, codes=[c1, c2])
    torch.mean(fa ** 2).backward()                   # target features are zero-input features: constant
    fz = R.features(torch.zeros_like(planes), sd64)
    a2 = planes.clone().requires_grad_()
    torch.mean((R.features(a2, sd64, gates=gates, codes=[c1, c2]) - fz) ** 2).backward()
    _gate("perceptual dx, tied pool windows", oc.grad.cpu().reshape(2, 1, 64, 64), a2.grad,
          a2.grad.float().double(), FLOOR_G)


def test_repeatable_and_no_host_sync():
    cva = _cva()
    sd = R.random_weights(14)
    o, t = _clips((1, 1, 4, 48, 40), seed=15)
    w = {k: v.cuda() for k, v in sd.items()}
    runs = []
    for _ in range(2):
        oc, tc = o.cuda().requires_grad_(), t.cuda().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            val = cva.metrics.perceptual_frames(oc, tc, w)
            val.backward()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        runs.append((val.detach().cpu(), oc.grad.cpu(), tc.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_combined_loss_value_and_gradient():
    cva = _cva()
    sd = R.random_weights(16)
    o, t = _clips((2, 1, 3, 40, 44), seed=17)
    loss = cva.CombinedLossWithSSIM(1.0, 0.01, 0.1, vgg_weights={f"features.{k}": v for k, v in sd.items()}).cuda()
    assert all(b.is_cuda for b in loss.buffers())
    oc = o.cuda().requires_grad_()
    val = loss(oc, t.cuda())
    val.backward()
    o64 = o.double().requires_grad_()
    r64 = R.combined(o64, t.double(), {k: v.double() for k, v in sd.items()})
    r64.backward()
    o32 = o.clone().requires_grad_()
    r32 = R.combined(o32, t, sd)
    r32.backward()
    _gate("CombinedLossWithSSIM value", val.detach().cpu().reshape(1), r64.detach().reshape(1),
          r32.detach().reshape(1), FLOOR_F)
    e = _err(oc.grad, o64.grad)
    log(f"CombinedLossWithSSIM d/doutput vs restatement: {e:.3e}")
    assert e < max(1e-3, 2 * _err(o32.grad, o64.grad))


def _video_net(seed):
    cva = _cva()
    torch.manual_seed(seed)
    net = cva.CDLNetVideo(K=3, M=16, P=[3, 5, 5], s=1, C=1, t0=5e-3, adaptive=True, depth=6, init=True)
    return net.cuda()


def test_train_step_with_combined_loss():
    cva = _cva()
    sd = R.random_weights(18)
    batch = cva.utils.synthetic_clip((1, 1, 6, 40, 40), seed=19).cuda()
    loss_fn = cva.CombinedLossWithSSIM(1.0, 0.01, 0.1, vgg_weights=sd).cuda()
    net = _video_net(20)
    ref = _video_net(20)
    ref.load_state_dict(net.state_dict())
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    gen = torch.Generator().manual_seed(21)
    loss, sigma = cva.train_step(net, opt, batch, 25, generator=gen, loss_fn=loss_fn, project=False)
    # the same net's backward driven by the restated loss's gradient with respect to its output
    noisy, sigma2 = cva.awgn(batch, 25, torch.Generator().manual_seed(21))
    xhat, _ = ref(noisy, sigma2)
    xd = xhat.detach().cpu().double().requires_grad_()
    rl = R.combined(xd, batch.cpu().double(), {k: v.double() for k, v in sd.items()})
    rl.backward()
    xhat.backward(xd.grad.float().cuda())
    assert abs(float(loss) - float(rl)) <= 1e-4 * abs(float(rl))
    for (n_, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        check(f"train_step grad {n_}", p.grad, q.grad, 2e-3)


def test_default_arguments_unchanged(tmp_path):
    cva = _cva()
    batch = cva.utils.synthetic_clip((1, 1, 6, 32, 32), seed=22).cuda()
    out = []
    for kw in ({}, {"loss_fn": None}):
        net = _video_net(23)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        loss, _ = cva.train_step(net, opt, batch, 25, generator=torch.Generator().manual_seed(24), **kw)
        out.append((loss.cpu(), [p.detach().cpu().clone() for p in net.parameters()]))
    assert torch.equal(out[0][0], out[1][0]) and all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    hist = []
    for i, kw in enumerate(({}, {"combmse": False, "loss_fn": None})):
        net = _video_net(25)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        lines = []
        h = cva.fit(net, opt, {"train": [batch], "val": [batch]}, epochs=1, device=torch.device("cuda"),
                    save_dir=str(tmp_path / str(i)), generator=torch.Generator().manual_seed(26), log=lines.append,
                    **kw)
        hist.append((h, lines, [p.detach().cpu().clone() for p in net.parameters()]))
    assert hist[0][0] == hist[1][0] and hist[0][1][1:] == hist[1][1][1:]
    assert all(torch.equal(a, b) for a, b in zip(hist[0][2], hist[1][2]))


def test_fit_trains_with_combmse(tmp_path):
    cva = _cva()
    sd = R.random_weights(27)
    batch = cva.utils.synthetic_clip((1, 1, 6, 32, 32), seed=28).cuda()
    net = _video_net(29)
    before = [p.detach().clone() for p in net.parameters()]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    loss_fn = cva.CombinedLossWithSSIM(vgg_weights=sd).cuda()
    h = cva.fit(net, opt, {"train": [batch, batch]}, epochs=1, device=torch.device("cuda"), save_dir=str(tmp_path),
                generator=torch.Generator().manual_seed(30), combmse=True, loss_fn=loss_fn, log=lambda s: None)
    assert h and h[0][1] == "train" and math.isfinite(h[0][2])
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
