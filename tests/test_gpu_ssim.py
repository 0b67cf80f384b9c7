"""cva.metrics on the device (cdl_ssim_fwd / cdl_ssim_bwd) against the float64 restatement (tests/ssim_restate.py).

Every gate is max(1e-6, 2 x the error the same restatement makes in fp32), measured per comparison: the E[x^2] -
E[x]^2 cancellation sets what fp32 can do, so no fixed fp32 number is guessed."""
import pytest
import torch

import ssim_restate as R
from gpu_util import check, log

pytestmark = pytest.mark.gpu


def _cva():
    import cdlnet_video_amd as cva
    return cva


def _images(shape, seed, scale=1.0, noise=0.1):
    cva = _cva()
    x = cva.utils.synthetic_clip(shape, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    y = x + noise * torch.randn(x.shape, generator=g)
    return x * scale, y * scale


def _gate(name, got, ref64, ref32):
    tol = max(1e-6, 2 * R_err(ref32, ref64))
    return check(name, got.double(), ref64, tol)


def R_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


SHAPES_4D = [((1, 1, 11, 11), 11), ((2, 3, 37, 53), 11), ((3, 1, 71, 130), 7), ((64, 1, 256, 256), 11),
             ((2, 1, 45, 33), 15), ((2, 2, 20, 24), 3)]


@pytest.mark.parametrize("shape,win", SHAPES_4D)
def test_ssim_values(shape, win):
    cva = _cva()
    x, y = _images(shape, seed=sum(shape) + win)
    got = cva.metrics.ssim(x.cuda(), y.cuda(), data_range=1.0, win_size=win, size_average=False)
    r64 = R.ssim(x.double(), y.double(), data_range=1.0, win_size=win, size_average=False)
    r32 = R.ssim(x, y, data_range=1.0, win_size=win, size_average=False)
    _gate(f"ssim per image {shape} win {win}", got.cpu(), r64, r32)
    # per channel (P = N * C planes): through the autograd entry's own output shape
    pc = cva.metrics._plane_ssim(x.cuda(), y.cuda(), torch.ones(shape[0] * shape[1], device="cuda"),
                                 cva.metrics._gaussian_window(win, 1.5), 0.01, 0.03, 1.0)
    _gate(f"ssim per channel {shape} win {win}", pc.cpu(), R.ssim_per_channel(x.double(), y.double(), 1.0, win),
          R.ssim_per_channel(x, y, 1.0, win))


def test_ssim_range_255_and_nonnegative():
    cva = _cva()
    x, y = _images((4, 3, 64, 96), seed=3, scale=255.0, noise=0.3)
    got = cva.metrics.ssim(x.cuda(), y.cuda())
    _gate("ssim data_range 255 (cancellation case)", got.cpu().reshape(1), R.ssim(x.double(), y.double()).reshape(1),
          R.ssim(x, y).reshape(1))
    got_n = cva.metrics.ssim(x.cuda(), -y.cuda(), nonnegative_ssim=True, size_average=False)
    ref_n = R.ssim(x.double(), -y.double(), nonnegative_ssim=True, size_average=False)
    assert (ref_n >= 0).all()
    _gate("ssim nonnegative", got_n.cpu() + 1, ref_n + 1, R.ssim(x, -y, nonnegative_ssim=True, size_average=False) + 1)


@pytest.mark.parametrize("shape,win", [((1, 1, 7, 7), 7), ((2, 3, 37, 53), 7), ((5, 1, 128, 128), 7),
                                       ((2, 2, 40, 31), 11), ((64, 1, 256, 256), 7)])
def test_structural_similarity_values(shape, win):
    cva = _cva()
    x, y = _images(shape, seed=7 + win)
    got = cva.metrics.structural_similarity(x.cuda(), y.cuda(), win_size=win)
    r64 = R.structural_similarity(x.double(), y.double(), win_size=win)
    r32 = R.structural_similarity(x, y, win_size=win)
    assert got.shape == shape[:2]
    _gate(f"structural_similarity {shape} win {win}", got.cpu(), r64, r32)
    if shape[1] == 3:
        col = cva.metrics.structural_similarity(x.cuda(), y.cuda(), win_size=win, channel_axis=1)
        _gate(f"structural_similarity colour {shape}", col.cpu(), r64.mean(1), r32.mean(1))


def _grads_64(fn, *args):
    args = [a.detach().double().requires_grad_() for a in args]
    fn(*args).backward()
    return [a.grad for a in args]


def _grads_32(fn, *args):
    args = [a.detach().float().requires_grad_() for a in args]
    fn(*args).backward()
    return [a.grad for a in args]


@pytest.mark.parametrize("shape,win", [((1, 1, 11, 11), 11), ((2, 3, 37, 53), 11), ((64, 1, 256, 256), 11),
                                       ((2, 1, 45, 33), 15), ((3, 2, 29, 70), 5)])
def test_ssim_gradients(shape, win):
    cva = _cva()
    x, y = _images(shape, seed=11 + win)
    w = torch.rand(shape[0], generator=torch.Generator().manual_seed(5)) + 0.5     # upstream per image
    rng = torch.tensor(1.2)

    def ref(a, b, r):
        return (R.ssim(a, b, data_range=r, win_size=win, size_average=False) * w.to(a.dtype)).sum()

    g64 = _grads_64(ref, x, y, rng)
    g32 = _grads_32(ref, x, y, rng)
    xd, yd, rd = (t.cuda().requires_grad_() for t in (x, y, rng))
    out = cva.metrics.ssim(xd, yd, data_range=rd, win_size=win, size_average=False)
    (out * w.cuda()).sum().backward()
    for name, got, a, b in zip(("dx", "dy", "dR"), (xd.grad, yd.grad, rd.grad), g64, g32):
        _gate(f"ssim {name} {shape} win {win}", got.cpu().reshape(a.shape), a, b)


def test_ssim_gradient_one_side():
    """Only X requires grad: dy is not computed and nothing else changes."""
    cva = _cva()
    x, y = _images((2, 1, 40, 50), seed=4)
    xa = x.cuda().requires_grad_()
    cva.metrics.ssim(xa, y.cuda(), data_range=1.0).backward()
    yb = y.cuda().requires_grad_()
    xb = x.cuda().requires_grad_()
    cva.metrics.ssim(xb, yb, data_range=1.0).backward()
    assert torch.equal(xa.grad, xb.grad)


@pytest.mark.parametrize("shape", [(2, 1, 8, 128, 128), (1, 3, 4, 37, 53)])
def test_ssim_frames_value_and_gradients(shape):
    cva = _cva()
    o, t = _images(shape, seed=21)
    r64 = R.ssim_frames(o.double(), t.double())
    r32 = R.ssim_frames(o, t)
    g64 = _grads_64(R.ssim_frames, o, t)
    g32 = _grads_32(R.ssim_frames, o, t)
    od, td = o.cuda().requires_grad_(), t.cuda().requires_grad_()
    loss = cva.metrics.ssim_frames(od, td)
    loss.backward()
    _gate(f"ssim_frames value {shape}", loss.detach().cpu().reshape(1), r64.reshape(1), r32.reshape(1))
    _gate(f"ssim_frames d output {shape}", od.grad.cpu(), g64[0], g32[0])
    _gate(f"ssim_frames d target {shape}", td.grad.cpu(), g64[1], g32[1])
    # the data_range path matters: the max / min elements of every frame carry a gradient the map alone does not give
    flat = o.transpose(0, 2).reshape(shape[2], -1)
    imax = flat.argmax(1)
    g_no_r = _grads_64(lambda a, b: sum(1 - R.ssim(a[:, :, k], b[:, :, k],
                                                  data_range=float(a[:, :, k].max() - a[:, :, k].min()))
                                        for k in range(shape[2])) / shape[2], o, t)[0]
    dg = (g64[0] - g_no_r).transpose(0, 2).reshape(shape[2], -1)
    assert (dg.gather(1, imax[:, None]).abs() > 0).all()


def test_determinism():
    cva = _cva()
    o, t = _images((2, 1, 8, 128, 128), seed=5)
    runs = []
    for _ in range(2):
        od = o.cuda().requires_grad_()
        v = cva.metrics.ssim_frames(od, t.cuda())
        v.backward()
        s = cva.metrics.structural_similarity(o.cuda(), t.cuda())
        runs.append((v.detach(), od.grad, s))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_ssim_frames_no_host_sync():
    cva = _cva()
    o, t = _images((2, 1, 8, 64, 64), seed=6)
    od, td = o.cuda().requires_grad_(), t.cuda()
    cva.metrics.ssim_frames(od, td).backward()          # first call: library load, scratch allocation
    od.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                # the hook is live: a device-to-host read is refused
            torch.ones(1, device="cuda").item()
        loss = cva.metrics.ssim_frames(od, td)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert od.grad is not None and torch.isfinite(od.grad).all()


def test_end_to_end_training_step():
    cva = _cva()
    torch.manual_seed(3)
    net = cva.CDLNetVideo(K=3, M=16, P=[3, 5, 5], s=1, C=1, t0=5e-3, adaptive=True, depth=4, init=True)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda()
    x = cva.utils.synthetic_clip((2, 1, 4, 40, 48), seed=8)
    y = x + torch.randn(x.shape, generator=torch.Generator().manual_seed(9)) * 25 / 255
    xd, yd = x.cuda(), y.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    xhat, _ = net(yd, 25.0)
    loss = torch.mean((xhat - xd) ** 2) + 0.1 * cva.metrics.ssim_frames(xhat, xd)
    opt.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}

    # the same net and data, with the SSIM term's dL/dxhat from float64 autograd of the restatement
    ref = cva.CDLNetVideo(K=3, M=16, P=[3, 5, 5], s=1, C=1, t0=5e-3, adaptive=True, depth=4, init=False)
    ref.load_state_dict(sd)
    ref = ref.cuda()
    xr, _ = ref(yd, 25.0)
    assert torch.equal(xr.detach(), xhat.detach())
    G = _grads_64(lambda a: 0.1 * R.ssim_frames(a, x.double()), xhat.detach().cpu())[0]
    (torch.mean((xr - xd) ** 2) + (xr * G.float().cuda()).sum()).backward()
    for n, p in ref.named_parameters():
        check(f"end-to-end MSE + 0.1 ssim_frames grad {n}", grads[n], p.grad, 1e-4)
    opt.step()
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_video_ssim():
    cva = _cva()
    torch.manual_seed(4)
    net = cva.CDLNetVideo(K=3, M=16, P=[3, 5, 5], s=1, C=1, t0=5e-3, adaptive=True, depth=4, init=True).cuda()
    x = cva.utils.synthetic_clip((2, 1, 8, 64, 64), seed=10)
    y = x + torch.randn(x.shape, generator=torch.Generator().manual_seed(11)) * 25 / 255
    with torch.no_grad():
        den, _ = net(y.cuda(), 25.0)
    got = cva.metrics.video_ssim(x.cuda(), den)
    d = den.cpu()
    frames64 = [float(R.structural_similarity(d[b, 0, k].double(), x[b, 0, k].double()))
                for b in range(2) for k in range(8)]
    frames32 = [float(R.structural_similarity(d[b, 0, k], x[b, 0, k])) for b in range(2) for k in range(8)]
    ref64, ref32 = sum(frames64) / 16, sum(frames32) / 16
    tol = max(1e-6, 2 * abs(ref32 - ref64))
    log(f"{'video_ssim':60s} abs_err={abs(got - ref64):.3e} tol={tol:.1e} value={got:.6f}")
    assert isinstance(got, float) and abs(got - ref64) < tol
    # colour frames: the mean over channels, as skimage's channel_axis
    xc, yc = _images((1, 3, 2, 40, 40), seed=12)
    gc = cva.metrics.video_ssim(xc.cuda(), yc.cuda())
    rc = sum(float(R.structural_similarity(yc[0, :, k].double(), xc[0, :, k].double()).mean()) for k in range(2)) / 2
    assert abs(gc - rc) < 1e-5


@pytest.mark.parametrize("kind", ["0-d", "per frame"])
def test_ssim_frames_tensor_data_range(kind):
    """A tensor data_range (the natural port of loss.py's `out.max() - out.min()`), requiring grad: one value shared
    by every (n, c, d) plane must reach each of them, in value and in dL/dR."""
    cva = _cva()
    shape = (2, 1, 8, 64, 64)
    o, t = _images(shape, seed=31)
    r = torch.tensor(1.1) if kind == "0-d" else torch.linspace(0.8, 1.5, shape[2])

    def ref(a, b, rr):
        if rr.dim() == 0:
            return R.ssim_frames(a, b, data_range=rr)
        return sum(1 - R.ssim(a[:, :, k], b[:, :, k], data_range=rr[k]) for k in range(shape[2])) / shape[2]

    r64 = ref(o.double(), t.double(), r.double())
    r32 = ref(o, t, r)
    g64 = _grads_64(ref, o, t, r)
    g32 = _grads_32(ref, o, t, r)
    od, rd = o.cuda().requires_grad_(), r.cuda().requires_grad_()
    loss = cva.metrics.ssim_frames(od, t.cuda(), data_range=rd)
    loss.backward()
    _gate(f"ssim_frames tensor data_range ({kind}) value", loss.detach().cpu().reshape(1), r64.reshape(1),
          r32.reshape(1))
    _gate(f"ssim_frames tensor data_range ({kind}) d output", od.grad.cpu(), g64[0], g32[0])
    _gate(f"ssim_frames tensor data_range ({kind}) dR", rd.grad.cpu().reshape(g64[2].shape), g64[2], g32[2])


def test_cs_output_of_the_abi():
    """cdl_ssim_fwd's optional per-plane cs mean (no Python caller uses it) against the restatement."""
    cva = _cva()
    m = cva.metrics
    ops = cva.ops
    x, y = _images((3, 2, 45, 70), seed=41)
    P, H, W = 6, 45, 70
    win = m._gaussian_window(11, 1.5)
    xd, yd = x.cuda().reshape(P, H, W).contiguous(), y.cuda().reshape(P, H, W).contiguous()
    rng = torch.full((P,), 1.0, device="cuda")
    s_out = torch.empty(P, device="cuda")
    cs_out = torch.empty(P, device="cuda")
    lib = cva._lib.lib()
    n = int(lib.cdl_ssim_scratch_floats(P, H, W, 11))
    scratch = torch.empty(n, device="cuda")
    rc = lib.cdl_ssim_fwd(ops._ptr(xd), ops._ptr(yd), P, H, W, m._window_arg(win), 11, 0.01, 0.03, 1.0,
                          ops._ptr(rng), ops._ptr(s_out), ops._ptr(cs_out), ops._ptr(scratch), n, ops._stream())
    cva._lib.check(rc, "cdl_ssim_fwd")
    s64, cs64 = R.ssim_cs_per_channel(x.double(), y.double(), 1.0)
    s32, cs32 = R.ssim_cs_per_channel(x, y, 1.0)
    _gate("abi ssim mean (with cs)", s_out.cpu().reshape(3, 2), s64, s32)
    _gate("abi cs mean", cs_out.cpu().reshape(3, 2), cs64, cs32)


@pytest.mark.parametrize("which", ["y", "R"])
def test_ssim_gradient_single_output(which):
    """dy alone (dx = NULL) and dL/dR alone (dx = dy = NULL) through cdl_ssim_bwd, against the restatement."""
    cva = _cva()
    shape = (2, 3, 37, 53)
    x, y = _images(shape, seed=51)
    rng = torch.tensor(1.3)
    idx = {"y": 1, "R": 2}[which]

    def ref(a, b, r):
        return R.ssim(a, b, data_range=r)

    args64 = [x.double(), y.double(), rng.double()]
    args32 = [x, y, rng]
    for args in (args64, args32):
        args[idx] = args[idx].clone().requires_grad_()
        ref(*args).backward()
    dev = [x.cuda(), y.cuda(), rng.cuda()]
    dev[idx] = dev[idx].clone().requires_grad_()
    cva.metrics.ssim(dev[0], dev[1], data_range=dev[2]).backward()
    _gate(f"ssim d{which} alone", dev[idx].grad.cpu(), args64[idx].grad, args32[idx].grad)
