"""The public calls on VIEWS: inputs carved out of a poisoned arena at element offsets 1 and 2 (4- and 8-byte aligned
bases, NaN on both sides; tests/arena_util.py), compared with the same call on `.clone()`d inputs.

The result of the call on views must equal the clones' BIT FOR BIT, whether or not the launch trace is the same: every
form a launcher falls to on a misaligned pointer (the scalar assembles, k_wgm's element loads, k_dense_wgrad<false>,
the one-element ReLU) adds the same terms in the same order as its 16-byte form.  The clones' run
is the one tests/test_gpu_nets.py, test_gpu_fused.py, test_gpu_csr*.py hold to the oracle, so equality with it carries
those bounds over to views without a second, looser comparison.  Whether a case ran other launches on views, and which,
is written to the parity log (gpu_util.log).  After each call no guard word of any input may have changed."""
import pytest
import torch

from arena_util import Arena
from gpu_util import log

pytestmark = pytest.mark.gpu


def cva():
    import cdlnet_video_amd
    return cdlnet_video_amd


def detie(net, seed):
    """De-tie the K identical copies of the filters and thresholds (exact ties make the ST support ill-conditioned)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n in ("t", "t2"):
                p.copy_(torch.rand(p.shape, generator=gen) * 1.8e-2 + 2e-3)
            elif n not in ("g", "g1", "g2"):
                p.add_(0.05 * p.abs().mean() * torch.randn(p.shape, generator=gen))
    return net.cuda()


def views_vs_clones(tag, call, inputs, off):
    """call(**tensors) -> {name: tensor}: once on clones (fresh, aligned allocations), once on arena views at `off`."""
    o = cva().ops
    arena = Arena("cuda")
    views = {k: (None if v is None else arena.put(v, off, k)) for k, v in inputs.items()}
    for v in views.values():
        assert v is None or v.data_ptr() % 16 == (4 * off) % 16
    with o.trace() as t0:
        ref = call(**{k: (None if v is None else v.clone()) for k, v in views.items()})
        torch.cuda.synchronize()
    with o.trace() as t1:
        got = call(**views)
        torch.cuda.synchronize()
    arena.check()
    for k, v in inputs.items():                                  # the inputs themselves are read-only
        assert v is None or torch.equal(views[k].cpu(), v), f"{tag}: input {k} was written"
    return compare(f"{tag} off{off}", t0, t1, ref, got)


def compare(tag, t0, t1, ref, got):
    """Bit equality of two runs; returns whether their launch traces are the same, and logs the sites that differ."""
    sig = lambda t: [(r.file, r.line, r.func, r.note) for r in t]
    same = sig(t0) == sig(t1)
    only1 = sorted({f"{r.file}:{r.line} {r.note}" for r in t1} - {f"{r.file}:{r.line} {r.note}" for r in t0})
    log(f"arena nets {tag:48s} same launches on views: {same}" + ("" if same else f"; only on views: {only1}"))
    assert set(got) == set(ref)
    for k in got:
        assert not bool(torch.isnan(got[k]).any()), f"{tag} {k}: NaN (a guard word was read and used)"
        assert torch.equal(got[k], ref[k]), f"{tag} {k}: other bits on views than on clones (same launches: {same})"
    return same


def fwd_bwd(net, target, with_mask=False):
    def call(y, sigma, mask=None):
        net.zero_grad(set_to_none=True)
        y = y.detach().requires_grad_()
        xhat, z = net(y, sigma, mask=mask) if with_mask else net(y, sigma)
        (torch.mean((target - xhat) ** 2) + 1e-3 * z.abs().mean()).backward()
        out = {"xhat": xhat.detach(), "z": z.detach(), "grad y": y.grad}
        out.update({f"grad {n}": p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
        return out
    return call


def sigma_for(kind, N, grid, gen):
    if kind == "map":
        return 15.0 + 20.0 * torch.rand((N, 1) + tuple(grid), generator=gen)
    return 15.0 + 20.0 * torch.rand(N + 1, generator=gen)[:N].contiguous()       # one level per sample


NETS = {
    # the fused 2-D tier, the JDD net (C = 3 + Bayer mask) and the video net on the tile kernel, at smoke() / fixture sizes
    "cdlnet-fused2d": (lambda c: c.CDLNet(K=4, M=32, P=7, s=1, C=1, t0=5e-3, adaptive=True, init=True), (2, 1, 48, 40), False),
    "jdd": (lambda c: c.CDLNet(K=3, M=64, P=7, s=1, C=3, t0=5e-3, adaptive=True, init=True), (1, 3, 32, 72), True),
    "video": (lambda c: c.CDLNetVideo(K=3, M=16, P=[3, 5, 5], s=1, C=1, t0=5e-3, adaptive=True, depth=6, init=True),
              (1, 1, 6, 24, 40), False),
    # N = 1, M = 169, P = 7: the per-iteration code and filter-gradient views of the sweep itself are misaligned
    "s2030-arch": (lambda c: c.CDLNet(K=3, M=169, P=7, s=2, C=1, t0=5e-3, adaptive=True, init=True), (1, 1, 75, 77), False),
}


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("sig", ["map", "levels"])
@pytest.mark.parametrize("name", list(NETS))
def test_net_forward_backward_on_views(name, sig, off):
    c = cva()
    make, shape, masked = NETS[name]
    torch.manual_seed(3)
    net = detie(make(c), 11)
    gen = torch.Generator().manual_seed(5)
    x = c.utils.synthetic_clip(shape, seed=6)
    y = x + torch.randn(shape, generator=gen) * 25 / 255
    mask = c.gen_bayer_mask(x) if masked else None
    if masked:
        y = y * mask
    from cdlnet_video_amd.net import _code_grid
    sigma = sigma_for(sig, shape[0], _code_grid(shape[2:], net.s), gen)
    views_vs_clones(f"{name} {sig}", fwd_bwd(net, x.cuda(), masked), {"y": y, "sigma": sigma, "mask": mask} if masked
                    else {"y": y, "sigma": sigma}, off)


@pytest.mark.parametrize("off", [1, 2])
def test_jvp_with_v_a_view(off):
    c = cva()
    torch.manual_seed(4)
    net = detie(c.CDLNet(K=4, M=32, P=7, s=1, C=1, t0=5e-3, adaptive=True, init=True), 12)
    shape = (2, 1, 48, 40)
    gen = torch.Generator().manual_seed(7)
    y = c.utils.synthetic_clip(shape, seed=8) + torch.randn(shape, generator=gen) * 25 / 255
    v = torch.randn(shape, generator=gen)

    def call(y, v):
        with torch.no_grad():
            xhat, xdot = net.jvp(y, v, 25.0)
        return {"xhat": xhat, "xdot": xdot}
    views_vs_clones("jvp", call, {"y": y, "v": v}, off)


def csr_nets():
    c = cva()
    torch.manual_seed(1)
    kw = dict(K=3, M=8, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True)
    one, two = c.CDLNet_CSR(**kw), c.CDLNet_CSRf2(**kw)
    with torch.no_grad():
        one.g.fill_(0.5)
        two.g1.fill_(0.6)
        two.g2.fill_(0.4)
    return detie(one, 13), detie(two, 14)


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("driver", ["loop", "v2"])
def test_recurrent_drivers_on_unbound_clip(driver, off):
    """frames = list(clip.unbind(0)) of a (T,1,1,21,23) clip: 483 floats per frame, every second one 4-byte aligned; sigma
    a (T,1,Hc,Wc) tensor of maps that _per_frame_sigma splits into views.  Against lists of cloned frames and maps."""
    c = cva()
    one, two = csr_nets()
    T = 4
    gen = torch.Generator().manual_seed(9)
    clip = c.utils.synthetic_clip((T, 1, 21, 23), seed=10).reshape(T, 1, 1, 21, 23)
    clip = clip + torch.randn(clip.shape, generator=gen) * 25 / 255
    sigma = 15.0 + 20.0 * torch.rand((T, 1, 21, 23), generator=gen)
    net, fn = (one, c.csr_inference_loop) if driver == "loop" else (two, c.csr_inference_v2)
    o = c.ops
    arena = Arena("cuda")
    clip_v, sigma_v = arena.put(clip, off, "clip"), arena.put(sigma, off, "sigma")
    frames = list(clip_v.unbind(0))
    assert {f.data_ptr() % 16 for f in frames} >= {4 * off, (4 * off + 483 * 4) % 16}
    with o.trace() as t0:
        ref = fn(net, [f.clone() for f in frames], [sigma_v[t:t + 1].clone() for t in range(T)])
        torch.cuda.synchronize()
    with o.trace() as t1:
        got = fn(net, frames, sigma_v)
        torch.cuda.synchronize()
    arena.check()
    assert torch.equal(clip_v.cpu(), clip) and torch.equal(sigma_v.cpu(), sigma)
    assert len(got) == len(ref) == T
    compare(f"csr {driver} off{off}", t0, t1, {f"frame {t}": ref[t] for t in range(T)}, {f"frame {t}": got[t] for t in range(T)})
    # a caller feeds the returned frames onwards: the slices csr_inference_v2 returns are views too
    stacked = torch.stack([g.contiguous() for g in got])
    assert torch.equal(c.ssim(got[1], got[2], data_range=1.0), c.ssim(stacked[1], stacked[2], data_range=1.0))


@pytest.mark.parametrize("off", [1, 2])
def test_csr_step_with_neighbour_codes_from_one_stacked_tensor(off):
    c = cva()
    from cdlnet_video_amd.temporal import csr_step
    _, two = csr_nets()
    shape = (1, 1, 21, 23)
    gen = torch.Generator().manual_seed(15)
    x = c.utils.synthetic_clip(shape, seed=16)
    y = x + torch.randn(shape, generator=gen) * 25 / 255
    codes = 0.05 * torch.randn((2, 1, 8, 21, 23), generator=gen) * (torch.rand((2, 1, 8, 21, 23), generator=gen) < 0.4)
    sigma = 15.0 + 20.0 * torch.rand((1, 1, 21, 23), generator=gen)
    target = x.cuda()

    def call(y, codes, sigma):
        two.zero_grad(set_to_none=True)
        codes = codes.detach().requires_grad_()
        y = y.detach().requires_grad_()
        z_prev, z_after = codes[0], codes[1]                     # 8 * 483 floats apart: views of one recorded tensor
        xhat, z = csr_step(two, y, z_prev, z_after, sigma=sigma)
        (torch.mean((target - xhat) ** 2) + 1e-3 * z.abs().mean()).backward()
        out = {"xhat": xhat.detach(), "z": z.detach(), "grad y": y.grad, "grad codes": codes.grad}
        out.update({f"grad {n}": p.grad.clone() for n, p in two.named_parameters() if p.grad is not None})
        return out
    views_vs_clones("csr_step", call, {"y": y, "codes": codes, "sigma": sigma}, off)


@pytest.mark.parametrize("off", [1, 2])
def test_building_blocks_on_views(off):
    """cva.ST, prox_CSR_f2, functional.analysis / synthesis with gradients to every tensor argument."""
    c = cva()
    Fn = c.functional
    gen = torch.Generator().manual_seed(17)
    N, C, M, H, W, P = 2, 1, 8, 21, 23, 5
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(M, C, P, P, generator=gen) * 0.2
    u = 0.05 * torch.randn(N, M, H, W, generator=gen)
    zp = 0.05 * torch.randn(N, M, H, W, generator=gen) * (torch.rand(N, M, H, W, generator=gen) > 0.4)
    za = 0.05 * torch.randn(N, M, H, W, generator=gen) * (torch.rand(N, M, H, W, generator=gen) > 0.4)
    lam = torch.rand(1, M, 1, 1, generator=gen) * 0.02
    g1 = torch.rand(1, M, 1, 1, generator=gen) * 1.2
    g2 = torch.rand(1, M, 1, 1, generator=gen) * 1.2
    up = torch.randn(N, M, H, W, generator=gen).cuda()
    upx = torch.randn(N, C, H, W, generator=gen).cuda()

    def call(x, w, u, zp, za, lam, g1, g2):
        leaves = {k: v.detach().requires_grad_() for k, v in dict(x=x, w=w, u=u, zp=zp, za=za, lam=lam, g1=g1, g2=g2).items()}
        L = leaves
        a = Fn.analysis(L["x"], L["w"], 1)
        st = c.ST(L["u"], L["lam"])
        pr = c.prox_CSR_f2(L["u"], L["zp"], L["za"], L["lam"], L["g1"], L["g2"])
        sy = Fn.synthesis(L["zp"], L["w"], 1)
        ((a * up).sum() + (st * up).sum() + (pr * up).sum() + (sy * upx).sum()).backward()
        out = {"analysis": a.detach(), "ST": st.detach(), "prox_CSR_f2": pr.detach(), "synthesis": sy.detach()}
        out.update({f"grad {k}": v.grad for k, v in leaves.items()})
        return out
    views_vs_clones("blocks", call, dict(x=x, w=w, u=u, zp=zp, za=za, lam=lam, g1=g1, g2=g2), off)


@pytest.mark.parametrize("off", [1, 2])
def test_ssim_on_contiguous_planes_of_a_batch(off):
    """cva.metrics.ssim on x[n]-style views of a carved batch: odd plane sizes, so the planes alternate in alignment."""
    c = cva()
    gen = torch.Generator().manual_seed(18)
    X = torch.rand(3, 2, 1, 33, 35, generator=gen)
    Y = (X + 0.1 * torch.randn(X.shape, generator=gen)).clamp(0, 1)

    def call(X, Y):
        out = {}
        for n in range(3):
            xn = X[n].detach().requires_grad_()
            s = c.metrics.ssim(xn, Y[n], data_range=1.0)
            s.backward()
            out[f"ssim {n}"], out[f"grad x {n}"] = s.detach(), xn.grad
        return out
    views_vs_clones("ssim", call, {"X": X, "Y": Y}, off)
