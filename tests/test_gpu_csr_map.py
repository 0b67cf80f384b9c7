"""Noise-level maps and data gradients of the CSR nets on the device: the reference's fixtures
replayed through temporal.csr_step, a constant map against one level per sample, and the frame-recurrent drivers."""
import pytest
import torch

from csr_map_util import FIXTURES, INTERNAL, VARIANT, replay
from gpu_util import check, load_golden

pytestmark = pytest.mark.gpu

XTOL, GTOL = 1e-5, 2e-4
XHAT_OF = {"grad_z0": "xh0", "grad_z1": "xh1", "grad_zp": "xp", "grad_zc": "xc", "grad_za": "xa"}   # the call that made z


def build(g, variant):
    import cdlnet_video_amd as cva
    K, M, P, s, C = g["hyper"]
    cls = cva.CDLNet_CSR if variant == "csr" else cva.CDLNet_CSRf2
    net = cls(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=True, init=False)
    net.load_state_dict(g["sd"])
    return net.cuda()


@pytest.mark.parametrize("kind", sorted(FIXTURES))
def test_fixture_through_csr_step(kind):
    """Every recorded value of the reference run: xhat / z of every call, the parameter gradients, dL/dy, dL/dsigma in
    the shape sigma was given, and the neighbour-code gradients."""
    import cdlnet_video_amd as cva
    g = load_golden(FIXTURES[kind])
    net = build(g, VARIANT[kind])
    call = lambda y, zp, za, sigma: cva.temporal.csr_step(net, y, zp, za, sigma)
    loss, outs, leaves = replay(kind, g, call, "cuda")
    for name, got in outs.items():
        check(f"csr_step {kind} {name}", got, g[name], XTOL)
    assert abs(float(loss.detach()) - g["loss"]) < 1e-5 * max(1.0, abs(g["loss"]))
    for name in XHAT_OF.values():
        if name in outs:
            outs[name].retain_grad()
    loss.backward()
    F = cva.functional
    for name, t in leaves.items():
        if name in INTERNAL:
            # a code the chain hands on: the reference's retained .grad is what reaches z from the later calls (the .grad
            # of the z csr_step returned) plus the path through the same call's xhat = crop(D z) + mean, D = B[0]
            zz = outs[name[5:]].detach().requires_grad_(True)
            s_ = net.s
            params = [torch.zeros(zz.shape[0], 1, 1, 1, device="cuda"), cva.ops.stride_pads(g["w"].shape[2:], s_)]
            xx = F.post_process(F.synthesis(zz, net.B[0].weight.detach(), s_), params)
            (inner,) = torch.autograd.grad(xx, zz, outs[XHAT_OF[name]].grad)
            check(f"csr_step {kind} {name}", t.grad + inner, g[name], GTOL)
            continue
        assert t.grad is not None and t.grad.shape == g[name].shape, name
        check(f"csr_step {kind} {name}", t.grad, g[name], GTOL)
    n = 0
    for name, p in net.named_parameters():
        ref = g["grad"].get(name)                              # absent: the reference left it without a gradient
        if p.grad is None or ref is None:                      # a parameter no call of the chain uses
            assert ref is None or float(ref.abs().max()) == 0.0, name
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        check(f"csr_step {kind} grad {name}", p.grad, ref, GTOL)
        n += 1
    assert n >= 5


def detied(cls, seed, **kw):
    """A small net with distinct filters per iteration and thresholds away from ties."""
    torch.manual_seed(seed)
    net = cls(t0=5e-3, adaptive=True, init=True, **kw)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n in ("t", "t2"):
                p.uniform_(2e-3, 1.5e-2)
            elif n in ("g", "g1", "g2"):
                p.uniform_(0.2, 1.4)
            else:
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    return net.cuda()


@pytest.mark.parametrize("both", [False, True])
def test_constant_map_equals_one_level_per_sample(both):
    """A map that is constant over each sample's pixels against the per-sample sigma of the same values: xhat / z, and
    dL/dsigma of the map summed to the per-sample shape.  The (N,1,1,1), (1,1,Hc,Wc) and (N,1,Hc,Wc) forms agree."""
    import cdlnet_video_amd as cva
    net = detied(cva.CDLNet_CSRf2, 31, K=3, M=8, P=5, s=2, C=1)
    N, sp = 2, (22, 26)
    x = cva.utils.synthetic_clip((N, 1) + sp, seed=3).cuda()
    gen = torch.Generator().manual_seed(32)
    y = x + (torch.randn(x.shape, generator=gen) * 25 / 255).cuda()
    w = torch.randn(x.shape, generator=gen).cuda()
    with torch.no_grad():
        _, zp = net(y, None, None, 25.0)
        _, za = net(y.flip(0), None, None, 25.0)
    za = za if both else None

    def run(sigma):
        sigma = sigma.clone().requires_grad_(True)
        yy = y.clone().requires_grad_(True)
        xhat, z = cva.temporal.csr_step(net, yy, zp, za, sigma)
        (torch.mean((x - xhat) ** 2) + torch.mean(w * xhat) + 0.1 * z.abs().mean()).backward()
        grads = [p.grad.clone() for p in net.parameters() if p.grad is not None]
        net.zero_grad(set_to_none=True)
        return xhat.detach(), z.detach(), sigma.grad, yy.grad, grads

    tag = f"constant map[{'f2' if both else 'f1'}]"
    for levels, forms in ((torch.tensor([15.0, 30.0]), [(N, 1, 11, 13)]),
                          (torch.tensor([25.0, 25.0]), [(1, 1, 11, 13), (N, 1, 11, 13)])):
        per = levels.reshape(N, 1, 1, 1).cuda()
        ref = run(per)
        assert ref[2].shape == per.shape
        full = None
        for shape in reversed(forms):                              # the (N,1,Hc,Wc) form first
            got = run(per[:shape[0]].expand(shape).contiguous())
            assert got[2].shape == shape
            check(f"{tag} {shape} xhat", got[0], ref[0], 1e-6)
            check(f"{tag} {shape} z", got[1], ref[1], 1e-6)
            if shape[0] == N:
                full = got[2]
                check(f"{tag} {shape} dsigma", full.sum_to_size(per.shape), ref[2], 1e-6)
            else:       # one map for every sample: the sum over the samples of the full form's gradient, pixel by pixel
                check(f"{tag} {shape} dsigma", got[2], full.sum(0, keepdim=True), 1e-6)
                # and summed to one number against the per-sample gradients: the two samples' terms cancel to 1e-5 of
                # their size, so the bound is 1e-6 of the size of the terms, not of the difference that is left
                assert abs(float(got[2].sum() - ref[2].sum())) <= 1e-6 * float(ref[2].abs().sum()), (tag, shape)
            check(f"{tag} {shape} dy", got[3], ref[3], 1e-6)
            for i, (a, b) in enumerate(zip(got[4], ref[4])):
                check(f"{tag} {shape} grad {i}", a, b, 1e-5)


def test_csr_step_returns_the_bits_of_the_net_call():
    """With a scalar or per-sample sigma and nothing requiring a data gradient csr_step is net(...), on every branch."""
    import cdlnet_video_amd as cva
    x = cva.utils.synthetic_clip((2, 1, 20, 24), seed=5).cuda()
    sig = torch.tensor([15.0, 30.0]).reshape(2, 1, 1, 1).cuda()
    f2 = detied(cva.CDLNet_CSRf2, 33, K=2, M=6, P=5, s=1, C=1)
    one = detied(cva.CDLNet_CSR, 34, K=2, M=6, P=5, s=1, C=1)
    with torch.no_grad():
        _, z = f2(x, None, None, 25.0)
        for sigma in (25.0, sig):
            for prev, after in ((None, None), (z, None), (None, z), (z, z.flip(0))):
                a, b = f2(x, prev, after, sigma), cva.temporal.csr_step(f2, x, prev, after, sigma)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            for prev in (None, z):
                a, b = one(x, prev, sigma), cva.temporal.csr_step(one, x, prev, None, sigma)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xh, _ = cva.temporal.csr_step(f2, x, z, z.flip(0), sig)                      # and the parameter gradients
    xh.square().mean().backward()
    got = [p.grad.clone() for p in f2.parameters()]
    f2.zero_grad(set_to_none=True)
    xh, _ = f2(x, z, z.flip(0), sig)
    xh.square().mean().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(got, f2.parameters()))
    with pytest.raises(ValueError):
        cva.temporal.csr_step(f2, x, z, None, torch.rand(2, 1, 7, 7).cuda())    # no broadcast form of the code grid
    with pytest.raises(ValueError):
        cva.temporal.csr_step(one, x, z, z, 25.0)


# ------------------------------------------------------------------------------------------ drivers
def _frames(T, N, sp, seed):
    import cdlnet_video_amd as cva
    gen = torch.Generator().manual_seed(seed)
    clean = [cva.utils.synthetic_clip((N, 1) + sp, seed=seed + t) for t in range(T)]
    return [(c + torch.randn(c.shape, generator=gen) * 25 / 255).cuda() for c in clean]


def _maps(T, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(10.0 + 30.0 * torch.rand(shape, generator=gen)).cuda() for _ in range(T)]


def test_inference_v2_with_per_frame_maps():
    import cdlnet_video_amd as cva
    net = detied(cva.CDLNet_CSRf2, 35, K=2, M=6, P=5, s=1, C=1)
    T, N, sp = 3, 1, (20, 24)
    frames, maps = _frames(T, N, sp, 40), _maps(T, (1, 1) + sp, 41)
    step = cva.temporal.csr_step
    with torch.no_grad():
        codes = [None] * (T + 2)
        for t in range(T):
            _, codes[t + 1] = step(net, frames[t], codes[t], None, maps[t])
        want = [step(net, frames[0], None, codes[1], maps[0])[0]]
        want += [step(net, frames[t], codes[t], codes[t + 1], maps[t])[0] for t in range(1, T)]
    for sigma in (maps, torch.cat(maps)):                                        # a list, or a (T,1,Hc,Wc) tensor
        got = cva.csr_inference_v2(net, frames, sigma)
        assert len(got) == T and all(torch.equal(a, b) for a, b in zip(got, want))
    with torch.no_grad():                                                        # a float sigma: today's calls
        codes = [None] * (T + 2)
        for t in range(T):
            _, codes[t + 1] = net(frames[t], codes[t], None, 25.0)
        want = [net(frames[0], None, codes[1], 25.0)[0]]
        xb, _ = net(torch.cat(frames[1:]), torch.cat(codes[1:T]), torch.cat(codes[2:T + 1]), 25.0)
        want += [xb[i * N:(i + 1) * N] for i in range(T - 1)]
    got = cva.csr_inference_v2(net, frames, 25.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_inference_loop_with_per_frame_maps():
    import cdlnet_video_amd as cva
    net = detied(cva.CDLNet_CSR, 36, K=2, M=6, P=5, s=2, C=1)
    T, N, sp = 3, 2, (19, 21)
    frames, maps = _frames(T, N, sp, 50), _maps(T, (N, 1, 10, 11), 51)
    step = cva.temporal.csr_step

    def chain(call, sig):
        with torch.no_grad():
            _, zp = call(frames[0], None, sig(0))
            _, zc = call(frames[1], zp, sig(1))
            first, zp = call(frames[0], zc, sig(0))
            out = [first]
            for t in range(1, T):
                xh, zp = call(frames[t], zp, sig(t))
                out.append(xh)
        return out

    want = chain(lambda y, zp, s_: step(net, y, zp, None, s_), lambda t: maps[t])
    got = cva.csr_inference_loop(net, frames, maps)
    assert len(got) == T and all(torch.equal(a, b) for a, b in zip(got, want))
    want = chain(lambda y, zp, s_: net(y, zp, s_), lambda t: 25.0)
    got = cva.csr_inference_loop(net, frames, 25.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_clip_forward_with_maps():
    """train.clip_forward goes through csr_step for the frames whose sigma is a map, and the chain is differentiable."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import train
    net = detied(cva.CDLNet_CSR, 37, K=2, M=6, P=5, s=1, C=1)
    frames, maps = _frames(2, 2, (20, 24), 60), _maps(2, (2, 1, 20, 24), 61)
    step = cva.temporal.csr_step
    cur = None
    for _ in range(2):
        out0, prev = step(net, frames[0], cur, None, maps[0])
        out1, cur = step(net, frames[1], prev, None, maps[1])
    got = train.clip_forward(net, frames, maps)
    assert torch.equal(got[0], out0) and torch.equal(got[1], out1)
    (got[0].square().mean() + got[1].square().mean()).backward()
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert grads["B2.0.weight"] is None                        # never applied: D is B[0]
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for n, v in grads.items() if n != "B2.0.weight")
