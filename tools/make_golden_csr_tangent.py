#!/usr/bin/env python3
"""Generate tests/golden/c5..c9 (the tangent of the CSR nets and their clip training steps) by running the UNMODIFIED
reference on CPU: prox_CSR / prox_CSR_f2 and CDLNet_CSR / CDLNet_CSRf2 (model/net.py) under forward-mode autograd, and
utils.awgn.  Same shims as tools/make_golden.py, `detie` / `smooth` as tools/make_golden_csr.py uses them.

    c5_csr_tangent_pointwise   the jvp of the two proximal maps on the c0 grid and its five threshold cases (exact zeros,
                               ties, negative thresholds), random tangents
    c6_csr_jvp_chain           the jvp of CDLNet_CSR's 4-call clip chain (traincsr.py:201-204) jointly in both frames, the
                               SURE loss  sum_t mean((y_t - xhat_t)^2) + 2 mean((sigma_t/255)^2 b_t xdot_t)  and its gradients
    c7_csrf2_jvp_chain         the same for CDLNet_CSRf2's 5-call chain (traincsr.py:257-261; line 259 names its own output
                               as its input -- the noisy third frame is passed, the z_prev of that call stays as written)
    c8_csr_clip_step           one supervised clip step (loss, gradient norm, post-Adam weights) of CDLNet_CSR
    c9_csrf2_clip_step         ... of CDLNet_CSRf2, at one noise level for all frames (awgn's scalar form)

Route of c8 / c9: traincsr.py does not import under the stubs tools/make_golden_fit.py uses (its data module,
datafastmri, imports h5py, which is not installed), so the call sequence of its train_model is restated here around the unmodified nets and the
unmodified awgn, statement by statement (noise draws first, in frame order; zero_grad; the chain; the summed MSE;
backward; clip_grad_norm_; Adam step; no projection).

Seed rule of c6 / c7: every shrinkage argument of the chain is recorded (a pass-through wrapper around model.net.ST) in the
float32 run and in a float64 run of the same chain; a seed is accepted only if the gate patterns  (x != 0 and |x| - t > 0)
agree everywhere.  The smallest | |x| - t | of the float32 run is stored as `gate_margin`.  The jvp must also agree with a
float64 central finite difference (h = 1e-7) to 5e-7 of max; a seed whose difference straddles a gate is passed over too.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_csr_tangent.py
"""
import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwad

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, save, smooth, state, grads_of   # noqa: E402
from make_golden_csr import detie                                               # noqa: E402


def chain(net, variant, ys, sigmas):
    """The trainer's clip chain (cdlnet_video_amd.train._clip_chain: the order of network calls of traincsr.py's
    train_model, which code feeds which call) driven over the unmodified reference net; the outputs that enter the loss."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from cdlnet_video_amd.train import _clip_chain
    if variant == "csr":
        call = lambda t, prev, after: net(ys[t], prev, sigmas[t])
    else:
        call = lambda t, prev, after: net(ys[t], prev, after, sigmas[t])
    outs = _clip_chain(call, len(ys))
    return [outs[t] for t in range(len(ys))]


class Recorder:
    """Pass-through wrapper of model.net.ST that keeps the gate pattern and the margin of every call."""

    def __init__(self, net_mod):
        self.mod, self.orig, self.gates, self.margin = net_mod, net_mod.ST, [], float("inf")

    def __enter__(self):
        def ST(x, t):
            xv = (fwad.unpack_dual(x).primal if torch.is_tensor(x) else x).detach()
            tv = (fwad.unpack_dual(t).primal if torch.is_tensor(t) else torch.as_tensor(t)).detach()
            d = xv.abs() - tv
            self.gates.append((xv != 0) & (d > 0))
            self.margin = min(self.margin, float(d.abs().min()))
            return self.orig(x, t)
        self.mod.ST = ST
        return self

    def __exit__(self, *exc):
        self.mod.ST = self.orig
        return False


def jvp_fixture(net_mod, name, variant, seed, shape, sigma_of, thr):
    """Try seeds from `seed` upwards until the float32 and float64 gate patterns agree; write the fixture."""
    D = 2 if variant == "csr" else 3
    cls = net_mod.CDLNet_CSR if variant == "csr" else net_mod.CDLNet_CSRf2
    mse = lambda a, b: torch.mean((a - b) ** 2)
    for sd_ in range(seed, seed + 50):
        g = torch.Generator().manual_seed(sd_)
        torch.manual_seed(sd_)
        net = cls(K=3, M=6, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True)
        detie(net, g, thr)
        xs = [smooth(shape, g)]
        for _ in range(D - 1):
            xs.append((0.9 * xs[-1] + 0.1 * smooth(shape, g)).clamp(0, 1))
        sig = sigma_of(shape[0])
        sigmas = [sig] * D
        ys = [x + torch.randn(shape, generator=g) * sig / 255 for x in xs]
        bs = [torch.randn(shape, generator=g) for _ in range(D)]
        with Recorder(net_mod) as r32, fwad.dual_level():
            outs = chain(net, variant, [fwad.make_dual(y.clone(), b) for y, b in zip(ys, bs)], sigmas)
            xh, xd = zip(*(fwad.unpack_dual(o) for o in outs))
            loss = sum(mse(y, a) + 2.0 * torch.mean((s_ / 255.0) ** 2 * b * d)
                       for y, a, b, d, s_ in zip(ys, xh, bs, xd, sigmas))
            loss.backward()
        net64 = cls(K=3, M=6, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=False).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        d64 = lambda t: t.double() if torch.is_tensor(t) else t
        with Recorder(net_mod) as r64, fwad.dual_level():
            outs64 = chain(net64, variant, [fwad.make_dual(y.double(), b.double()) for y, b in zip(ys, bs)],
                           [d64(s_) for s_ in sigmas])
            xd64 = [fwad.unpack_dual(o).tangent.detach() for o in outs64]
        same = len(r32.gates) == len(r64.gates) and all(bool((a == b).all()) for a, b in zip(r32.gates, r64.gates))
        print(f"{name}: seed {sd_}: gates agree: {same}; margin {r32.margin:.3e}")
        if not same:
            continue
        # the jvp against a float64 central difference of the same chain
        h = 1e-7
        with torch.no_grad():
            up = chain(net64, variant, [y.double() + h * b.double() for y, b in zip(ys, bs)], [d64(s_) for s_ in sigmas])
            dn = chain(net64, variant, [y.double() - h * b.double() for y, b in zip(ys, bs)], [d64(s_) for s_ in sigmas])
        fd_err = max(float(((a - c) / (2 * h) - d).abs().max() / d.abs().max()) for a, c, d in zip(up, dn, xd64))
        print(f"{name}: jvp vs float64 central difference (h = {h}): {fd_err:.2e}")
        if fd_err >= 5e-7:                              # a gate within h |tangent| of its threshold: the difference straddles it
            continue
        arrays = {f"x{t}": xs[t] for t in range(D)}
        arrays.update({f"y{t}": ys[t] for t in range(D)})
        arrays.update({f"b{t}": bs[t] for t in range(D)})
        arrays.update({f"xhat{t}": xh[t] for t in range(D)})
        arrays.update({f"xdot{t}": xd[t] for t in range(D)})
        save(name, sigma=sig, loss=loss, seed=sd_, gate_margin=r32.margin, fd_err=fd_err, **arrays, **state(net),
             **grads_of(net), hyper=np.array([3, 6, 5, 1, 1]))
        return
    raise SystemExit(f"{name}: no seed with equal float32 / float64 gates")


def clip_step_fixture(net_mod, ref_utils, name, variant, seed, shape5, thr, noise_std=(20, 30), tries=50):
    """traincsr.py's train_model for this model type (phase 'train', supervised), restated around the unmodified net.
    Seed choice (the issue sets none for these fixtures; made before any device run): of the `tries` seeds from `seed`
    upwards, the one whose float32 run has the fewest gate decisions that differ from a float64 run of the same chain, and
    among those the one whose post-step weights are best conditioned (`step`: the smallest Adam sensitivity; the device test
    holds the post-step weights to 2e-5); both figures and the gate margin are stored."""
    cls = net_mod.CDLNet_CSR if variant == "csr" else net_mod.CDLNet_CSRf2
    B, C, D, H, W = shape5
    lr, clip_grad = 1e-3, 5e-2

    def prepare(sd_):
        g = torch.Generator().manual_seed(sd_)
        torch.manual_seed(sd_)
        net = cls(K=3, M=6, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=True)
        detie(net, g, thr)
        frames = [smooth((B, C, H, W), g)]
        for _ in range(D - 1):
            frames.append((0.9 * frames[-1] + 0.1 * smooth((B, C, H, W), g)).clamp(0, 1))
        batch = torch.stack(frames, dim=2)
        torch.manual_seed(sd_ + 1000)                   # the noise stream a test replays with a CPU generator
        clean = [batch[:, :, d, :, :] for d in range(D)]
        noisy, sigmas = zip(*(ref_utils.awgn(x, noise_std) for x in clean))
        return net, batch, clean, list(noisy), list(sigmas)

    def step(net, clean, noisy, sigmas):
        """The step itself; also how far Adam's first update  lr g / (|g| + 1e-8)  of any entry would move, relative to the
        tensor's largest weight, under a gradient error of 1e-5 of the tensor's largest gradient (the agreement the suite
        holds a device to at identical gates): entries with |g| near Adam's eps make the post-step weights ill-conditioned."""
        before = state(net)
        opt = torch.optim.Adam(net.parameters(), lr=lr)
        opt.zero_grad()
        outs = chain(net, variant, noisy, sigmas)
        losses = [torch.mean((o - x) ** 2) for o, x in zip(outs, clean)]
        loss = sum(losses[1:], losses[0])
        loss.backward()
        grads = grads_of(net)
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), clip_grad)
        sens = 0.0
        for p in net.parameters():
            if p.grad is not None:
                gc = p.grad.abs()
                sens = max(sens, float((lr * 1e-8 * 1e-5 * gc.max() / (gc + 1e-8) ** 2).max() / p.detach().abs().max()))
        opt.step()
        after = {"after/" + k: v.clone() for k, v in net.state_dict().items()}
        return dict(loss=loss, mse=loss / float(D), grad_norm=total, **before, **grads, **after), sens

    best = None
    for sd_ in range(seed, seed + tries):
        net, batch, clean, noisy, sigmas = prepare(sd_)
        net64 = cls(K=3, M=6, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=False).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        with torch.no_grad(), Recorder(net_mod) as r32:
            chain(net, variant, noisy, sigmas)
        with torch.no_grad(), Recorder(net_mod) as r64:
            chain(net64, variant, [y.double() for y in noisy], [s_.double() if torch.is_tensor(s_) else s_ for s_ in sigmas])
        flips = sum(int((a != b).sum()) for a, b in zip(r32.gates, r64.gates))
        payload, sens = step(net, clean, noisy, sigmas)
        print(f"{name}: seed {sd_}: gate decisions that differ: {flips}; margin {r32.margin:.3e}; Adam sensitivity {sens:.2e}")
        if best is None or (flips, sens) < (best[2], best[3]):
            best = (sd_, r32.margin, flips, sens, payload, batch, noisy, sigmas)
    seed, margin, flips, sens, payload, batch, noisy, sigmas = best
    save(name, clip=batch, seed=seed, gate_margin=margin, gate_flips_f32_f64=flips, adam_sensitivity=sens,
         noise_seed=seed + 1000, noise_std=np.array(noise_std, dtype=np.int64), lr=lr, clip_grad=clip_grad,
         **{f"noisy{d}": noisy[d] for d in range(D)}, **{f"sigma{d}": sigmas[d] for d in range(D)}, **payload,
         hyper=np.array([3, 6, 5, 1, 1]))


def main():
    net_mod, ref_utils = import_reference()
    only = set(sys.argv[1:])                            # e.g. `c8 c9`: regenerate these alone
    want = lambda tag: not only or tag in only

    if want("c5"):
        pointwise_fixture(net_mod)
    per_sample = lambda n: torch.tensor([15.0, 30.0][:n]).reshape(n, 1, 1, 1)
    csr_thr = {"t": (2e-3, 1.5e-2), "t2": (2e-3, 1.5e-2), "g": (0.2, 1.4)}
    f2_thr = {"t": (2e-3, 1.5e-2), "g1": (0.2, 1.4), "g2": (0.2, 1.4)}
    # ---- C6 / C7: the jvp of the clip chains, jointly in all frames --------------------------------------------------
    if want("c6"):
        jvp_fixture(net_mod, "c6_csr_jvp_chain", "csr", 61, (2, 1, 20, 24), per_sample, csr_thr)
    if want("c7"):
        jvp_fixture(net_mod, "c7_csrf2_jvp_chain", "f2", 71, (1, 1, 18, 22), lambda n: 25.0, f2_thr)
    # ---- C8 / C9: one supervised clip step ---------------------------------------------------------------------------
    if want("c8"):
        clip_step_fixture(net_mod, ref_utils, "c8_csr_clip_step", "csr", 81, (2, 1, 2, 20, 24), csr_thr)
    if want("c9"):
        clip_step_fixture(net_mod, ref_utils, "c9_csrf2_clip_step", "f2", 91, (1, 1, 3, 18, 22), f2_thr, noise_std=25)


def pointwise_fixture(net_mod):
    c0 = np.load(os.path.join(OUT, "c0_prox_pointwise.npz"))
    u, zp, za = (torch.from_numpy(c0[k]) for k in ("u", "zp", "za"))
    cases = [tuple(float(v) for v in row) for row in c0["cases"]]
    g = torch.Generator().manual_seed(555)
    ud, zpd, zad = (torch.randn(u.shape, generator=g) for _ in range(3))
    T = torch.tensor
    j1 = torch.stack([torch.func.jvp(lambda a, b: net_mod.prox_CSR(a, b, T(l), T(g1)), (u, zp), (ud, zpd))[1]
                      for l, g1, _ in cases])
    j1u = torch.stack([torch.func.jvp(lambda a: net_mod.prox_CSR(a, zp, T(l), T(g1)), (u,), (ud,))[1]
                       for l, g1, _ in cases])
    j2 = torch.stack([torch.func.jvp(lambda a, b, c: net_mod.prox_CSR_f2(a, b, c, T(l), T(g1), T(g2)), (u, zp, za),
                                     (ud, zpd, zad))[1] for l, g1, g2 in cases])
    j2u = torch.stack([torch.func.jvp(lambda a: net_mod.prox_CSR_f2(a, zp, za, T(l), T(g1), T(g2)), (u,), (ud,))[1]
                       for l, g1, g2 in cases])
    save("c5_csr_tangent_pointwise", u=u, zp=zp, za=za, cases=np.array(cases), ud=ud, zpd=zpd, zad=zad, jvp_csr=j1,
         jvp_csr_u=j1u, jvp_csr_f2=j2, jvp_csr_f2_u=j2u)


if __name__ == "__main__":
    main()
