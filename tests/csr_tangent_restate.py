"""Float64 restatement of the CSR nets' tangent (jvp_recurrent), from the oracle's operators alone.

prox_CSR / prox_CSR_f2 are piecewise linear in (u, z_prev, z_after).  Which piece a code element sits on is decided by the
gates st_dx(x, t) = (x != 0 and |x| - t > 0) of the nested shrinkages; `gates` evaluates them in float32 from a given
(u_k, z_prev, z_after, lam, gam*), term by term in the reference's order (model/net.py:229-262) -- the decisions the device
takes from the same numbers.  Given the gates the tangent is a select (`prox_tangent`), the sweep a linear recursion
(`tangent_sweep`) and everything after that runs in float64 under autograd.  This plays the role `supports=` plays in
tangent_util.py: a device result is compared at ITS OWN gates, so a gate that differs between two arithmetics (the
split-bf16 tier against fp32) does not enter the comparison.

`call` / `chain` restate one network call and the trainer's clip chains (traincsr.py:201-204, 257-261) with the gates taken
from a float32 run of the same call on the CPU."""
import torch

from oracle import cdl_oracle as O


def st_dx(x, t):
    return (x != 0) & (x.abs() - t > 0)


def gates(u, zp, za, lam, g1, g2=None):
    """The gates of prox_CSR (za None: (Ga, Gm)) / prox_CSR_f2 ((Ga, Gb, Gm)) in the arithmetic of the inputs; lam, g* broadcast
    against u as the reference's thresholds do ((N,M,1,1))."""
    sign, ST = torch.sign, O.soft_threshold
    if za is None:
        ls = lam * sign(zp)
        a = u - zp - ls
        tg = lam * g1
        m = ST(a, tg) + zp + ls
        return st_dx(a, tg), st_dx(m, lam)
    ca = zp + lam * sign(zp) + lam * g2 * sign(zp - za)
    cb = za + lam * sign(za) + lam * g1 * sign(za - zp)
    a = u - ca
    inner = ST(a, g1 * lam)
    b = inner - cb + lam * g1 * sign(a)
    mid = ST(b, g2 * lam)
    m = mid + cb - lam * g1 * sign(a)
    return st_dx(a, g1 * lam), st_dx(b, g2 * lam), st_dx(m, lam)


def prox_tangent(G, ud, zpd=None, zad=None):
    """The tangent of the map on the piece `G` selects, along (ud, zpd, zad); a None neighbour tangent is zero.  A single
    gate (G,) is the plain shrinkage's: [z != 0] ud."""
    zero = torch.zeros_like(ud)
    zpd = zero if zpd is None else zpd
    if len(G) == 1:
        return torch.where(G[0], ud, zero)
    if len(G) == 2:
        Ga, Gm = G
        return torch.where(Gm, torch.where(Ga, ud, zpd), zero)
    Ga, Gb, Gm = G
    zad = zero if zad is None else zad
    return torch.where(Gm, torch.where(Gb, torch.where(Ga, ud - zpd, zero), zad), zero)


def tangent_sweep(A, B, vp, mask_p, G, zpd, zad, s, pad, D=None):
    """ud_0 = A_0 vp, rd_k = mask B_k zd_k - vp, ud_k = zd_k - A_k rd_k, zd_{k+1} = Jprox_k(ud_k; zpd, zad), xdp = D zd_K.
    G[k]: the gates of iteration k.  Returns (xdp, zd_K)."""
    zd = prox_tangent(G[0], O.analysis(vp, A[0], s, pad), zpd, zad)
    for k in range(1, len(A)):
        r = O.synthesis(zd, B[k], s, pad)
        if mask_p is not None:
            r = mask_p * r
        zd = prox_tangent(G[k], zd - O.analysis(r - vp, A[k], s, pad), zpd, zad)
    return O.synthesis(zd, B[0] if D is None else D, s, pad), zd


def branch(sd, variant, z_prev, z_after, K):
    """(A, B, t, g1, g2, zp, za) of the branch forward takes (net.py:438-455, 545-563); zp None: the plain loop."""
    A, B = [sd[f"A.{k}.weight"] for k in range(K)], [sd[f"B.{k}.weight"] for k in range(K)]
    if variant == "csr":
        assert z_after is None
        if z_prev is None:
            return ([sd[f"A2.{k}.weight"] for k in range(K)], [sd[f"B2.{k}.weight"] for k in range(K)], sd["t2"], None, None,
                    None, None)
        return A, B, sd["t"], sd["g"], None, z_prev, None
    if z_prev is not None and z_after is not None:
        return A, B, sd["t"], sd["g1"], sd["g2"], z_prev, z_after
    if z_prev is not None:
        return A, B, sd["t"], sd["g1"], None, z_prev, None
    if z_after is not None:
        return A, B, sd["t"], sd["g2"], None, z_after, None
    return A, B, sd["t"], None, None, None, None


def primal_gates(sd, variant, y, z_prev, z_after, *, K, P, s, sigma, adaptive=True, mask=None):
    """One forward call in the arithmetic of the inputs, keeping the gates of every iteration: [G_0..G_{K-1}]."""
    A, B, t, g1, g2, zp, za = branch(sd, variant, z_prev, z_after, K)
    yp, _, _, mask_p = O.preprocess(y, s, mask)
    c = 0.0 if (sigma is None or not adaptive) else sigma / 255.0
    pad = O._conv_pad(P, 2)
    th = lambda p, k: O._thresholds(p, k, c)
    G, z = [], None
    for k in range(K):
        if k == 0:
            u = O.analysis(yp, A[0], s, pad)
        else:
            r = O.synthesis(z, B[k], s, pad)
            if mask_p is not None:
                r = mask_p * r
            u = z - O.analysis(r - yp, A[k], s, pad)
        if zp is None:
            z = O.soft_threshold(u, th(t, k))
            G.append((z != 0,))
        elif za is None:
            G.append(gates(u, zp, None, th(t, k), th(g1, k)))
            z = O.prox_csr(u, zp, th(t, k), th(g1, k))
        else:
            G.append(gates(u, zp, za, th(t, k), th(g1, k), th(g2, k)))
            z = O.prox_csr_f2(u, zp, za, th(t, k), th(g1, k), th(g2, k))
    return G


def call(sd, variant, y, v, prev=None, after=None, *, K, P, s, sigma, adaptive=True, mask=None, G=None):
    """jvp_recurrent of one call in float64: (xhat, xdot, z, zd), differentiable in the float64 leaves of `sd` and in the
    incoming (z, zd) pairs `prev` / `after`.  G: the gates (default: those of a float32 run of this call)."""
    z_prev, zd_prev = prev if prev is not None else (None, None)
    z_after, zd_after = after if after is not None else (None, None)
    kw = dict(K=K, P=P, s=s, sigma=sigma, adaptive=adaptive, mask=mask)
    if G is None:
        f = lambda x: x.detach().float() if torch.is_tensor(x) else x
        G = primal_gates({k: f(w) for k, w in sd.items()}, variant, f(y), f(z_prev), f(z_after),
                         **{k: f(w) for k, w in kw.items()})
    xhat, z = O.ista_csr(sd, y, z_prev, z_after, variant="f2" if variant == "f2" else "csr", **kw)
    A, B, _, _, _, zp, za = branch(sd, variant, z_prev, z_after, K)
    vp, vmean, pads, mask_p = O.preprocess(v, s, mask)
    if variant == "f2" and z_prev is None and z_after is not None:
        zpd, zad = zd_after, None                      # the one-neighbour map around z_after
    else:
        zpd, zad = zd_prev, zd_after
    xdp, zd = tangent_sweep(A, B, vp, mask_p, G, zpd if zp is not None else None, zad if za is not None else None, s,
                            O._conv_pad(P, 2), D=sd["B.0.weight"])
    return xhat, O.postprocess(xdp, vmean, pads), z, zd


def chain(sd, variant, ys, bs, sigmas, **kw):
    """The clip chains of traincsr.py (CDLNet_CSR: 201-204 on 2 frames; CDLNet_CSRf2: 257-261 on 3, the third call's input
    repaired to the noisy third frame) run with `call`, the (z, zd) pair of one call fed to its neighbour's.  Returns
    {frame: (xhat, xdot)} of the calls that enter the loss."""
    run = lambda t, prev, after: call(sd, variant, ys[t], bs[t], prev, after, sigma=sigmas[t], **kw)
    if variant == "csr":
        cur = None
        for _ in range(2):
            xp, xdp, z, zd = run(0, cur, None)
            xc, xdc, zc, zdc = run(1, (z, zd), None)
            cur = (zc, zdc)
        return {0: (xp, xdp), 1: (xc, xdc)}
    xp, xdp, z, zd = run(0, None, None)
    prev = (z, zd)
    run(1, prev, None)
    xa, xda, za, zda = run(2, prev, None)
    xc, xdc, _, _ = run(1, prev, (za, zda))
    xp, xdp, _, _ = run(0, None, (za, zda))
    return {0: (xp, xdp), 1: (xc, xdc), 2: (xa, xda)}


def sure(outs, ys, bs, sigmas):
    """sum_t mean((y_t - xhat_t)^2) + 2 mean((sigma_t / 255)^2 b_t xdot_t)."""
    loss = 0.0
    for t, (xhat, xdot) in outs.items():
        loss = loss + torch.mean((ys[t] - xhat) ** 2) + 2.0 * torch.mean((sigmas[t] / 255.0) ** 2 * bs[t] * xdot)
    return loss
