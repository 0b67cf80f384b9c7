"""The CSR call under a noise-level map restated on prescribed PIECES (beside tests/csr_tangent_restate.py, which prescribes
the gates of the tangent alone).

prox_CSR / prox_CSR_f2 are piecewise affine in (u, z_prev, z_after, thresholds).  `pieces` evaluates, in the arithmetic of
its inputs and term by term in the reference's order (model/net.py:229-262), the gates st_dx(x, t) = (x != 0 and |x| - t > 0)
of the nested shrinkages together with the signs of their arguments; `prox_at` is the map on that piece, in whatever precision
its inputs have, with autograd's derivative of the reference expression (sign() has none).  With the pieces taken from the
DEVICE's float32 u_k a float64 restatement of a whole call -- primal and tangent -- is a polynomial in its leaves, so device
results compare with it at the identical-support tolerances, gates that differ between arithmetics never entering.

Thresholds under a map: element (n, m, pix) takes t[k,0,m] + c[n,pix] * t[k,1,m], the product rounded before the sum
(`thresholds`: the reference's broadcast; in float32 the numbers the kernels form)."""
import torch

import csr_tangent_restate as R
from oracle import cdl_oracle as O


def thresholds(p, k, c):
    """(N,M,*code grid) from the (K,2,M,1,1) parameter and the (N,1,*code grid) map c = sigma / 255: product, then sum."""
    prod = c * p[k, 1:2]
    return p[k, :1] + prod


def pieces(u, zp, za, lam, g1, g2=None):
    """{gates, signs} of prox_CSR (za None) / prox_CSR_f2 at these numbers."""
    sign = torch.sign
    ST = O.soft_threshold
    if za is None:
        ls = lam * sign(zp)
        a = u - zp - ls
        tg = lam * g1
        m = ST(a, tg) + zp + ls
        return dict(G=(R.st_dx(a, tg), R.st_dx(m, lam)), sa=sign(a), sm=sign(m))
    ca = zp + lam * sign(zp) + lam * g2 * sign(zp - za)
    cb = za + lam * sign(za) + lam * g1 * sign(za - zp)
    a = u - ca
    inner = ST(a, g1 * lam)
    b = inner - cb + lam * g1 * sign(a)
    mid = ST(b, g2 * lam)
    m = mid + cb - lam * g1 * sign(a)
    return dict(G=(R.st_dx(a, g1 * lam), R.st_dx(b, g2 * lam), R.st_dx(m, lam)), sa=sign(a), sb=sign(b), sm=sign(m))


def prox_at(pc, u, zp, za, lam, g1, g2=None):
    """The map on the piece `pc`, in the precision of the inputs: ST(x, t) -> G (x - s t) with the gate G and the sign s
    prescribed.  The signs of the neighbour codes (and of their difference) are read off the inputs, which are exact."""
    sign = torch.sign
    dt = u.dtype
    zero = torch.zeros((), dtype=dt)
    if za is None:
        Ga, Gm = pc["G"]
        ls = lam * sign(zp)
        a = u - zp - ls
        inner = torch.where(Ga, a - pc["sa"].to(dt) * (lam * g1), zero)
        m = inner + zp + ls
        return torch.where(Gm, m - pc["sm"].to(dt) * lam, zero)
    Ga, Gb, Gm = pc["G"]
    sa = pc["sa"].to(dt)
    ca = zp + lam * sign(zp) + lam * g2 * sign(zp - za)
    cb = za + lam * sign(za) + lam * g1 * sign(za - zp)
    a = u - ca
    inner = torch.where(Ga, a - sa * (g1 * lam), zero)
    b = inner - cb + lam * g1 * sa
    mid = torch.where(Gb, b - pc["sb"].to(dt) * (g2 * lam), zero)
    m = mid + cb - lam * g1 * sa
    return torch.where(Gm, m - pc["sm"].to(dt) * lam, zero)


def call_at(pcs, A, B, t, g1, g2, y, v, zp, zdp, za, zda, c, *, s, P, mask=None):
    """One neighbour-branch call and its tangent on the pieces pcs[k] of iteration k: (xhat, xdot, z, zd).  A, B, t, g1, g2,
    zp, zdp, za, zda: float64 (leaves); c: the (N,1,*code grid) map, float64; g2 / za / zda None: the one-neighbour map."""
    K = len(A)
    pad = O._conv_pad(P, 2)
    yp, mean, pads, mask_p = O.preprocess(y, s, mask)
    vp, vmean, _, _ = O.preprocess(v, s, mask)
    z = None
    for k in range(K):
        if k == 0:
            u = O.analysis(yp, A[0], s, pad)
        else:
            r = O.synthesis(z, B[k], s, pad)
            if mask_p is not None:
                r = mask_p * r
            u = z - O.analysis(r - yp, A[k], s, pad)
        z = prox_at(pcs[k], u, zp, za, thresholds(t, k, c), thresholds(g1, k, c),
                    thresholds(g2, k, c) if za is not None else None)
    xhat = O.postprocess(O.synthesis(z, B[0], s, pad), mean, pads)
    xdp, zd = R.tangent_sweep(A, B, vp, mask_p, [pc["G"] for pc in pcs], zdp, zda if za is not None else None, s, pad)
    return xhat, O.postprocess(xdp, vmean, pads), z, zd


def run_pieces(A, B, t, g1, g2, y, zp, za, c, *, s, P, mask=None):
    """The pieces of every iteration of one call run in the arithmetic of the inputs (the CPU's own; the device tests take
    them from the device's u_k instead), and the call's (xhat, z)."""
    pad = O._conv_pad(P, 2)
    yp, mean, pads, mask_p = O.preprocess(y, s, mask)
    pcs, z = [], None
    for k in range(len(A)):
        if k == 0:
            u = O.analysis(yp, A[0], s, pad)
        else:
            r = O.synthesis(z, B[k], s, pad)
            if mask_p is not None:
                r = mask_p * r
            u = z - O.analysis(r - yp, A[k], s, pad)
        lam, a1 = thresholds(t, k, c), thresholds(g1, k, c)
        a2 = thresholds(g2, k, c) if za is not None else None
        pcs.append(pieces(u, zp, za, lam, a1, a2))
        z = O.prox_csr(u, zp, lam, a1) if za is None else O.prox_csr_f2(u, zp, za, lam, a1, a2)
    return pcs, O.postprocess(O.synthesis(z, B[0], s, pad), mean, pads), z
