"""Reference values for the tangent sweeps (net.jvp), from the oracle alone.

With the supports of z_1..z_K prescribed, O.ista is affine in y (shrink_on_support: [code != 0] (u - sign(code) tau)), so
    xdot_ref = ista(y + v; supports) - ista(y; supports)
is the directional derivative J(y) v exactly (no step size), and autograd of the oracle through that difference gives
the parameter gradients of any loss on (xhat, xdot).  Everything here runs in float64."""
import torch

from oracle import cdl_oracle as O


def to64(sd):
    return {k: v.detach().double() for k, v in sd.items()}


def _leaves(sd, K):
    keys = O.trainable(sd, K, False)
    work = dict(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work.update(leaves)
    return work, leaves


def tangent_and_grads(sd, y, v, supports, loss_fn, **kw):
    """(xhat, xdot, loss, grads) in float64: fixed-support difference and its autograd.  loss_fn(xhat, xdot) -> scalar.
    kw: K, P, s, sigma, adaptive, mask, ndim as O.ista takes them (tensors in any float dtype)."""
    K = kw["K"]
    d = lambda t: t.double() if torch.is_tensor(t) else t
    kw = {k: d(val) for k, val in kw.items()}
    work, leaves = _leaves(to64(sd), K)
    sup = [c.double() for c in supports]
    y, v = y.double(), v.double()
    xhat, _ = O.ista(work, y, supports=sup, **kw)
    xhat_v, _ = O.ista(work, y + v, supports=sup, **kw)
    xdot = xhat_v - xhat
    loss = loss_fn(xhat, xdot)
    loss.backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in leaves.items()}
    return xhat.detach(), xdot.detach(), float(loss.detach()), grads


def func_jvp_and_grads(sd, y, v, loss_fn, **kw):
    """The same quantities from torch.func.jvp of the oracle's own forward (its shrinkage, no prescribed support)."""
    K = kw["K"]
    d = lambda t: t.double() if torch.is_tensor(t) else t
    kw = {k: d(val) for k, val in kw.items()}
    work, leaves = _leaves(to64(sd), K)
    xhat, xdot = torch.func.jvp(lambda yy: O.ista(work, yy, **kw)[0], (y.double(),), (v.double(),))
    loss = loss_fn(xhat, xdot)
    loss.backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in leaves.items()}
    return xhat.detach(), xdot.detach(), float(loss.detach()), grads


def code_density(codes):
    """Fraction of non-zeros of every code."""
    return [float((c != 0).float().mean()) for c in codes]
