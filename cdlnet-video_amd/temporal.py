"""Frame-recurrent inference drivers of the CSR nets (reference analyzemri.py:87-182).

The reference's loops draw the noise themselves; here the caller hands over the already noisy (and, for
JDD, already masked) frames, so the same sequence of network calls can be replayed deterministically.
Every call runs through the HIP kernels (CDLNet_CSR / CDLNet_CSRf2 in net.py); these functions only
carry the sparse code of one frame into the call for its neighbour.

`csr_step` is one call of a CSR net on the surface that takes what `net(...)` refuses: a
noise-level map as sigma, and y / sigma that require grad.  The drivers go through it for the frames whose sigma is a map.
`csr_jvp_step` is the same surface for `jvp_recurrent`: the call with its tangent, sigma a map or not (section 38).
"""
import torch


def _sigma_at(sigma, t):
    return sigma[t] if isinstance(sigma, (list, tuple)) else sigma


def _is_sigma_map(sigma, y):
    """net._noise_scale's rule: a tensor with neither 1 nor N elements is a noise-level map."""
    return torch.is_tensor(sigma) and sigma.numel() not in (1, y.shape[0])


def _per_frame_sigma(sigma, frames):
    """A (T,1,Hc,Wc) tensor of per-frame maps is split into T maps that broadcast over each frame's batch.  With T equal
    to the batch size such a tensor could as well be one batch map for every frame: that is refused, a list says which."""
    T, y = len(frames), frames[0]
    if torch.is_tensor(sigma) and sigma.dim() == y.dim() and sigma.shape[0] == T and any(d > 1 for d in sigma.shape[2:]):
        if T == y.shape[0]:
            raise ValueError(f"sigma of shape {tuple(sigma.shape)} with {T} frames of batch size {T} is ambiguous: pass a list "
                             "with one map per frame (per-frame maps: [sigma[t:t+1] for t ..]; one batch map for all frames: "
                             "[sigma] * T)")
        return [sigma[t:t + 1] for t in range(T)]
    return sigma


def csr_step(net, y, z_prev=None, z_after=None, sigma=None, mask=1):
    """One call of a CDLNet_CSR / CDLNet_CSRf2 with banks and branch picked exactly as their forward picks them (second
    bank A2 / B2 / t2 for a CDLNet_CSR without a neighbour, g2 for the after-only branch of a CDLNet_CSRf2, D = B[0]
    everywhere), on the surface where sigma may be a noise-level map (any tensor that broadcasts to (N,1,*code grid); t, g1
    and g2 all follow it) and gradients reach y and sigma (in the shape it was given) as well as the parameters and the
    neighbour codes.  With a float or per-sample sigma and no data gradient asked for it returns the bits of net(...).
    The no-neighbour branch is the plain loop (loop.run); the others are functional.ista_csr."""
    from . import functional, loop
    from .net import CDLNet_CSR, CDLNet_CSRf2, _code_grid, _mask_tensor, _noise_scale
    functional._no_mask_gradient(mask)
    if not isinstance(net, (CDLNet_CSR, CDLNet_CSRf2)):
        raise TypeError(f"csr_step: expected a CDLNet_CSR or CDLNet_CSRf2, got {type(net).__name__}")
    if not y.is_cuda:
        raise RuntimeError(f"csr_step: input is on {y.device}. This package has no CPU compute path; the iterations run "
                           "in HIP kernels on a ROCm device.")
    sigma = sigma if net.adaptive else None
    one = isinstance(net, CDLNet_CSR)
    if one and z_after is not None:
        raise ValueError("csr_step: CDLNet_CSR has no z_after")
    A, B = net._filters()
    if z_prev is None and z_after is None:
        y = y.to(torch.float32)
        c = _noise_scale(sigma, True, y.shape[0], y.device, _code_grid(y.shape[2:], net.s))
        mask_t = _mask_tensor(mask, y)
        if one:
            A = [m.weight for m in net.A2]
            B = [net.B[0].weight] + [m.weight for m in net.B2][1:]      # B2[0] is never applied
        return tuple(loop.run(y, mask_t, c, net.t2 if one else net.t, A, B, net.s)[:2])
    if one:
        return functional.ista_csr(y, z_prev, None, sigma, mask, net.t, net.g, None, A, B, net.s)
    if z_prev is not None and z_after is not None:
        return functional.ista_csr(y, z_prev, z_after, sigma, mask, net.t, net.g1, net.g2, A, B, net.s)
    if z_prev is not None:
        return functional.ista_csr(y, z_prev, None, sigma, mask, net.t, net.g1, None, A, B, net.s)
    return functional.ista_csr(y, z_after, None, sigma, mask, net.t, net.g2, None, A, B, net.s)


def csr_jvp_step(net, y, v, z_prev=None, zdot_prev=None, z_after=None, zdot_after=None, sigma=None, mask=1):
    """(xhat, xdot, z, zdot): one call of a CDLNet_CSR / CDLNet_CSRf2 and its derivative along (v, zdot_prev, zdot_after) in
    (y, z_prev, z_after) at the primal's gates -- net.jvp_recurrent on the surface where sigma may be a noise-level map (any
    tensor that broadcasts to (N,1,*code grid); t, g1 and g2 all follow it, and the gates are the ones csr_step's primal
    takes).  Banks and branch are picked as csr_step / jvp_recurrent pick them.  All four outputs are
    differentiable in the parameters and in the neighbour codes and tangents; gradients with respect to y, v, sigma or mask
    are not produced.  With a float or per-sample sigma it returns the bits of net.jvp_recurrent(...)."""
    from . import functional
    from .net import CDLNet_CSR, CDLNet_CSRf2, _code_grid, _mask_tensor, _noise_scale
    functional._no_mask_gradient(mask)
    if not isinstance(net, (CDLNet_CSR, CDLNet_CSRf2)):
        raise TypeError(f"csr_jvp_step: expected a CDLNet_CSR or CDLNet_CSRf2, got {type(net).__name__}")
    if isinstance(net, CDLNet_CSR) and (z_after is not None or zdot_after is not None):
        raise ValueError("csr_jvp_step: CDLNet_CSR has no z_after")
    # jvp_recurrent's own checks and branch pick (net._check_tangent, net._jvp_branch); only forward's refusal of a map is
    # not taken over
    net._check_tangent(y, v, sigma, mask, (("prev", z_prev, zdot_prev), ("after", z_after, zdot_after)), who="csr_jvp_step")
    y, v = y.to(torch.float32), v.to(torch.float32)
    c = _noise_scale(sigma, net.adaptive, y.shape[0], y.device, _code_grid(y.shape[2:], net.s))
    return net._jvp_branch(y, v, _mask_tensor(mask, y), c, z_prev, zdot_prev, z_after, zdot_after)


def _call(net, y, codes, sigma, mask):
    """net(y, *codes, sigma, mask=mask) -- through csr_step when this frame's sigma is a noise-level map."""
    if _is_sigma_map(sigma, y):
        return csr_step(net, y, *codes, sigma=sigma, mask=mask)
    return net(y, *codes, sigma, mask=mask)


def _mask_at(mask, t):
    return mask[t] if isinstance(mask, (list, tuple)) else mask


@torch.no_grad()
def csr_inference_loop(net, frames, sigma=None, mask=1, bootstrap_curr=None):
    """analyzemri.py:87-156 with a CDLNet_CSR: frame 0 alone (second bank), frame 1 given z_0, frame 0
    again given z_1; then every frame t >= 1 given the running code.  `frames` is a sequence of
    (B, C, H, W) noisy frames; `sigma` / `mask` one value or one per frame (noise-level maps: a list, or a (T,1,Hc,Wc)
    tensor with one map per frame; those frames go through csr_step).  `bootstrap_curr` is the
    realisation of frame 1 used for the bootstrap call (the reference draws a second, independent one
    for the loop; default: the same frame).  Returns the list of denoised frames."""
    if len(frames) < 2:
        raise ValueError("the recurrent loop needs at least two frames")
    sigma = _per_frame_sigma(sigma, frames)
    s0, s1 = _sigma_at(sigma, 0), _sigma_at(sigma, 1)
    m0, m1 = _mask_at(mask, 0), _mask_at(mask, 1)
    _, z_prev = _call(net, frames[0], (None,), s0, m0)
    _, z_curr = _call(net, frames[1] if bootstrap_curr is None else bootstrap_curr, (z_prev,), s1, m1)
    first, z_prev = _call(net, frames[0], (z_curr,), s0, m0)
    results = [first]
    for t in range(1, len(frames)):
        xhat, z_prev = _call(net, frames[t], (z_prev,), _sigma_at(sigma, t), _mask_at(mask, t))
        results.append(xhat)
    return results


@torch.no_grad()
def csr_inference_v2(net, frames, sigma=None, mask=1):
    """analyzemri.py:162-182 with a CDLNet_CSRf2: a causal pass that records every frame's code
    (frame t given z_{t-1}), then a second pass in which frame t sees the recorded codes on both
    sides of it exactly as the reference indexes them: z_prev_list[t] (the code of frame t-1, None for
    t = 0) as `z_prev` and z_prev_list[t+1] (frame t's own first-pass code) as `z_after`."""
    T = len(frames)
    sigma = _per_frame_sigma(sigma, frames)
    codes = [None] * (T + 2)
    for t in range(T):
        _, codes[t + 1] = _call(net, frames[t], (codes[t], None), _sigma_at(sigma, t), _mask_at(mask, t))
    # second pass: frame t only needs recorded codes, so frames 1..T-1 (both neighbours given) go through the
    # network as ONE batch -- the samples of a batch are independent in every kernel, so the result per frame is
    # what the reference's frame-by-frame loop computes; frame 0 (no previous code) takes the other branch alone
    out = [_call(net, frames[0], (None, codes[1]), _sigma_at(sigma, 0), _mask_at(mask, 0))[0]]
    if T > 1:
        same_sigma = not isinstance(sigma, (list, tuple))
        same_mask = not isinstance(mask, (list, tuple))
        if same_sigma and same_mask and not torch.is_tensor(sigma) and not torch.is_tensor(mask):
            B = frames[0].shape[0]
            xb, _ = net(torch.cat(list(frames[1:])), torch.cat(codes[1:T]), torch.cat(codes[2:T + 1]), sigma, mask=mask)
            out.extend(xb[i * B:(i + 1) * B] for i in range(T - 1))
        else:
            out.extend(_call(net, frames[t], (codes[t], codes[t + 1]), _sigma_at(sigma, t), _mask_at(mask, t))[0]
                       for t in range(1, T))
    return out
