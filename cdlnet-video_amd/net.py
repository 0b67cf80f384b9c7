"""Drop-in modules for the reference's `model/net.py` hot path.

Same constructor signatures, attribute names (`A`, `B`, `D`, `t`, `g`, `K`, `M`, `P`, `s`, `t0`,
`adaptive`), `state_dict` keys and `forward(y, sigma=None, mask=1) -> (xhat, z)` contract as
`CDLNet` (net.py:16-104), `CDLNetVideo` (net.py:121-227) and `GDLNet` (net.py:569-687); the K
iterations run in hand-written HIP kernels (libcdlnet_hip.so) instead of ATen convolutions.

The filter containers subclass `nn.Conv{2,3}d` / `nn.ConvTranspose{2,3}d` purely as parameter
holders: identical `weight` shapes and state_dict keys, and -- because their default
initialisers draw from the global RNG exactly like the reference's -- `torch.manual_seed(s);
CDLNet(...)` yields the reference's weights bit for bit.  Their `forward` is overridden to
call the HIP operators; no ATen convolution runs on the device.
"""
import sys

import numpy as np
import torch
import torch.nn as nn

from . import functional, loop, ops
from .gabor import ConvAdjoint2dGabor, filter_banks, gabor_kernel_cpu
from .solvers import gram_operator, power_method


def ST(x, t):
    """Shrinkage-thresholding sign(x)*relu(|x|-t) (net.py:11-14) on the device.

    Stand-alone form for callers of the reference's helper (t a number or broadcastable to x),
    differentiable in x and t (functional.shrink); inside the nets it is fused into the analysis
    kernel's epilogue.
    """
    return functional.shrink(x, t)


# ------------------------------------------------------------------------------------------ banks
class _Analysis2d(nn.Conv2d):
    def forward(self, x):
        return functional.analysis(x, self.weight, self.stride[0])


class _Synthesis2d(nn.ConvTranspose2d):
    def forward(self, z):
        return functional.synthesis(z, self.weight, self.stride[0])


class _Analysis3d(nn.Conv3d):
    def forward(self, x):
        return functional.analysis(x, self.weight, self.stride[0])


class _Synthesis3d(nn.ConvTranspose3d):
    def forward(self, z):
        return functional.synthesis(z, self.weight, self.stride[0])


def _code_grid(spatial, s):
    """Spatial extent of the codes of an image of extent `spatial`: the stride-padded extent over the stride."""
    return tuple(-(-int(d) // int(s)) for d in spatial)


def _noise_scale(sigma, adaptive, N, device, code_spatial):
    """c = sigma/255 (net.py:82): None for c = 0, an (N,) tensor (one level per sample), or -- a noise-level MAP -- a
    dense (N, 1, *code_spatial) tensor.

    A float, and a tensor with 1 or N elements whatever its shape, is one level per sample.  Every other tensor is a map
    and must broadcast to (N, 1, *code_spatial) as it does against a code tensor in the reference: one level per frame
    (N,1,D,1,1), a full map (N,1,Hc,Wc) / (N,1,Dc,Hc,Wc), or anything between; it is expanded on the host (it is 1/M of
    a code tensor).  The one ambiguity of the first rule: a (1,1,H,W) map with H*W == N is read as N per-sample levels --
    expand it to (N,1,H,W) to have it read as a map.

    Under loop.set_frame_tier("fused") a map of a clip with extent 1 on both in-plane axes -- (N,1,D,1,1), (1,1,D,1,1),
    (D,1,1): one level per frame -- comes back as a contiguous (N,1,D,1,1) tensor: the form the fused generic tier reads as a
    threshold row per (sample, frame); a sweep that takes another route expands it itself (loop._forward_sweep)."""
    if sigma is None or not adaptive:
        return None
    if torch.is_tensor(sigma):
        if sigma.numel() in (1, N):
            c = sigma.to(device=device, dtype=torch.float32).reshape(-1) / 255.0
            if c.numel() == 1:
                c = c.expand(N)
            return c.contiguous()
        want = (N, 1) + tuple(code_spatial)
        if sigma.dim() > len(want):
            raise ValueError(f"sigma of shape {tuple(sigma.shape)} does not broadcast to the code grid {want}")
        shape = (1,) * (len(want) - sigma.dim()) + tuple(sigma.shape)
        if shape[1] != 1:
            raise ValueError(f"sigma of shape {tuple(sigma.shape)} varies over the channel axis: a noise-level map holds "
                             f"one level per code pixel, (N, 1, *code grid) = {want}")
        if any(a not in (1, b) for a, b in zip(shape, want)):
            raise ValueError(f"sigma of shape {tuple(sigma.shape)} does not broadcast to the code grid {want} "
                             "(the stride-padded image extent over the stride; utils.sigma_to_code_grid maps an "
                             "image-resolution map onto it)")
        c = sigma.to(device=device, dtype=torch.float32).reshape(shape) / 255.0
        if loop.FRAME_TIER == "fused" and len(want) == 5 and shape[3:] == (1, 1) and want[3:] != (1, 1):
            return c.expand(want[:3] + (1, 1)).contiguous()        # one level per frame: the sweep expands it where it must
        return c.expand(want).contiguous()
    return torch.full((N,), float(sigma) / 255.0, device=device, dtype=torch.float32)


def _is_map(c):
    return c is not None and c.dim() > 1


def _mask_tensor(mask, y):
    if torch.is_tensor(mask):
        return torch.broadcast_to(mask.to(dtype=torch.float32), y.shape).contiguous()
    if mask is None or mask == 1:
        return None
    raise ValueError("mask must be 1 (no mask) or a tensor shaped like y")


class _ISTANet(nn.Module):
    """Shared forward / generator plumbing."""

    def _filters(self):
        A = [m.weight for m in self.A]
        B = [m.weight for m in self.B]
        return A, B

    def _run(self, y, sigma, mask, all_codes):
        if not y.is_cuda:
            raise RuntimeError(
                f"{type(self).__name__}.forward: input is on {y.device}. This package has no CPU "
                "compute path; the iterations run in HIP kernels on a ROCm device.")
        y = y.to(torch.float32)
        A, B = self._filters()
        c = _noise_scale(sigma, self.adaptive, y.shape[0], y.device, _code_grid(y.shape[2:], self.s))
        return loop.run(y, _mask_tensor(mask, y), c, self.t, A, B, self.s, all_codes)

    def forward(self, y, sigma=None, mask=1):
        """LISTA + D with noise-adaptive thresholds: returns (xhat, z_K)."""
        xhat, z = self._run(y, sigma, mask, False)
        return xhat, z

    def _jvp_refusal(self):
        """Why this net has no tangent sweep (None: it has one)."""
        return None

    def jvp(self, y, v, sigma=None, mask=1):
        """(xhat, xdot): the forward pass and its directional derivative J(y) v in the observation, at the supports of
        the primal codes (where the net is affine in y: the derivative autograd of the reference gives, without a step
        size).  xhat is what forward returns; both are differentiable in the parameters -- `t` through xhat alone (the
        thresholds do not appear in the tangent recursion).  v is a constant direction shaped like
        y; gradients with respect to y, v, sigma or mask are not produced."""
        why = self._jvp_refusal()
        if why is not None:
            raise NotImplementedError(f"cdlnet_video_amd: {type(self).__name__}.jvp: {why}")
        if not torch.is_tensor(v):
            raise TypeError("jvp: v must be a tensor shaped like y")
        for name, t in (("y", y), ("v", v)):
            if not t.is_cuda:
                raise RuntimeError(
                    f"{type(self).__name__}.jvp: {name} is on {t.device}. This package has no CPU "
                    "compute path; the iterations run in HIP kernels on a ROCm device.")
        if tuple(v.shape) != tuple(y.shape):
            raise ValueError(f"jvp: v has shape {tuple(v.shape)}, y has {tuple(y.shape)}")
        for name, t in (("v", v), ("y", y), ("sigma", sigma), ("mask", mask)):
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(f"cdlnet_video_amd: jvp: `{name}` requires grad; the tangent sweep returns "
                                          "parameter gradients only (detach() it)")
        if loop.CODE_LAYOUT == "blocked_bf16":
            raise NotImplementedError("cdlnet_video_amd: jvp with set_code_layout('blocked_bf16') is not implemented "
                                      "(tangent codes are stored in fp32)")
        y, v = y.to(torch.float32), v.to(torch.float32)
        A, B = self._filters()
        c = _noise_scale(sigma, self.adaptive, y.shape[0], y.device, _code_grid(y.shape[2:], self.s))
        return loop.run_tangent(y, v, _mask_tensor(mask, y), c, self.t, A, B, self.s)

    def forward_generator(self, y, sigma=None, mask=1):
        """Yields z_1..z_K, then xhat (net.py:94-104, 214-227)."""
        outs = self._run(y, sigma, mask, True)
        xhat, zK, earlier = outs[0], outs[1], outs[2:]
        for z in earlier:
            yield z
        yield zK
        yield xhat


# ------------------------------------------------------------------------------------------ 2-D
class CDLNet(_ISTANet):
    """Convolutional Dictionary Learning Network (2-D; JDD = C=3 + Bayer mask)."""

    def __init__(self, K=3, M=64, P=7, s=1, C=1, t0=0, adaptive=False, init=True):
        super().__init__()
        if P % 2 == 0:
            raise ValueError("P must be odd (the reference's conv / conv-transpose pair needs it)")
        self.A = nn.ModuleList([_Analysis2d(C, M, P, stride=s, padding=(P - 1) // 2, bias=False)
                                for _ in range(K)])
        self.B = nn.ModuleList([_Synthesis2d(M, C, P, stride=s, padding=(P - 1) // 2,
                                             output_padding=s - 1, bias=False) for _ in range(K)])
        self.D = self.B[0]
        self.t = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self.g = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))       # unused, kept for checkpoints
        W = torch.randn(M, C, P, P)
        for k in range(K):
            self.A[k].weight.data = W.clone()
            self.B[k].weight.data = W.clone()
        if init:
            print("Running power-method on initial dictionary...")
            with torch.no_grad():
                op = gram_operator(self.A[0].weight, self.D.weight, s, (P - 1) // 2)
                L = power_method(op, torch.rand(1, C, 128, 128), num_iter=200, verbose=False)[0]
            print(f"Done. L={L:.3e}.")
            if L < 0:
                print("STOP: something is very very wrong...")
                sys.exit()
            for k in range(K):
                self.A[k].weight.data /= np.sqrt(L)
                self.B[k].weight.data /= np.sqrt(L)
        self.K, self.M, self.P, self.s, self.t0, self.adaptive = K, M, P, s, t0, adaptive

    @torch.no_grad()
    def project(self):
        """l2-ball projection of every filter, R+ projection of the thresholds (net.py:66-74)."""
        self.t.clamp_(0.0)
        ops.project_filter_banks_([m.weight.data for m in self.A] + [m.weight.data for m in self.B])

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Accepts upstream CDLNet-OJSP checkpoints that predate the unused `g` parameter."""
        if "g" not in state_dict and "t" in state_dict:
            state_dict = dict(state_dict)
            state_dict["g"] = self.g.detach().clone()
        return super().load_state_dict(state_dict, strict=strict, **kw)


# ------------------------------------------------------------------------------------------ CSR
def prox_CSR(u, z_prev, lambd, gamma):
    """The reference's helper (net.py:229-242) on the device; lambd, gamma numbers or broadcastable to u; differentiable
    in every tensor argument (functional.prox_csr)."""
    return functional.prox_csr(u, z_prev, lambd, gamma)


def prox_CSR_f2(u, z_prev, z_after, lambd, gamma1, gamma2):
    """The reference's helper (net.py:244-262) on the device (functional.prox_csr_f2)."""
    return functional.prox_csr_f2(u, z_prev, z_after, lambd, gamma1, gamma2)


class _CSRBase(_ISTANet):
    """Constructor plumbing shared by the two CSR nets (2-D only, like the reference's)."""

    def _banks(self, K, M, P, s, C):
        A = nn.ModuleList([_Analysis2d(C, M, P, stride=s, padding=(P - 1) // 2, bias=False) for _ in range(K)])
        B = nn.ModuleList([_Synthesis2d(M, C, P, stride=s, padding=(P - 1) // 2, output_padding=s - 1,
                                        bias=False) for _ in range(K)])
        return A, B

    def _spectral_init(self, K, M, P, s, C, init):
        W = torch.randn(M, C, P, P)
        for k in range(K):
            self.A[k].weight.data = W.clone()
            self.B[k].weight.data = W.clone()
        if init:
            print("Running power-method on initial dictionary...")
            with torch.no_grad():
                op = gram_operator(self.A[0].weight, self.D.weight, s, (P - 1) // 2)
                L = power_method(op, torch.rand(1, C, 128, 128), num_iter=200, verbose=False)[0]
            print(f"Done. L={L:.3e}.")
            if L < 0:
                print("STOP: something is very very wrong...")
                sys.exit()
            for k in range(K):
                self.A[k].weight.data /= np.sqrt(L)
                self.B[k].weight.data /= np.sqrt(L)

    @torch.no_grad()
    def project(self):
        """net.py:419-424 / 518-523: only `t`, `A`, `B` are projected (not t2, g*, A2, B2)."""
        self.t.clamp_(0.0)
        ops.project_filter_banks_([m.weight.data for m in self.A] + [m.weight.data for m in self.B])

    def _jvp_refusal(self):
        return ("the CSR nets take neighbour codes, which jvp(y, v) cannot carry; their tangent sweep is "
                "jvp_recurrent(y, v, z_prev, zdot_prev, ...)")

    def _check_tangent(self, y, v, sigma, mask, pairs, who=None):
        """Argument checks of a tangent call, jvp's and each neighbour tangent with its code: jvp_recurrent's, and those of
        temporal.csr_jvp_step (which names itself in `who`)."""
        fn = who or "jvp_recurrent"
        qual = who or f"{type(self).__name__}.jvp_recurrent"
        if not torch.is_tensor(v):
            raise TypeError(f"{fn}: v must be a tensor shaped like y")
        for label, code, dot in pairs:
            if dot is not None and code is None:
                raise ValueError(f"{fn}: zdot_{label} given without z_{label} (a tangent belongs to a code)")
        for label, x in (("y", y), ("v", v)):
            if not x.is_cuda:
                raise RuntimeError(
                    f"{qual}: {label} is on {x.device}. This package has no CPU "
                    "compute path; the iterations run in HIP kernels on a ROCm device.")
        if tuple(v.shape) != tuple(y.shape):
            raise ValueError(f"{fn}: v has shape {tuple(v.shape)}, y has {tuple(y.shape)}")
        for label, x in (("v", v), ("y", y), ("sigma", sigma), ("mask", mask)):
            if torch.is_tensor(x) and x.requires_grad:
                raise NotImplementedError(f"cdlnet_video_amd: {qual}: `{label}` requires grad; the tangent sweep "
                                          "returns parameter and neighbour-code gradients only (detach() it)")
        if loop.CODE_LAYOUT == "blocked_bf16":
            raise NotImplementedError(f"cdlnet_video_amd: {fn} with set_code_layout('blocked_bf16') is not "
                                      "implemented (tangent codes are stored in fp32)")

    def _prep_tangent(self, y, v, sigma, mask, pairs):
        """Argument checks of jvp_recurrent: the tangent's (_check_tangent) and forward's (_prep)."""
        self._check_tangent(y, v, sigma, mask, pairs)
        y, mask_t, c = self._prep(y, sigma, mask)
        return y, v.to(torch.float32), mask_t, c

    def _jvp_branch(self, y, v, mask_t, c, z_prev, zdot_prev, z_after=None, zdot_after=None):
        """The tangent call of the branch forward takes (_tangent_branch of the variant): jvp_recurrent after its checks, and
        temporal.csr_jvp_step after its own (c may then be a noise-level map)."""
        t, A, B, nb = self._tangent_branch(z_prev, zdot_prev, z_after, zdot_after)
        if nb is None:
            return loop.run_tangent(y, v, mask_t, c, t, A, B, self.s, codes=True)
        zp, zdp, za, zda, g1, g2 = nb
        return loop.run_csr_tangent(y, v, mask_t, c, zp, zdp, za, zda, t, g1, g2, A, B, self.s)

    def _prep(self, y, sigma, mask):
        if not y.is_cuda:
            raise RuntimeError(
                f"{type(self).__name__}.forward: input is on {y.device}. This package has no CPU "
                "compute path; the iterations run in HIP kernels on a ROCm device.")
        if torch.is_grad_enabled() and (y.requires_grad or (torch.is_tensor(sigma) and sigma.requires_grad)):
            # the CSR sweeps (TemporalISTA) return parameter and neighbour-code gradients only; the no-neighbour
            # branch runs UnrolledISTA, which could, but the variant's surface stays one contract
            raise NotImplementedError(f"cdlnet_video_amd: {type(self).__name__}: gradients with respect to y / sigma "
                                      "are not implemented; detach() them")
        y = y.to(torch.float32)
        c = _noise_scale(sigma, self.adaptive, y.shape[0], y.device, _code_grid(y.shape[2:], self.s))
        if _is_map(c):
            # the three threshold families (t, g1, g2) would each follow the map; on every branch, the no-neighbour one
            # included, so that the variant keeps one contract
            raise NotImplementedError(f"cdlnet_video_amd: {type(self).__name__}: a noise-level map (sigma of shape "
                                      f"{tuple(sigma.shape)}) is not implemented for the CSR nets; pass one level per sample")
        return y, _mask_tensor(mask, y), c


class CDLNet_CSR(_CSRBase):
    """CDLNet with the frame-recurrent CSR prior (net.py:363-463): without a neighbour code the plain
    loop on the second bank (A2, B2, t2; the final synthesis is still D = B[0]); with `z_prev` the
    first bank and prox_CSR(., z_prev, t, g)."""

    def __init__(self, K=3, M=64, P=7, s=1, C=1, t0=0, adaptive=False, init=True):
        super().__init__()
        if P % 2 == 0:
            raise ValueError("P must be odd (the reference's conv / conv-transpose pair needs it)")
        self.A, self.B = self._banks(K, M, P, s, C)
        self.A2, self.B2 = self._banks(K, M, P, s, C)
        self.D = self.B[0]
        self.t = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self.t2 = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self.g = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self._spectral_init(K, M, P, s, C, init)
        self.K, self.M, self.P, self.s, self.t0, self.adaptive = K, M, P, s, t0, adaptive

    def forward(self, y, z_prev=None, sigma=None, mask=1):
        y, mask_t, c = self._prep(y, sigma, mask)
        if z_prev is None:
            A = [m.weight for m in self.A2]
            B = [self.B[0].weight] + [m.weight for m in self.B2][1:]      # B2[0] is never applied
            xhat, z = loop.run(y, mask_t, c, self.t2, A, B, self.s)[:2]
            return xhat, z
        A, B = self._filters()
        return loop.run_csr(y, mask_t, c, z_prev, None, self.t, self.g, None, A, B, self.s)

    def jvp_recurrent(self, y, v, z_prev=None, zdot_prev=None, sigma=None, mask=1):
        """(xhat, xdot, z, zdot): forward(y, z_prev, sigma, mask) and the derivative of (xhat, z) along (v, zdot_prev) in
        (y, z_prev), at the gates of the primal's proximal maps (where the net is affine in both: the derivative autograd of
        the reference gives).  zdot_prev None: a constant neighbour.  All four are differentiable in
        the parameters and in z_prev / zdot_prev, so the calls of a clip chain; the thresholds get their gradient through
        (xhat, z) alone.  Gradients with respect to y, v, sigma or mask are not produced."""
        y, v, mask_t, c = self._prep_tangent(y, v, sigma, mask, (("prev", z_prev, zdot_prev),))
        return self._jvp_branch(y, v, mask_t, c, z_prev, zdot_prev)

    def _tangent_branch(self, z_prev, zdot_prev, z_after=None, zdot_after=None):
        """(t, A, B, neighbours): without a neighbour the plain loop on the second bank (neighbours None; B2[0] is never
        applied), else (z_prev, zdot_prev, None, None, g, None) on the first."""
        if z_after is not None or zdot_after is not None:
            raise ValueError("CDLNet_CSR has no z_after")
        if z_prev is None:
            A = [m.weight for m in self.A2]
            B = [self.B[0].weight] + [m.weight for m in self.B2][1:]
            return self.t2, A, B, None
        A, B = self._filters()
        return self.t, A, B, (z_prev, zdot_prev, None, None, self.g, None)


class CDLNet_CSRf2(_CSRBase):
    """CDLNet with previous- and next-frame CSR priors (net.py:464-568): one bank, thresholds t, g1, g2;
    the branch is chosen by which neighbour codes are given."""

    def __init__(self, K=3, M=64, P=7, s=1, C=1, t0=0, adaptive=False, init=True):
        super().__init__()
        if P % 2 == 0:
            raise ValueError("P must be odd (the reference's conv / conv-transpose pair needs it)")
        self.A, self.B = self._banks(K, M, P, s, C)
        self.D = self.B[0]
        self.t = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self.g1 = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self.g2 = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        self._spectral_init(K, M, P, s, C, init)
        self.K, self.M, self.P, self.s, self.t0, self.adaptive = K, M, P, s, t0, adaptive

    def forward(self, y, z_prev=None, z_after=None, sigma=None, mask=1):
        y, mask_t, c = self._prep(y, sigma, mask)
        A, B = self._filters()
        if z_prev is None and z_after is None:
            xhat, z = loop.run(y, mask_t, c, self.t, A, B, self.s)[:2]
            return xhat, z
        if z_prev is not None and z_after is not None:
            return loop.run_csr(y, mask_t, c, z_prev, z_after, self.t, self.g1, self.g2, A, B, self.s)
        if z_prev is not None:
            return loop.run_csr(y, mask_t, c, z_prev, None, self.t, self.g1, None, A, B, self.s)
        return loop.run_csr(y, mask_t, c, z_after, None, self.t, self.g2, None, A, B, self.s)

    def jvp_recurrent(self, y, v, z_prev=None, zdot_prev=None, z_after=None, zdot_after=None, sigma=None, mask=1):
        """(xhat, xdot, z, zdot): forward(y, z_prev, z_after, sigma, mask) and the derivative of (xhat, z) along
        (v, zdot_prev, zdot_after) in (y, z_prev, z_after) at the primal's gates; the branch is forward's.  See
        CDLNet_CSR.jvp_recurrent."""
        y, v, mask_t, c = self._prep_tangent(y, v, sigma, mask, (("prev", z_prev, zdot_prev), ("after", z_after, zdot_after)))
        return self._jvp_branch(y, v, mask_t, c, z_prev, zdot_prev, z_after, zdot_after)

    def _tangent_branch(self, z_prev, zdot_prev, z_after=None, zdot_after=None):
        """(t, A, B, neighbours): forward's four branches -- no neighbour (None), both (g1, g2), the previous one (g1), or the
        next one alone, which takes the one-neighbour map around z_after with g2."""
        A, B = self._filters()
        if z_prev is None and z_after is None:
            return self.t, A, B, None
        if z_prev is not None and z_after is not None:
            return self.t, A, B, (z_prev, zdot_prev, z_after, zdot_after, self.g1, self.g2)
        if z_prev is not None:
            return self.t, A, B, (z_prev, zdot_prev, None, None, self.g1, None)
        return self.t, A, B, (z_after, zdot_after, None, None, self.g2, None)


# ------------------------------------------------------------------------------------------ 3-D
class _DenseConv3d(nn.Conv3d):
    """Parameter holder of a ResidualBlock convolution; stand-alone forward = the HIP analysis operator."""

    def forward(self, x):
        g = ops.residual_geometry(x, self.weight)
        return ops.analysis(g, x, self.weight.detach())


class ResidualBlock(nn.Module):
    """net.py:105-120: relu(conv2(relu(conv1 x)) + x) with two bias-free 3x3x3 convolutions, on the HIP
    operators (forward and backward: loop.ResidualBlockFn).  Same constructor and state_dict keys."""

    def __init__(self, in_channels, out_channels, kernel_size=(3, 3, 3), stride=1, padding=1):
        super().__init__()
        ks = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
        pd = (padding,) * 3 if isinstance(padding, int) else tuple(padding)
        if in_channels != out_channels or stride != 1 or any(k % 2 == 0 for k in ks) or pd != tuple(k // 2 for k in ks):
            raise ValueError("ResidualBlock: the skip connection needs in == out channels, stride 1 and "
                             "'same' padding (the only form the reference builds, net.py:150)")
        self.conv1 = _DenseConv3d(in_channels, out_channels, ks, stride=1, padding=pd, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _DenseConv3d(out_channels, out_channels, ks, stride=1, padding=pd, bias=False)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("ResidualBlock.forward: this package has no CPU compute path")
        return loop.ResidualBlockFn.apply(x.to(torch.float32), self.conv1.weight, self.conv2.weight)


class CDLNetVideo(_ISTANet):
    """3-D (video / volume) twin; `P` is (kD, kH, kW) or an int (cube)."""

    def __init__(self, K=3, M=64, P=(7, 7, 5), s=1, C=1, t0=0, adaptive=False, depth=3, init=True,
                 residual=False):
        super().__init__()
        if isinstance(P, int):
            P = (P, P, P)
        P = tuple(int(p) for p in P)
        if any(p % 2 == 0 for p in P):
            raise ValueError("every filter extent must be odd")
        pad = tuple(p // 2 for p in P)
        self.A = nn.ModuleList([_Analysis3d(C, M, P, stride=s, padding=pad, bias=False)
                                for _ in range(K)])
        self.B = nn.ModuleList([_Synthesis3d(M, C, P, stride=s, padding=pad, output_padding=s - 1,
                                             bias=False) for _ in range(K)])
        self.D = self.B[0]
        self.t = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1, 1))
        self.residual = bool(residual)
        if self.residual:                       # created here, as the reference does: same RNG draws
            self.residual_blocks = nn.ModuleList([ResidualBlock(M, M) for _ in range(K)])
        W = torch.randn(M, C, *P)
        for k in range(K):
            self.A[k].weight.data = W.clone()
            self.B[k].weight.data = W.clone()
        if init:
            print("Running power-method on initial dictionary...")
            with torch.no_grad():
                op = gram_operator(self.A[0].weight, self.D.weight, s, pad)
                L = power_method(op, torch.rand(1, C, depth, 128, 128), num_iter=200, verbose=False)[0]
            print(f"Done. L={L:.3e}.")
            if L < 0:
                print("STOP: something is very very wrong...")
                sys.exit()
            for k in range(K):
                self.A[k].weight.data /= np.sqrt(L)
                self.B[k].weight.data /= np.sqrt(L)
        self.K, self.M, self.P, self.s, self.t0, self.adaptive = K, M, P, s, t0, adaptive

    def _run(self, y, sigma, mask, all_codes):
        if not self.residual:
            return super()._run(y, sigma, mask, all_codes)
        if not y.is_cuda:
            raise RuntimeError(f"CDLNetVideo.forward: input is on {y.device}; this package has no CPU compute path")
        y = y.to(torch.float32)
        A, B = self._filters()
        c = _noise_scale(sigma, self.adaptive, y.shape[0], y.device, _code_grid(y.shape[2:], self.s))
        blocks = [(b.conv1.weight, b.conv2.weight) for b in self.residual_blocks]
        return loop.run_residual(y, _mask_tensor(mask, y), c, self.t, A, B, self.s, blocks, all_codes)

    def _jvp_refusal(self):
        return "residual=True (a ResidualBlock after every iteration) has no tangent sweep" if self.residual else None

    def forward_generator(self, y, sigma=None, mask=1):
        """net.py:214-227; with residual blocks the yielded codes are the ST outputs (before the block)."""
        if not self.residual:
            yield from super().forward_generator(y, sigma, mask)
            return
        outs = self._run(y, sigma, mask, True)
        yield from outs[2:]
        yield outs[0]

    @torch.no_grad()
    def project(self):
        """net.py:184-190.  (The reference's own call raises on torch >= 2: `torch.norm` with a
        3-axis `dim`; this does what it evidently means -- the l2 norm over the filter volume.)"""
        self.t.clamp_(0.0)
        ops.project_filter_banks_([m.weight.data for m in self.A] + [m.weight.data for m in self.B])


# ------------------------------------------------------------------------------------------ Gabor
class GDLNet(_ISTANet):
    """Gabor Dictionary Learning Network: same loop, filters synthesised from Gabor parameters."""

    def __init__(self, K=3, M=64, P=7, s=1, C=1, t0=0, order=1, adaptive=False, shared="", init=True):
        super().__init__()
        self.A = nn.ModuleList([ConvAdjoint2dGabor(M, C, P, stride=s, order=order) for _ in range(K)])
        self.B = nn.ModuleList([ConvAdjoint2dGabor(M, C, P, stride=s, order=order) for _ in range(K)])
        self.D = self.B[0]
        self.t = nn.Parameter(t0 * torch.ones(K, 2, M, 1, 1))
        alpha = torch.randn(order, M, C, 1, 1)
        a = torch.randn(order, M, C, 2)
        w0 = torch.randn(order, M, C, 2)
        psi = torch.randn(order, M, C)
        for k in range(K):
            for bank in (self.A[k], self.B[k]):
                bank.alpha.data = alpha.clone()
                bank.a.data = a.clone()
                bank.w0.data = w0.clone()
                bank.psi.data = psi.clone()
            if k > 0:                                   # parameter sharing by aliasing (net.py:607-622)
                if "alpha" in shared:
                    self.A[k].alpha = self.A[0].alpha
                    if k > 1:                           # never share the scale with D = B[0]
                        self.B[k].alpha = self.B[1].alpha
                if "a_" in shared:
                    self.A[k].a, self.B[k].a = self.A[0].a, self.B[0].a
                if "w0" in shared:
                    self.A[k].w0, self.B[k].w0 = self.A[0].w0, self.B[0].w0
                if "psi" in shared:
                    self.A[k].psi, self.B[k].psi = self.A[0].psi, self.B[0].psi
        if init:
            print("Running power-method on initial dictionary...")
            with torch.no_grad():
                wa = gabor_kernel_cpu(self.A[0].alpha, self.A[0].a, self.A[0].w0, self.A[0].psi, P, True)
                wd = gabor_kernel_cpu(self.D.alpha, self.D.a, self.D.w0, self.D.psi, P, False)
                L = power_method(gram_operator(wa, wd, s, (P - 1) // 2), torch.rand(1, C, 128, 128),
                                 num_iter=200, verbose=False)[0]
            print(f"Done. L={L:.3e}.")
            if L < 0:
                print("STOP: something is very very wrong...")
                sys.exit()
            for k in range(K):                          # net.py:637-642
                self.A[k].alpha.data /= np.sqrt(L)
                self.B[k].alpha.data /= np.sqrt(L)
                if "alpha" in shared:
                    self.B[1].alpha.data /= np.sqrt(L)
                    break
        self.K, self.M, self.P, self.s, self.t0 = K, M, P, s, t0
        self.order, self.adaptive = order, adaptive

    def _filters(self):
        """All 2K banks from one launch and one autograd node (gabor.filter_banks); same values as the per-module
        `get_filter` calls of the reference (net.py:665-671)."""
        K = len(self.A)
        banks = filter_banks(list(self.A) + list(self.B), [True] * K + [False] * K)
        return banks[:K], banks[K:]

    @torch.no_grad()
    def project(self):
        self.t.clamp_(0.0)
