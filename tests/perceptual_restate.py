"""Torch restatement of the perceptual term of the reference's CombinedLossWithSSIM, written from its definition (the
oracle of the perceptual tests; torchvision is not installed here).  Runs in the dtype of its inputs: float64 is the
oracle, float32 gives the error an fp32 evaluation of the same formulas makes, which sets the GPU tests' tolerances.

F = VGG16 features[:16]: conv(3->64), relu, conv(64->64), relu, maxpool 2x2/2, conv(64->128), relu, conv(128->128),
relu, maxpool, conv(128->256), relu, conv(256->256), relu, conv(256->256), relu -- every conv 3x3, padding 1, bias; the
pools in floor mode.  The input is a one-channel frame repeated to three channels.

`features` can replace every ReLU by a prescribed 0/1 gate and every max-pool by a gather at prescribed argmax codes
(0..3, row-major in the 2x2 window): given those, F is affine in its input and the gradient is exactly defined.
"""
import torch
import torch.nn.functional as F

import ssim_restate

CONVS = (0, 2, 5, 7, 10, 12, 14)
SHAPES = {0: (64, 3), 2: (64, 64), 5: (128, 64), 7: (128, 128), 10: (256, 128), 12: (256, 256), 14: (256, 256)}
POOL_AFTER = (2, 7)                       # the max-pools follow the convolutions at these indices


def random_weights(seed=0, bias_scale=0.05):
    """Kaiming-normal (fan_out, relu) weights as torchvision initialises VGG, with non-zero biases: bare "N.*" keys."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in CONVS:
        o, c = SHAPES[i]
        std = (2.0 / (o * 9)) ** 0.5
        sd[f"{i}.weight"] = torch.randn((o, c, 3, 3), generator=g) * std
        sd[f"{i}.bias"] = torch.randn((o,), generator=g) * bias_scale
    return sd


def _pool_at(h, codes):
    """h (P, C, H, W), codes (P, C, H//2, W//2) in 0..3 -> h at those window positions (differentiable in h)."""
    P, C, H, W = h.shape
    Hp, Wp = codes.shape[-2:]
    rows = 2 * torch.arange(Hp, device=h.device).view(Hp, 1) + (codes // 2)
    cols = 2 * torch.arange(Wp, device=h.device).view(1, Wp) + (codes % 2)
    idx = (rows * W + cols).reshape(P, C, -1)
    return h.reshape(P, C, H * W).gather(2, idx).reshape(P, C, Hp, Wp)


def features(x, sd, sum_conv1=True, gates=None, codes=None, trace=None):
    """x (P, 1, H, W) -> relu3_3 (P, 256, H4, W4).  sum_conv1: conv1_1 as a 1 -> 64 convolution with the filters
    summed over their three input channels (otherwise the three-channel repeat).  gates: seven 0/1 tensors replacing
    the ReLUs; codes: two argmax-code tensors replacing the max-pools.  trace (a list): receives, per layer, the
    pre-activation and, per pool, the first-maximum codes of its input (torch's max-pool convention)."""
    dt = x.dtype
    h = x
    for k, i in enumerate(CONVS):
        w, b = sd[f"{i}.weight"].to(dt), sd[f"{i}.bias"].to(dt)
        if i == 0:
            if sum_conv1:
                h = F.conv2d(h, w.sum(dim=1, keepdim=True), b, padding=1)
            else:
                h = F.conv2d(h.repeat(1, 3, 1, 1), w, b, padding=1)
        else:
            h = F.conv2d(h, w, b, padding=1)
        if trace is not None:
            trace.append(h.detach())
        h = h * gates[k].to(dt) if gates is not None else F.relu(h)
        if i in POOL_AFTER:
            p = POOL_AFTER.index(i)
            if codes is not None:
                h = _pool_at(h, codes[p])
            else:
                pooled, idx = F.max_pool2d(h, 2, 2, return_indices=True)
                if trace is not None:
                    W = h.shape[-1]
                    r, c = idx // W, idx % W
                    trace.append(((r % 2) * 2 + (c % 2)).to(torch.uint8))
                h = pooled
    return h


def perceptual(output, target, sd, per_frame=False, **kw):
    """(B, 1, T, H, W) clips -> the perceptual term: per_frame=True is the reference's loop
    (1/T) sum_t mean((F(o_t) - F(g_t))^2); otherwise one mean over all B*T planes (the same value)."""
    B, C, T, H, W = output.shape
    if per_frame:
        total = 0.0
        for t in range(T):
            fo = features(output[:, :, t], sd, **kw)
            fg = features(target[:, :, t], sd, **kw)
            total = total + torch.mean((fo - fg) ** 2)
        return total / T
    o = output.permute(0, 2, 1, 3, 4).reshape(B * T, 1, H, W)
    g = target.permute(0, 2, 1, 3, 4).reshape(B * T, 1, H, W)
    return torch.mean((features(o, sd, **kw) - features(g, sd, **kw)) ** 2)


def combined(output, target, sd, alpha=1.0, beta=0.01, gamma=0.1):
    """CombinedLossWithSSIM: alpha * MSE + beta * perceptual + gamma * mean_t (1 - SSIM_t) (tests/ssim_restate.py)."""
    mse = torch.mean((output - target) ** 2)
    return alpha * mse + beta * perceptual(output, target, sd) + gamma * ssim_restate.ssim_frames(output, target)
