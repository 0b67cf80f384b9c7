"""Torch restatement of pytorch_msssim's `ms_ssim`, written from its definition on top of tests/ssim_restate.py (the
oracle of the MS-SSIM tests; pytorch_msssim is not installed here).  Runs in the dtype of its inputs: float64 is the
oracle, float32 gives the error an fp32 evaluation of the same formulas makes, which sets the GPU tests' tolerances.

    for i in 0 .. L-1:
        ssim_i, cs_i = per-(n, c) means of the SSIM map and of the cs map of (X_i, Y_i)
        if i < L-1: X_{i+1} = avg_pool2d(X_i, kernel_size=2, padding=[H_i % 2, W_i % 2])      (same for Y)
    v = stack(relu(cs_0), .., relu(cs_{L-2}), relu(ssim_{L-1}))         # (L, N, C)
    ms = prod_i v_i ** weights_i                                        # (N, C)
"""
import torch
import torch.nn.functional as F

import ssim_restate as R

WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def pool(x):
    """One step of the pyramid for (N, C, H, W): torch's default avg_pool2d (count_include_pad=True, stride 2), an odd
    axis padded by one zero row / column on each side, of which only the leading one is ever read."""
    return F.avg_pool2d(x, kernel_size=2, padding=[x.shape[-2] % 2, x.shape[-1] % 2])


def level_sizes(H, W, levels):
    out = []
    for _ in range(levels):
        out.append((H, W))
        H, W = (H + H % 2) // 2, (W + W % 2) // 2
    return out


def table(X, Y, data_range=255, win_size=11, win_sigma=1.5, levels=5, K=(0.01, 0.03)):
    """(levels, N, C, 2): the raw (ssim_i, cs_i) means of every level."""
    rows = []
    for i in range(levels):
        s, cs = R.ssim_cs_per_channel(X, Y, data_range, win_size, win_sigma, K)
        rows.append(torch.stack([s, cs], -1))
        if i < levels - 1:
            X, Y = pool(X), pool(Y)
    return torch.stack(rows)


def combine(tab, weights):
    """(L, N, C, 2) table -> (v (L, N, C), ms (N, C))."""
    v = torch.relu(torch.cat([tab[:-1, ..., 1], tab[-1:, ..., 0]]))
    w = torch.as_tensor(weights, dtype=tab.dtype)
    return v, torch.prod(v ** w.view(-1, 1, 1), dim=0)


def ms_ssim_per_channel(X, Y, data_range=255, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    weights = WEIGHTS if weights is None else weights
    return combine(table(X, Y, data_range, win_size, win_sigma, len(weights), K), weights)[1]


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim for 4-D input.  data_range: number, or tensor broadcastable to (N, C, 1, 1)."""
    ms = ms_ssim_per_channel(X, Y, data_range, win_size, win_sigma, weights, K)
    return ms.mean() if size_average else ms.mean(1)


def ms_ssim_frames(output, target, data_range=None, weights=None):
    """mean_t (1 - ms_ssim(frame t)), literally per frame; data_range None: max - min of the output frame, a (D,) tensor:
    its t-th value, anything else as given."""
    D = output.shape[2]
    total = 0
    for t in range(D):
        o, g = output[:, :, t], target[:, :, t]
        if data_range is None:
            r = o.max() - o.min()
        elif torch.is_tensor(data_range) and data_range.dim() == 1:
            r = data_range[t]
        else:
            r = data_range
        total = total + (1 - ms_ssim(o, g, data_range=r, weights=weights))
    return total / D
