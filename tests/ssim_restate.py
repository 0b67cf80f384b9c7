"""Torch restatement of the two SSIM definitions the reference uses, written from their formulas (the oracle of the
ssim tests; neither library is installed here).  Runs in the dtype of its inputs: float64 is the oracle, float32
gives the error an fp32 evaluation of the same formulas makes, which sets the GPU tests' tolerances.

* pytorch_msssim's `ssim` (loss.py's CombinedLossWithSSIM): Gaussian 1-D window, depthwise conv2d along H then W
  with no padding, compensation (kappa) 1, mean of the map per channel.
* skimage's `structural_similarity` (analyzemri.py): uniform_filter of size win_size with scipy's 'reflect'
  border (the edge sample repeats: d c b a | a b c d | d c b a), sample covariance (kappa = n / (n - 1)), map cropped
  by (win_size - 1) // 2 on every side, then the mean.
"""
import torch
import torch.nn.functional as F


def gaussian_window(win_size=11, win_sigma=1.5, dtype=torch.float64):
    coords = torch.arange(win_size, dtype=dtype) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    return g / g.sum()


def _filter_valid(x, win):
    """x (N, C, H, W), win (T,): depthwise conv2d along H, then along W, no padding (pytorch_msssim's
    gaussian_filter)."""
    C, T = x.shape[1], win.numel()
    w = win.to(x.dtype)
    out = F.conv2d(x, w.reshape(1, 1, T, 1).expand(C, 1, T, 1), groups=C)
    return F.conv2d(out, w.reshape(1, 1, 1, T).expand(C, 1, 1, T), groups=C)


def _maps(mu1, mu2, e11, e22, e12, kappa, C1, C2):
    s1 = kappa * (e11 - mu1 * mu1)
    s2 = kappa * (e22 - mu2 * mu2)
    s12 = kappa * (e12 - mu1 * mu2)
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
    return ssim_map, cs_map


def ssim_cs_per_channel(X, Y, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """pytorch_msssim's _ssim: (N, C) means of the SSIM map and of the cs map.  data_range: number, or tensor
    broadcastable to (N, C, 1, 1) (one value per plane)."""
    win = gaussian_window(win_size, win_sigma, X.dtype)
    C1 = (K[0] * data_range) ** 2
    C2 = (K[1] * data_range) ** 2
    f = lambda t: _filter_valid(t, win)                                       # noqa: E731
    ssim_map, cs_map = _maps(f(X), f(Y), f(X * X), f(Y * Y), f(X * Y), 1.0, C1, C2)
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ssim_per_channel(X, Y, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """(N, C) means of the SSIM map."""
    return ssim_cs_per_channel(X, Y, data_range, win_size, win_sigma, K)[0]


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """pytorch_msssim.ssim for 4-D input."""
    pc = ssim_per_channel(X, Y, data_range, win_size, win_sigma, K)
    if nonnegative_ssim:
        pc = torch.relu(pc)
    return pc.mean() if size_average else pc.mean(1)


def ssim_frames(output, target, data_range=None):
    """loss.py:39-56's SSIM term, literally: per frame t, repeat to three channels, data_range = max - min of the
    repeated output frame, 1 - ssim; averaged over the frames."""
    D = output.shape[2]
    total = 0
    for t in range(D):
        o3 = output[:, :, t].repeat(1, 3, 1, 1)
        g3 = target[:, :, t].repeat(1, 3, 1, 1)
        R = o3.max() - o3.min() if data_range is None else data_range
        total = total + (1 - ssim(o3, g3, data_range=R))
    return total / D


def _reflect_index(n, r):
    """scipy.ndimage mode 'reflect' indices of a length-n axis padded by r on both sides."""
    idx = torch.arange(-r, n + r)
    idx = torch.where(idx < 0, -idx - 1, idx)
    return torch.where(idx >= n, 2 * n - idx - 1, idx)


def uniform_filter_reflect(x, size):
    """scipy.ndimage.uniform_filter(x, size) over the last two axes of x (..., H, W), mode 'reflect'."""
    r = size // 2
    H, W = x.shape[-2:]
    xp = x[..., _reflect_index(H, r), :][..., _reflect_index(W, r)]
    lead = xp.shape[:-2]
    flat = xp.reshape(-1, 1, *xp.shape[-2:])
    w = torch.full((size,), 1.0 / size, dtype=x.dtype)
    out = _filter_valid(flat, w)
    return out.reshape(*lead, H, W)


def structural_similarity(x, y, data_range=1.0, win_size=7, K1=0.01, K2=0.03, full=False):
    """skimage.metrics.structural_similarity (gaussian_weights=False, use_sample_covariance=True) of every trailing
    (H, W) plane: a tensor shaped like the leading dims.  full=True also returns the uncropped map."""
    if win_size % 2 != 1:
        raise ValueError("Window size must be odd.")
    if win_size > min(x.shape[-2:]):
        raise ValueError("win_size exceeds image extent.")
    NP = win_size ** 2
    cov_norm = NP / (NP - 1)
    f = lambda t: uniform_filter_reflect(t, win_size)                        # noqa: E731
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    S, _ = _maps(f(x), f(y), f(x * x), f(y * y), f(x * y), cov_norm, C1, C2)
    pad = (win_size - 1) // 2
    H, W = x.shape[-2:]
    mssim = S[..., pad:H - pad, pad:W - pad].mean(dim=(-2, -1))
    return (mssim, S) if full else mssim


def structural_similarity_valid(x, y, data_range=1.0, win_size=7, K1=0.01, K2=0.03):
    """The same mean, from valid filtering (what the device kernel computes)."""
    NP = win_size ** 2
    w = torch.full((win_size,), 1.0 / win_size, dtype=x.dtype)
    lead, (H, W) = x.shape[:-2], x.shape[-2:]
    f = lambda t: _filter_valid(t.reshape(-1, 1, H, W), w)                    # noqa: E731
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    S, _ = _maps(f(x), f(y), f(x * x), f(y * y), f(x * y), NP / (NP - 1), C1, C2)
    return S.mean(dim=(-2, -1)).reshape(lead)
