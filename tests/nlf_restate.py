"""Restatement of the blind noise-level function var(y | x) = a x + b and its sigma map, used by
test_nlf_cpu.py and test_gpu_nlf.py.  Written from the definition in float64 numpy: the band |HHy| and the local mean m
by slicing, the bins by a floor and a sort per bin, the fit by its five sums, the map by a reflect-padded box mean.
Nothing here is shared with the package but the taps of the oracle and utils.sigma_to_code_grid."""
import numpy as np
import torch

import cdlnet_video_amd as cva
from oracle import cdl_oracle as O

TAPS = 10
TINY = 1e-12                           # floor of a variance inside a weight


# ------------------------------------------------------------------------------------------------ test content
def content(H, W, seed):
    """x in [0.05, 0.95]: a ramp along the columns (0.7) plus a sine along the rows (0.3) with a seeded phase, so that
    the local means span the intensity range."""
    phi = np.random.default_rng(seed).random()
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    return 0.05 + 0.9 * (0.7 * j / (W - 1) + 0.3 * (0.5 + 0.5 * np.sin(2 * np.pi * (1.5 * i / (H - 1) + phi))))


def noisy(H, W, seed, a0, b0):
    """(x, y): y = x + randn * sqrt(a0 x + b0), the noise from default_rng(100 + seed)."""
    x = content(H, W, seed)
    return x, x + np.random.default_rng(100 + seed).standard_normal((H, W)) * np.sqrt(a0 * x + b0)


# ------------------------------------------------------------------------------------------------ 1. bands
def bands(y):
    """(d, m) of an image y (C,H,W), each (C,Hb,Wb) float64: d = |HHy| at stride 2, m the mean of the 7 x 7 pixels that
    carry non-zero taps (rows 2i+2 .. 2i+8, columns 2j+2 .. 2j+8)."""
    y = np.asarray(y, dtype=np.float64)
    f = O.hh_filter()[0, 0].double().numpy()
    C, H, W = y.shape
    Hb, Wb = (H - TAPS) // 2 + 1, (W - TAPS) // 2 + 1
    d, m = np.zeros((C, Hb, Wb)), np.zeros((C, Hb, Wb))
    for a in range(TAPS):
        for b in range(TAPS):
            v = y[:, a:a + 2 * Hb - 1:2, b:b + 2 * Wb - 1:2]
            d += f[a, b] * v
            if 2 <= a <= 8 and 2 <= b <= 8:
                m += v
    return np.abs(d), m / 49.0


# ------------------------------------------------------------------------------------------------ 2, 3. bins
def bin_index(m, bins, lo, hi, f32=False):
    """Bin of every sample, -1 for none.  f32: the arithmetic of the device -- m, lo and hi in float32, the scale
    bins / (hi - lo) rounded to float32 once, k = (int)floorf((m - lo) * scale), every operation rounded to float32."""
    if f32:
        m, lo, hi = np.asarray(m, dtype=np.float32), np.float32(lo), np.float32(hi)
        scale = np.float32(bins / (float(hi) - float(lo)))
        k = np.floor(((m - lo).astype(np.float32) * scale).astype(np.float32))
    else:
        m = np.asarray(m, dtype=np.float64)
        k = np.floor((m - lo) * (bins / (hi - lo)))
    inside = (m >= lo) & (m < hi) & (k < bins)
    return np.where(inside, k, -1).astype(np.int64)


def bin_stats(d, m, bins=32, lo=0.0, hi=1.0, f32=False):
    """(sigma_b, count_b, centre_b) of one image's bands (any shape, all channels pool).  sigma_b keeps d's dtype: a
    float32 band gives float32(median) / float32(0.6745), the device's own division."""
    d = np.asarray(d).reshape(-1)
    k = bin_index(np.asarray(m).reshape(-1), bins, lo, hi, f32)
    sigma, count = np.zeros(bins, dtype=d.dtype), np.zeros(bins, dtype=np.int64)
    for b in range(bins):
        members = np.sort(d[k == b])
        count[b] = members.size
        if members.size:
            sigma[b] = members[(members.size - 1) // 2] / d.dtype.type(0.6745)
    centre = lo + (np.arange(bins) + 0.5) * ((hi - lo) / bins)
    return sigma, count, centre


# ------------------------------------------------------------------------------------------------ 4. fit
def _solve(w, x, v):
    w = w / w.max()
    sw, swx, swxx, swv, swxv = w.sum(), (w * x).sum(), (w * x * x).sum(), (w * v).sum(), (w * x * v).sum()
    det = sw * swxx - swx * swx
    a, b = (sw * swxv - swx * swv) / det, (swxx * swv - swx * swxv) / det
    if a < 0:
        return 0.0, swv / sw
    if b < 0:
        return swxv / swxx, 0.0
    return a, b


def fit(sigma, count, centre, min_count=64, iters=2, fallback=None):
    """(a, b) of one image's bins, python floats."""
    sigma, count, centre = (np.asarray(t, dtype=np.float64) for t in (sigma, count, centre))
    use = count >= max(min_count, 1)
    if use.sum() == 0:
        return 0.0, 0.0 if fallback is None else float(fallback)
    x, v, c = centre[use], sigma[use] ** 2, count[use]
    if use.sum() == 1:
        return 0.0, float(v[0])
    a, b = _solve(c / np.maximum(v, TINY) ** 2, x, v)
    for _ in range(iters):
        a, b = _solve(c / np.maximum(a * x + b, TINY) ** 2, x, v)
    return float(a), float(b)


def usable_span(count, centre, min_count=64):
    """(first, last) usable bin centre."""
    c = np.asarray(centre)[np.asarray(count) >= max(min_count, 1)]
    return float(c[0]), float(c[-1])


def nlf(y, bins=32, lo=0.0, hi=1.0, min_count=64, iters=2):
    """(a, b, sigma_b, count_b, centre_b) of one image y (C,H,W); with no usable bin b is the square of the MAD estimate."""
    d, m = bands(y)
    sigma, count, centre = bin_stats(d, m, bins, lo, hi)
    flat = np.sort(d.reshape(-1))
    mad = flat[(flat.size - 1) // 2] / 0.6745
    a, b = fit(sigma, count, centre, min_count, iters, fallback=mad ** 2)
    return a, b, sigma, count, centre


# ------------------------------------------------------------------------------------------------ 5. map
def image_map(y, a, b, smooth=7, floor=1e-3):
    """sigma at the image grid (H,W) of one image y (C,H,W): sqrt(max(a m + b, floor^2)), m the channel mean under a
    smooth x smooth box with reflect padding."""
    m = np.asarray(y, dtype=np.float64).mean(axis=0)
    r = smooth // 2
    p = np.pad(m, r, mode="reflect")
    H, W = m.shape
    box = sum(p[i:i + H, j:j + W] for i in range(smooth) for j in range(smooth)) / (smooth * smooth)
    return np.sqrt(np.maximum(a * box + b, floor * floor))


def code_map(y, s=1, smooth=7, floor=1e-3, **fit_kw):
    """The blind map of a batch y (N,C,H,W) (a torch tensor or an array) on the code grid of a stride-s net:
    (N,1,ceil(H/s),ceil(W/s)) float64, every image its own fit."""
    y = np.asarray(y, dtype=np.float64)
    maps = []
    for img in y:
        a, b = nlf(img, **fit_kw)[:2]
        maps.append(image_map(img, a, b, smooth, floor))
    return cva.utils.sigma_to_code_grid(torch.from_numpy(np.stack(maps))[:, None], s)
