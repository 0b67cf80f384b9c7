"""Restatement of the local MAD noise-level estimate, used by test_nle_map_cpu.py and
test_gpu_nle_map.py.  Written from the definition with host torch / numpy only: the band by conv2d with the oracle's
taps, the cells by slicing and torch.median, the map by numpy.interp (piecewise linear, constant outside the nodes)
along each axis in float64."""
import math

import numpy as np
import torch

import cdlnet_video_amd as cva
from oracle import cdl_oracle as O

TAPS = 10


def band(y):
    """|HH| of y (N,C,H,W): (N,C,Hb,Wb), the tensor O.nle_mad takes its median of."""
    C = y.shape[1]
    return torch.nn.functional.conv2d(y, torch.cat([O.hh_filter()] * C), stride=2, groups=C).abs()


def cell_ranges(L, w, q):
    """[(i0, i1)] of the cells along an axis of band length L."""
    if L <= w:
        return [(0, L)]
    n = math.ceil((L - w) / q) + 1
    return [(min(i * q, L - w), min(i * q, L - w) + w) for i in range(n)]


def centres(L, w, q):
    """Cell centres in pixels: band sample i sees pixels 2i .. 2i+9."""
    return [i0 + i1 - 1 + 4.5 for i0, i1 in cell_ranges(L, w, q)]


def cells(y, w=32, q=None):
    """(N,1,ny,nx) for y (N,C,H,W); (N,1,D,ny,nx) for a clip (N,C,D,H,W), frame by frame."""
    q = w // 2 if q is None else q
    if y.dim() == 5:
        return torch.stack([cells(y[:, :, d], w, q) for d in range(y.shape[2])], dim=2)
    b = band(y)
    ry, rx = cell_ranges(b.shape[2], w, q), cell_ranges(b.shape[3], w, q)
    out = torch.empty(y.shape[0], 1, len(ry), len(rx))
    for iy, (y0, y1) in enumerate(ry):
        for ix, (x0, x1) in enumerate(rx):
            out[:, 0, iy, ix] = torch.median(b[:, :, y0:y1, x0:x1].reshape(y.shape[0], -1), dim=1)[0] / 0.6745
    return out


def interpolate(c, H, W, w=32, q=None):
    """Cells (N,1,ny,nx) of an H x W image -> (N,1,H,W), float64 inside."""
    q = w // 2 if q is None else q
    cy, cx = centres((H - TAPS) // 2 + 1, w, q), centres((W - TAPS) // 2 + 1, w, q)
    a = c[:, 0].double().numpy()
    rows = np.stack([[np.interp(np.arange(H), cy, a[n, :, j]) for j in range(a.shape[2])]
                     for n in range(a.shape[0])])                                  # (N, nx, H)
    full = np.stack([[np.interp(np.arange(W), cx, rows[n, :, i]) for i in range(H)] for n in range(a.shape[0])])
    return torch.from_numpy(full).float()[:, None]


def image_map(y, w=32, q=None):
    """The map at the image grid: (N,1,H,W), or (N,1,D,H,W) for a clip."""
    if y.dim() == 5:
        return torch.stack([image_map(y[:, :, d], w, q) for d in range(y.shape[2])], dim=2)
    return interpolate(cells(y, w, q), y.shape[2], y.shape[3], w, q)


def code_map(y, w=32, q=None, s=1):
    return cva.utils.sigma_to_code_grid(image_map(y, w, q), s)


def frames(clip):
    """(N,1,D,1,1): O.nle_mad of every frame."""
    return torch.stack([O.nle_mad(clip[:, :, d]) for d in range(clip.shape[2])], dim=2)


def cell_truth(true_map, w=32, q=None):
    """Mean of a true map (N,1,H,W) over the pixels each cell sees: (N,1,ny,nx)."""
    q = w // 2 if q is None else q
    H, W = true_map.shape[2:]
    ry, rx = cell_ranges((H - TAPS) // 2 + 1, w, q), cell_ranges((W - TAPS) // 2 + 1, w, q)
    out = torch.empty(true_map.shape[0], 1, len(ry), len(rx))
    for iy, (y0, y1) in enumerate(ry):
        for ix, (x0, x1) in enumerate(rx):
            out[:, 0, iy, ix] = true_map[:, 0, 2 * y0:2 * (y1 - 1) + TAPS, 2 * x0:2 * (x1 - 1) + TAPS].mean(dim=(1, 2))
    return out
