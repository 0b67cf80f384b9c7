"""Float64 restatement of the windowed weak-texture PCA estimate, used by
test_nle_pca_cells_cpu.py and test_gpu_nle_pca_cells.py: a cell is the whole-image estimate of nle_pca_restate.py on
the cell's crop, and the map is numpy.interp between the cell centres along each axis.  Host torch / numpy only."""
import math

import numpy as np
import torch

import nle_pca_restate as R

# image (H, W), N, window, step, p, itr, seed: seeds at which no pass's tau comes closer than 5e-5 (relative) to a
# texture strength of its cell, so an fp32 evaluation of Xtr keeps the same patches as this float64 one
PARITY_CASES = {
    "p7": ((75, 83), 2, 40, 20, 7, 3, 1),
    "p9": ((75, 83), 1, 48, 24, 9, 3, 5),
    "p5": ((75, 83), 1, 40, 20, 5, 5, 3),
    "p11": ((75, 83), 1, 48, 24, 11, 3, 0),
}
MIN_DISTANCE = 5e-5


def cell_ranges(L, w, q):
    """[(r0, r1)] of the cells along an axis of L pixels: one cell [0, L) if L <= w, otherwise ceil((L - w) / q) + 1
    cells of w pixels, the last flush with the border."""
    if L <= w:
        return [(0, L)]
    n = math.ceil((L - w) / q) + 1
    return [(min(i * q, L - w), min(i * q, L - w) + w) for i in range(n)]


def centres(L, w, q):
    return [r0 + (r1 - r0 - 1) / 2 for r0, r1 in cell_ranges(L, w, q)]


def clean(H, W):
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return (0.5 + 0.25 * torch.sin(2 * math.pi * (r / 37 + c / 53))
            + 0.15 * torch.sign(torch.sin(2 * math.pi * c / 29 + r / 11)))


def ramp(W):
    """The true noise level per column, in the image's scale: 5/255 at the left border to 25/255 at the right."""
    return torch.linspace(5.0, 25.0, W, dtype=torch.float64) / 255


def noisy(N, H, W, seed, C=1):
    """(N, C, H, W) float32: the clean image plus float64 noise whose level ramps across the width."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(N, C, H, W, dtype=torch.float64, generator=g)
    return (clean(H, W) + n * ramp(W)).float()


def fixed_image(N=2, H=40, W=45):
    """(N, 1, H, W) float32 from integer arithmetic and exactly rounded operations only: the same bits on every
    machine (no libm, no random generator)."""
    n, r, c = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    v = (7 * r * r + 3 * c * c + 5 * r * c + 11 * n) % 251
    return (0.4 + v.double() / 251 * 0.2 + (r + c).double() / 200).float()[:, None]


def cells(y, w, q, p, tau0, itr):
    """(nlevel, th, num) of every cell: three float64 arrays (N, C, ny, nx) for y (N, C, H, W), each cell the
    restatement's estimate of its crop."""
    N, C, H, W = y.shape
    ry, rx = cell_ranges(H, w, q), cell_ranges(W, w, q)
    out = np.zeros((3, N, C, len(ry), len(rx)))
    for n in range(N):
        for iy, (y0, y1) in enumerate(ry):
            for ix, (x0, x1) in enumerate(rx):
                out[:, n, :, iy, ix] = R.estimate(y[n:n + 1, :, y0:y1, x0:x1], p, tau0, itr)
    return out


def closest_distance(y, w, q, p, tau0, itr):
    """The smallest relative distance |Xtr - tau| / tau between the tau of any refinement pass of any cell and any
    texture strength of that cell (float64)."""
    N, C, H, W = y.shape
    best = math.inf
    for n in range(N):
        for y0, y1 in cell_ranges(H, w, q):
            for x0, x1 in cell_ranges(W, w, q):
                crop = y[n:n + 1, :, y0:y1, x0:x1]
                for c in range(C):
                    xtr = R.texture(crop[:, c], p)
                    for k in range(3, itr + 1):              # the tau of pass k - 1 is the th of a k-iteration run
                        tau = R.estimate(crop[:, c:c + 1], p, tau0, k)[1, 0]
                        if tau > 0 and math.isfinite(tau) and xtr.numel():
                            best = min(best, float(((xtr - tau).abs() / tau).min()))
    return best


def interpolate(c, H, W, w, q):
    """Cells (B, ny, nx) of H x W images -> (B, H, W) float64: numpy.interp along each axis (piecewise linear between
    the centres, constant outside them)."""
    cy, cx = centres(H, w, q), centres(W, w, q)
    a = np.asarray(c, dtype=np.float64)
    rows = np.stack([[np.interp(np.arange(H), cy, a[b, :, j]) for j in range(a.shape[2])] for b in range(a.shape[0])])
    return np.stack([[np.interp(np.arange(W), cx, rows[b, :, i]) for i in range(H)] for b in range(a.shape[0])])
