"""Blind noise-level estimation (reference model/nle.py): `noise_level(y, method="MAD")` / `nle_mad(y)`, `nle_pca(y)`,
and the local forms of the MAD estimate that produce a noise-level map: `nle_mad_cells`, `nle_mad_map`,
`nle_mad_frames`.

`nle_mad` runs in libcdlnet_hip.so (cdl_nle_mad): depthwise stride-2 correlation with the 'bior4.4'
diagonal (HH) analysis filter and an exact per-sample median.  `nle_pca` (weak-texture PCA) forms, per pass and
channel, the second moment of the weak-texture patches in one HIP sweep (cdl_nle_pca_gram); the host keeps only the
p^2 x p^2 eigenvalue problem and the constants of the patch size.
"""
import functools
import math

import numpy as np
import torch

from . import _lib, ops, utils


def nle_mad(y):
    """Median-absolute-deviation estimate of the AWGN standard deviation of y (N,C,H,W), in y's own
    scale; returns (N,1,1,1) like the reference (model/nle.py:17-27)."""
    y = ops._dev(y, "y")
    if y.dim() != 4:
        raise ValueError("nle_mad expects (N, C, H, W)")
    N, C, H, W = y.shape
    n = int(_lib.lib().cdl_nle_mad_scratch_floats(N, C, H, W))
    if n == 0:
        raise ValueError("image smaller than the 10 x 10 wavelet filter")
    scratch = ops._scratch(y.device, n)
    out = torch.empty(N, device=y.device, dtype=torch.float32)
    ops._call("cdl_nle_mad", y, out, scratch, n, N, C, H, W)
    return out.reshape(-1, 1, 1, 1)


TAPS = 10                              # the 'bior4.4' diagonal filter is 10 x 10; band sample i sees pixels 2i .. 2i+9


def band_length(L):
    return (L - TAPS) // 2 + 1


def cell_starts(L, window, step):
    """First band sample of every cell along an axis of band length L: one cell [0, L) if L <= window, otherwise
    ceil((L - window) / step) + 1 cells of `window` samples, the last flush with the border."""
    if L <= window:
        return [0]
    return [min(i * step, L - window) for i in range(-(-(L - window) // step) + 1)]


def _window_step(window, step):
    if window is None or int(window) != window or window < 2:
        raise ValueError(f"window {window!r}: expected an integer >= 2 (band samples)")
    step = int(window) // 2 if step is None else step
    if int(step) != step or step < 1:
        raise ValueError(f"step {step!r}: expected an integer >= 1 (band samples)")
    return int(window), int(step)


def _frames(y, name):
    """(images (B,C,H,W), leading shape of the result): a clip (N,C,D,H,W) is its N*D frames, never mixed."""
    y = ops._dev(y, "y")
    if y.dim() == 4:
        lead = (y.shape[0], 1)
    elif y.dim() == 5:
        lead = (y.shape[0], 1, y.shape[2])
        y = y.transpose(1, 2).reshape((-1, y.shape[1]) + tuple(y.shape[3:]))      # a view for C = 1
    else:
        raise ValueError(f"{name} expects (N, C, H, W) or (N, C, D, H, W)")
    if y.shape[-2] < TAPS or y.shape[-1] < TAPS:
        raise ValueError("image smaller than the 10 x 10 wavelet filter")
    return y.contiguous(), lead


def _cells(y, window, step):
    """cdl_nle_mad_cells on images y (B,C,H,W): (B, ny, nx)."""
    B, C, H, W = y.shape
    ny = len(cell_starts(band_length(H), window, step))
    nx = len(cell_starts(band_length(W), window, step))
    n = int(_lib.lib().cdl_nle_mad_cells_scratch_floats(B, C, H, W))
    scratch = ops._scratch(y.device, n)
    out = torch.empty((B, ny, nx), device=y.device, dtype=torch.float32)
    ops._call("cdl_nle_mad_cells", y, out, scratch, n, B, C, H, W, window, step)
    return out


def nle_mad_cells(y, window=32, step=None):
    """The MAD estimate of nle_mad over windows of the band instead of the whole image: the lower median of |HHy|
    over `window` x `window` band samples (all channels) / 0.6745, one value per cell, cells `step` samples apart
    (default window // 2), the last cell of an axis flush with the border; an axis whose band is no longer than the
    window is one cell.  y (N,C,H,W) gives (N,1,ny,nx); a clip (N,C,D,H,W) gives (N,1,D,ny,nx), every frame on its
    own.  In y's scale.  A window covering the band returns the bits of nle_mad."""
    window, step = _window_step(window, step)
    imgs, lead = _frames(y, "nle_mad_cells")
    cells = _cells(imgs, window, step)
    return cells.reshape(lead + tuple(cells.shape[1:]))


@functools.lru_cache(maxsize=64)
def _interp_plan(L, window, step, device):
    """(lo, hi, t) on `device` for one axis of L pixels: pixel p takes (1 - t) * cell[lo] + t * cell[hi], the
    piecewise-linear interpolation between the cell centres, constant beyond the first and the last.  A cell
    [i0, i1) of the band sees pixels 2 i0 .. 2 (i1 - 1) + 9: centre i0 + i1 - 1 + 4.5.  Device ops only."""
    Lb = band_length(L)
    n = len(cell_starts(Lb, window, step))
    i0 = (torch.arange(n, device=device) * step).clamp(max=max(Lb - window, 0))
    centre = (2 * i0 + (min(window, Lb) - 1)).double() + 4.5
    p = torch.arange(L, device=device, dtype=torch.float64)
    hi = torch.bucketize(p, centre).clamp(max=n - 1)            # first centre >= p
    lo = (hi - 1).clamp(min=0)
    gap = centre[hi] - centre[lo]
    t = torch.where(gap > 0, (p - centre[lo]) / gap.clamp(min=1.0), torch.zeros_like(p)).clamp(0.0, 1.0)
    return lo, hi, t.float()


def _interpolate(cells, H, W, window, step):
    """cells (B, ny, nx) -> (B, H, W), separable."""
    lo, hi, t = _interp_plan(H, window, step, cells.device)
    rows = torch.lerp(cells.index_select(1, lo), cells.index_select(1, hi), t[:, None])
    lo, hi, t = _interp_plan(W, window, step, cells.device)
    return torch.lerp(rows.index_select(2, lo), rows.index_select(2, hi), t)


def nle_mad_frames(clip):
    """One MAD estimate per frame of a clip (N,C,D,H,W): (N,1,D,1,1), each value the bits of nle_mad of that frame;
    the per-frame form of `sigma` the nets take (times 255)."""
    clip = ops._dev(clip, "clip")
    if clip.dim() != 5:
        raise ValueError("nle_mad_frames expects (N, C, D, H, W)")
    imgs, lead = _frames(clip, "nle_mad_frames")
    whole = max(band_length(imgs.shape[-2]), band_length(imgs.shape[-1]), 2)
    return _cells(imgs, whole, whole).reshape(lead + (1, 1))


def nle_mad_map(y, window=32, step=None, s=1):
    """A blind noise-level map for `net(y, 255 * nle_mad_map(y, s=net.s))`: the cells of nle_mad_cells interpolated
    to the image grid (separable, piecewise linear between the cell centres, constant beyond the outermost), then
    taken to the code grid of a stride-`s` net by utils.sigma_to_code_grid.  y (N,C,H,W) gives (N,1,ceil(H/s),ceil(W/s)),
    a clip (N,C,D,H,W) a map per frame on the clip's code grid.  window=None is one level per image, nle_mad(y)
    (N,1,1,1), or per frame, nle_mad_frames(y) (N,1,D,1,1).  In y's scale; no copy to the host, no synchronisation."""
    if window is None:
        if torch.is_tensor(y) and y.dim() == 5:
            return nle_mad_frames(y)
        return nle_mad(y)
    window, step = _window_step(window, step)
    imgs, lead = _frames(y, "nle_mad_map")
    H, W = imgs.shape[-2:]
    img_map = _interpolate(_cells(imgs, window, step), H, W, window, step).reshape(lead + (H, W))
    return utils.sigma_to_code_grid(img_map, s)


def _derivative_matrix(p, horizontal):
    """Rows: every valid position of the half-difference [1/2, 0, -1/2] inside a p x p patch (row-major pixel order),
    along rows (horizontal) or columns; D @ patch = the derivatives the texture strength squares and sums."""
    rows = []
    for i in range(p if horizontal else p - 2):
        for j in range(p - 2 if horizontal else p):
            r = torch.zeros(p * p, dtype=torch.float64)
            r[i * p + j] = 0.5
            r[(i * p + j + 2) if horizontal else ((i + 2) * p + j)] = -0.5
            rows.append(r)
    return torch.stack(rows)


def _gamma_quantile(q, shape, scale):
    """gamma.ppf(q, shape, scale) by bisection on the regularized incomplete gamma function in float64 (no scipy);
    for q > 1/2 on the upper tail, which keeps full relative precision of 1 - q."""
    a = torch.tensor(shape, dtype=torch.float64)

    def above(x):                    # is the quantile below x?
        xt = torch.tensor(x / scale, dtype=torch.float64)
        if q > 0.5:
            return float(torch.special.gammaincc(a, xt)) <= 1.0 - q
        return float(torch.special.gammainc(a, xt)) >= q

    lo, hi = 0.0, max(1.0, shape * scale)
    while not above(hi):
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if above(mid):
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def pca_constants(patchsize=7, conf=1 - 1e-6):
    """(tau0, r, tr(DD)) of the reference's nle_pca for one (patchsize, conf), in float64:
    DD = Dh^T Dh + Dv^T Dv of the two derivative matrices, r = rank(DD),
    tau0 = gamma.ppf(conf, r / 2, scale = 2 tr(DD) / r)  (the texture threshold per unit noise variance)."""
    Dh, Dv = _derivative_matrix(patchsize, True), _derivative_matrix(patchsize, False)
    DD = Dh.T @ Dh + Dv.T @ Dv
    r = int(torch.linalg.matrix_rank(DD, hermitian=True))
    tr = float(torch.trace(DD))
    return _gamma_quantile(conf, r / 2.0, 2.0 * tr / r), r, tr


def pca_gram(y, channel, patchsize, tau):
    """One pass on the device (cdl_nle_pca_gram): (G, count) with G = sum x x^T (float64 (p^2, p^2), on y's device)
    over the patches of `channel` whose texture strength is below tau (float32; +inf keeps every patch) and count
    their number (int)."""
    N, C, H, W = y.shape
    n = int(_lib.lib().cdl_nle_pca_scratch_floats(N, C, H, W, patchsize))
    if n == 0:
        raise ValueError(f"nle_pca: patchsize {patchsize} outside 3..11 or larger than the image {H} x {W}")
    scratch = ops._scratch(y.device, n)
    gram = torch.empty(patchsize * patchsize, patchsize * patchsize, device=y.device, dtype=torch.float64)
    count = torch.empty(1, device=y.device, dtype=torch.int64)
    ops._call("cdl_nle_pca_gram", y, N, C, H, W, channel, patchsize, tau, gram, count, scratch, n)
    return gram, int(count.item())


def _smallest_eigenvalue(gram, count):
    return float(torch.linalg.eigvalsh(gram.cpu() / (count - 1))[0])


def nle_pca(img, patchsize=7, conf=1 - 1e-6, itr=3):
    """Weak-texture PCA estimate of the AWGN standard deviation (reference model/nle.py:29-89), per channel of
    img (N,C,H,W); returns (nlevel, th, num) as the reference does: numpy.float64 scalars for C = 1, length-C float64
    arrays otherwise.  nlevel is what the reference's `noise_level(y, "PCA")` returns.

    Kept from the reference: patches (every p x p window at stride 1) are pooled over the whole batch, one estimate
    per channel; the second moment X X^T / (count - 1) is NOT centred; `num` (the number of patches the last pass
    kept) is a float; with fewer patches than p^2 the result is (0, 0, 0) (sig2 = 0, so tau = 0 keeps nothing).
    The refinement runs for i in range(2, itr): tau = sig2 * tau0, keep Xtr < tau, stop if fewer than p^2 remain.

    Where the reference's code fails, this one does what it evidently intends: C > 1 (the reference raises in
    conv2d) estimates every channel independently; itr <= 2 (the reference raises on inf.item()) returns th = inf
    with no refinement; H or W < patchsize (the reference's unfold raises) raises ValueError.

    Precision: the Gram matrices are formed on the device in fp32 matrix cores over shifted data and summed in fp64
    (csrc/cdl_nle_pca.hip), the smallest eigenvalue is taken in float64, so the result follows a float64 evaluation
    of the reference's formulas (the reference's own fp32 eigenvalue is ~1e-4 off it).  The threshold is compared
    in fp32, as the reference compares its fp32 texture strengths with an fp32 tau."""
    img = ops._dev(img, "img")
    if img.dim() != 4:
        raise ValueError("nle_pca expects (N, C, H, W)")
    N, C, H, W = img.shape
    p = int(patchsize)
    if not 3 <= p <= 11:
        raise ValueError(f"nle_pca: patchsize {p} outside 3..11")
    if H < p or W < p:
        raise ValueError(f"nle_pca: image {H} x {W} smaller than the {p} x {p} patch")
    img = img.contiguous()
    tau0 = pca_constants(p, conf)[0]
    total = N * (H - p + 1) * (W - p + 1)
    nlevel, th, num = np.empty(C), np.empty(C), np.empty(C)
    for c in range(C):
        tau, kept = math.inf, total
        if total < p * p:
            sig2 = 0.0
        else:
            gram, kept = pca_gram(img, c, p, math.inf)
            sig2 = _smallest_eigenvalue(gram, kept)
        for _ in range(2, itr):
            tau = sig2 * tau0
            gram, kept = pca_gram(img, c, p, tau)
            if kept < p * p:
                break
            sig2 = _smallest_eigenvalue(gram, kept)
        nlevel[c] = np.sqrt(sig2)
        th[c] = tau
        num[c] = kept
    if C == 1:
        return nlevel[0], th[0], num[0]
    return nlevel, th, num


def noise_level(y, method="MAD", **kwargs):
    """model/nle.py:9-15 for "MAD" (or True / "wvlt"): nle_mad(y), an (N,1,1,1) tensor.  This entry point's contract is
    the MAD estimate only, and "PCA" keeps raising NotImplementedError; the weak-texture PCA estimate, i.e. what the
    reference's noise_level(y, "PCA") returns, is nle_pca(y)[0]."""
    if method in (True, "MAD", "wvlt"):
        return nle_mad(y)
    if method == "PCA":
        raise NotImplementedError("noise_level runs the MAD estimator only; for the weak-texture PCA estimate "
                                  "(the reference's noise_level(y, 'PCA')) call nle_pca(y)[0]")
    raise NotImplementedError(f"noise_level method {method!r}: only the MAD / wavelet estimator runs here")
