"""Blind noise-level estimation (reference model/nle.py): `noise_level(y, method="MAD")` / `nle_mad(y)`, `nle_pca(y)`,
and the local forms of the MAD estimate that produce a noise-level map: `nle_mad_cells`, `nle_mad_map`,
`nle_mad_frames`.

`nle_mad` runs in libcdlnet_hip.so (cdl_nle_mad): depthwise stride-2 correlation with the 'bior4.4'
diagonal (HH) analysis filter and an exact per-sample median.  `nle_pca` (weak-texture PCA) forms, per pass and
channel, the second moment of the weak-texture patches in one HIP sweep (cdl_nle_pca_gram); the host keeps only the
p^2 x p^2 eigenvalue problem and the constants of the patch size.  `nle_pca_cells`, `nle_pca_map` and `nle_pca_frames`
are that estimate per region and per frame: every cell of a regular grid its own domain, all
Grams of a pass from one launch chain (cdl_nle_pca_gram_cells); `noise_level_map` dispatches between the two map
estimators.  `nlf_bins`, `nlf_fit_bins`, `nlf_fit` and `nlf_map` estimate signal-dependent noise, var(y | x) = a x + b
(DESIGN.md section 29): the band of the MAD estimate binned by local intensity on the device (cdl_nle_nlf_bins), a
constrained line fit of the bins' variances, and the map sqrt(a m + b) the nets take.
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


# ------------------------------------------------- signal-dependent noise: var(y | x) = a x + b
NLF_TINY = 1e-12                       # floor of a variance inside a weight of the fit


def _nlf_args(bins, lo, hi):
    if int(bins) != bins or bins < 1:
        raise ValueError(f"bins {bins!r}: expected an integer >= 1")
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        raise ValueError(f"hi {hi!r} <= lo {lo!r}: the bins need a range")
    return int(bins), lo, hi


def _nlf_centres(bins, lo, hi, device):
    return lo + (torch.arange(bins, device=device, dtype=torch.float64) + 0.5) * ((hi - lo) / bins)


def _nlf_images(y, pool_frames, name):
    """(images (B,C',H,W), leading shape, leading shape of a fit): with pool_frames the frames of a clip join the
    channel axis (a reshape), so every selection pools the whole clip."""
    if pool_frames and torch.is_tensor(y) and y.dim() == 5:
        imgs, _ = _frames(y.reshape((y.shape[0], -1) + tuple(y.shape[3:])), name)
        return imgs, (y.shape[0], 1), (y.shape[0], 1, 1)
    imgs, lead = _frames(y, name)
    return imgs, lead, lead


def _nlf_bins(imgs, bins, lo, hi):
    """cdl_nle_nlf_bins on images (B,C,H,W): (sigma (B, bins) float32, count (B, bins) int32)."""
    B, C, H, W = imgs.shape
    n = int(_lib.lib().cdl_nle_nlf_bins_scratch_floats(B, C, H, W))
    scratch = ops._scratch(imgs.device, n)
    sigma = torch.empty((B, bins), device=imgs.device, dtype=torch.float32)
    count = torch.empty((B, bins), device=imgs.device, dtype=torch.int32)
    ops._call("cdl_nle_nlf_bins", imgs, sigma, count, scratch, n, B, C, H, W, bins, lo, hi)
    return sigma, count


def nlf_bins(y, bins=32, lo=0.0, hi=1.0, pool_frames=False):
    """The noise level of y by local intensity instead of position: (sigma, count, centre).  Every sample of the band
    of nle_mad carries d = |HHy| and m, the mean of the 7 x 7 pixels under the filter's non-zero taps; `bins` equal
    bins on [lo, hi) collect the samples by m (all channels pool; m outside [lo, hi) belongs to no bin), and
    sigma[..., k] is the lower median of d over bin k / 0.6745, count[..., k] (int32) the number of its members, an
    empty bin 0 and 0; centre (bins,) float64 are the bins' centres.  y (N,C,H,W) gives (N,1,bins); a clip
    (N,C,D,H,W) gives (N,1,D,bins), every frame on its own, or (N,1,bins) with pool_frames, the whole clip in one set
    of bins (a sensor's noise-level function does not change within a clip).  In y's scale; exact selection, repeated
    calls return the same bits; no copy to the host."""
    bins, lo, hi = _nlf_args(bins, lo, hi)
    imgs, lead, _ = _nlf_images(y, pool_frames, "nlf_bins")
    sigma, count = _nlf_bins(imgs, bins, lo, hi)
    centre = _nlf_centres(bins, lo, hi, imgs.device)
    return sigma.reshape(lead + (bins,)), count.reshape(lead + (bins,)), centre


def nlf_fit_bins(sigma, count, centre, min_count=64, iters=2, fallback=None):
    """(a, b) of var = a x + b from the bins of nlf_bins, float64, shaped like sigma without its last axis.  Plain
    torch on whatever device the bins are on, batched, no copy to the host:
      1. only bins with count >= min_count (and at least one member) are used;
      2. weighted least squares of v = sigma^2 against x = centre with w = count / max(v, tiny)^2 (the variance of a
         bin's v is proportional to v^2 / count);
      3. `iters` reweightings with w = count / max(a x + b, tiny)^2, the fitted variance in place of the noisy one;
      4. after every solve the constraints a >= 0, b >= 0: a < 0 gives a = 0, b = sum(w v) / sum(w); otherwise b < 0
         gives b = 0, a = sum(w x v) / sum(w x x);
      5. fewer than two usable bins: a = 0 and b the usable bin's v; none: b = fallback (a variance, broadcast against
         the result; None: 0)."""
    v = sigma.double() ** 2
    x = centre.double().expand_as(v)
    use = (count >= max(int(min_count), 1))
    cnt = torch.where(use, count.double(), torch.zeros_like(v))
    nuse = use.sum(dim=-1)

    def solve(var):
        w = cnt / var.clamp(min=NLF_TINY) ** 2
        w = w / w.amax(dim=-1, keepdim=True).clamp(min=1e-300)        # the fit does not depend on the scale of w
        sw, swx, swxx = w.sum(-1), (w * x).sum(-1), (w * x * x).sum(-1)
        swv, swxv = (w * v).sum(-1), (w * x * v).sum(-1)
        det = sw * swxx - swx * swx
        det = torch.where(nuse >= 2, det, torch.ones_like(det))
        a, b = (sw * swxv - swx * swv) / det, (swxx * swv - swx * swxv) / det
        zero = torch.zeros_like(a)
        flat = swv / sw.clamp(min=1e-300)
        through = swxv / swxx.clamp(min=1e-300)
        neg_a, neg_b = a < 0, (a >= 0) & (b < 0)
        a, b = torch.where(neg_a, zero, torch.where(neg_b, through, a)), torch.where(neg_a, flat, torch.where(neg_b, zero, b))
        return a, b

    a, b = solve(v)
    for _ in range(int(iters)):
        a, b = solve(a[..., None] * x + b[..., None])
    one = torch.where(use, v, torch.zeros_like(v)).sum(-1)              # the usable bin's variance where there is one
    fb = torch.zeros_like(one) if fallback is None else torch.as_tensor(fallback, dtype=torch.float64, device=v.device).expand_as(one)
    a = torch.where(nuse >= 2, a, torch.zeros_like(a))
    b = torch.where(nuse >= 2, b, torch.where(nuse == 1, one, fb))
    return a, b


def nlf_fit(y, bins=32, lo=0.0, hi=1.0, min_count=64, iters=2, pool_frames=False):
    """The noise-level function var(y | x) = a x + b of Poisson-Gaussian noise, blind: (a, b), float32, each (N,1,1,1)
    for y (N,C,H,W) and (N,1,D,1,1) for a clip (N,C,D,H,W), a fit per frame, or (N,1,1,1,1) with pool_frames, one fit
    for the clip.  nlf_bins, then nlf_fit_bins with the square of the image's MAD estimate (nle_mad) where no bin is
    usable.  a, b >= 0.  In y's scale (b a variance, a a variance per unit of intensity); no copy to the host, no
    synchronisation."""
    bins, lo, hi = _nlf_args(bins, lo, hi)
    imgs, _, lead = _nlf_images(y, pool_frames, "nlf_fit")
    sigma, count = _nlf_bins(imgs, bins, lo, hi)
    centre = _nlf_centres(bins, lo, hi, imgs.device)
    mad = nle_mad(imgs).reshape(-1)
    a, b = nlf_fit_bins(sigma, count, centre, min_count, iters, fallback=mad.double() ** 2)
    shape = lead + (1, 1)
    return a.float().reshape(shape), b.float().reshape(shape)


def nlf_map(y, a=None, b=None, s=1, smooth=7, floor=1e-3, **fit_kw):
    """A blind noise-level map for signal-dependent noise, `net(y, 255 * nlf_map(y, s=net.s))`: the noise-level function
    (a, b) -- given, or fitted by nlf_fit(y, **fit_kw) when a is None -- evaluated on the local intensity,
    sigma_img = sqrt(max(a m + b, floor^2)) with m the channel mean of y smoothed by a `smooth` x `smooth` box (odd;
    reflect padding) at the image grid, then taken to the code grid of a stride-`s` net by utils.sigma_to_code_grid.
    y (N,C,H,W) gives (N,1,ceil(H/s),ceil(W/s)), a clip (N,C,D,H,W) a map per frame on the clip's code grid.  In y's
    scale; thin torch ops, no copy to the host, no synchronisation."""
    if int(smooth) != smooth or smooth < 1 or smooth % 2 == 0:
        raise ValueError(f"smooth {smooth!r}: expected an odd integer >= 1")
    if (a is None) != (b is None):
        raise ValueError("a and b are given together or not at all")
    if a is None:
        a, b = nlf_fit(y, **fit_kw)
    elif fit_kw:
        raise TypeError(f"nlf_map: {sorted(fit_kw)} belong to the fit, but a and b were given")
    imgs, lead = _frames(y, "nlf_map")                               # a clip: its frames, (N*D, C, H, W)
    H, W = imgs.shape[-2:]
    r = int(smooth) // 2
    if r >= min(H, W):
        raise ValueError(f"smooth {smooth}: the reflect padding needs an image larger than {r} pixels")
    m = imgs.mean(dim=1, keepdim=True)
    if r:
        m = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(m, (r, r, r, r), mode="reflect"), int(smooth), stride=1)
    m = m.reshape(lead + (H, W))
    var = a * m + b                                                   # numbers, or device tensors that broadcast
    return utils.sigma_to_code_grid(var.clamp(min=float(floor) ** 2).sqrt().float(), s)


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


# ------------------------------------------------------------- weak-texture PCA per region
def _pca_grid(y, window, step, patchsize, name):
    """Checked (images (B,C,H,W), leading shape, window, step, p) of a cells call; every refusal is made here, before
    any device work.  window None: the whole frame is one cell."""
    if not torch.is_tensor(y):
        raise TypeError(f"{name}: expected a tensor")
    if y.dim() not in (4, 5):
        raise ValueError(f"{name} expects (N, C, H, W) or (N, C, D, H, W)")
    p = int(patchsize)
    if p != patchsize or not 3 <= p <= 11:
        raise ValueError(f"{name}: patchsize {patchsize!r} outside 3..11")
    H, W = y.shape[-2:]
    if H < p or W < p:
        raise ValueError(f"{name}: image {H} x {W} smaller than the {p} x {p} patch")
    if window is None:
        window = step = max(H, W)
    if int(window) != window or window < p:
        raise ValueError(f"{name}: window {window!r}: expected an integer >= patchsize {p} (pixels)")
    step = int(window) // 2 if step is None else step
    if int(step) != step or step < 1:
        raise ValueError(f"{name}: step {step!r}: expected an integer >= 1 (pixels)")
    y = ops._dev(y, "y")
    if y.dim() == 4:
        lead = tuple(y.shape[:2])
    else:
        lead = (y.shape[0], y.shape[1], y.shape[2])
        y = y.transpose(1, 2).reshape((-1, y.shape[1]) + tuple(y.shape[3:]))      # frames are samples: never mixed
    return y.contiguous(), lead, int(window), int(step), p


def pca_gram_cells(y, channel, patchsize, window, step, tau):
    """One pass over every cell on the device (cdl_nle_pca_gram_cells): (G (B, ny, nx, p^2, p^2) float64, count
    (B, ny, nx) int64) for images y (B,C,H,W), cells of `window` pixels `step` apart by the rule of cell_starts; a
    cell's G sums x x^T over the patches wholly inside it whose texture strength is below the cell's own
    tau (B, ny, nx) (float32, on the device; +inf keeps every patch).  No copy to the host."""
    B, C, H, W = y.shape
    ny, nx = len(cell_starts(H, window, step)), len(cell_starts(W, window, step))
    n = int(_lib.lib().cdl_nle_pca_gram_cells_scratch_floats(B, C, H, W, patchsize, window, step))
    if n == 0:
        raise ValueError(f"nle_pca_cells: patchsize {patchsize}, window {window}, step {step} refused for {H} x {W}")
    if tuple(tau.shape) != (B, ny, nx) or tau.dtype != torch.float32:
        raise ValueError(f"tau: expected float32 {(B, ny, nx)}")
    scratch = ops._scratch(y.device, n)
    P2 = patchsize * patchsize
    gram = torch.empty((B, ny, nx, P2, P2), device=y.device, dtype=torch.float64)
    count = torch.empty((B, ny, nx), device=y.device, dtype=torch.int64)
    ops._call("cdl_nle_pca_gram_cells", y, B, C, H, W, channel, patchsize, window, step, tau, gram, count, scratch, n)
    return gram, count


def _smallest_eigenvalues(cov):
    """Smallest eigenvalue of every matrix of cov (..., n, n) float64, by the device's batched symmetric solver: no
    Gram leaves the device.  (torch reads the solver's status back, one host synchronisation per pass; DESIGN.md
    section 25.)"""
    return torch.linalg.eigvalsh(cov)[..., 0]


def _pca_cells(imgs, window, step, p, conf, itr):
    """(sig2, th, num) float64 (B, C, ny, nx) on the device: the steps of nle_pca for every cell at once."""
    B, C, H, W = imgs.shape
    ny, nx = len(cell_starts(H, window, step)), len(cell_starts(W, window, step))
    total = (min(window, H) - p + 1) * (min(window, W) - p + 1)          # patches of a cell: the same for all
    tau0 = pca_constants(p, conf)[0]
    f64 = dict(device=imgs.device, dtype=torch.float64)
    if total < p * p:                   # sig2 = 0: the first refinement's tau = 0 keeps nothing and stops the cell
        zero = torch.zeros((B, C, ny, nx), **f64)
        if itr > 2:
            return zero, zero.clone(), zero.clone()
        return zero, torch.full_like(zero, math.inf), torch.full_like(zero, float(total))
    P2 = p * p
    out = []
    for c in range(C):
        tau = torch.full((B, ny, nx), math.inf, **f64)
        gram, kept = pca_gram_cells(imgs, c, p, window, step, tau.float())
        sig2 = _smallest_eigenvalues(gram / (kept - 1)[..., None, None])
        alive = torch.ones_like(kept, dtype=torch.bool)
        for _ in range(2, itr):
            tau = torch.where(alive, sig2 * tau0, tau)
            gram, cnt = pca_gram_cells(imgs, c, p, window, step, tau.float())
            kept = torch.where(alive, cnt, kept)
            alive = alive & (cnt >= P2)                  # a cell that keeps fewer than p^2 patches stops here
            eig = _smallest_eigenvalues(gram / (cnt - 1).clamp(min=1)[..., None, None])
            sig2 = torch.where(alive, eig, sig2)
        out.append((sig2, tau, kept.double()))
    return tuple(torch.stack([o[i] for o in out], dim=1) for i in range(3))


def nle_pca_cells(y, window=64, step=None, patchsize=7, conf=1 - 1e-6, itr=3):
    """The weak-texture PCA estimate of nle_pca over windows of the image: (nlevel, th, num), float64 device tensors,
    one value per channel and cell -- (N, C, ny, nx) for y (N,C,H,W), (N, C, D, ny, nx) for a clip (N,C,D,H,W), every
    frame on its own.  Cells are `window` x `window` pixels, `step` apart (default window // 2), the last of an axis
    flush with the border, an axis no longer than the window one cell (cell_starts, in pixels); window=None is the
    whole frame as one cell per sample.

    Every cell is its own domain and follows the steps of nle_pca on its crop: only the (window - p + 1)^2 patches
    wholly inside it, samples never pooled; the first pass keeps every patch, then for _ in range(2, itr):
    tau = sig2 * tau0, keep Xtr < tau; a cell whose kept count falls below p^2 stops there with its previous sig2 and
    reports the tau and the count that stopped it; fewer than p^2 patches in a cell give (0, 0, 0).  The Gram
    matrices of all cells form in one launch chain per pass and channel (cdl_nle_pca_gram_cells); the refinement is
    vectorised over cells with device masks.  In y's scale."""
    imgs, lead, window, step, p = _pca_grid(y, window, step, patchsize, "nle_pca_cells")
    sig2, th, num = _pca_cells(imgs, window, step, p, conf, int(itr))
    out = (sig2.sqrt(), th, num)
    if len(lead) == 3:                                   # (N*D, C, ny, nx) -> (N, C, D, ny, nx)
        out = tuple(t.reshape((lead[0], lead[2]) + tuple(t.shape[1:])).transpose(1, 2).contiguous() for t in out)
    return out


def _pca_levels(y, window, step, patchsize, conf, itr, name):
    """(levels (B, ny, nx) float64: the root mean square over channels of the cells' estimates, images' shape info)."""
    imgs, lead, window, step, p = _pca_grid(y, window, step, patchsize, name)
    sig2 = _pca_cells(imgs, window, step, p, conf, int(itr))[0]
    return sig2.mean(dim=1).clamp(min=0.0).sqrt(), imgs, lead, window, step     # a flat cell's eigenvalue may round below 0


def nle_pca_frames(clip, patchsize=7, conf=1 - 1e-6, itr=3):
    """One weak-texture PCA estimate per frame of a clip (N,C,D,H,W): (N,1,D,1,1) float32, the root mean square over
    channels of the frame's whole-image levels; the per-frame form of `sigma` the nets take (times 255)."""
    if not torch.is_tensor(clip) or clip.dim() != 5:
        raise ValueError("nle_pca_frames expects (N, C, D, H, W)")
    lev, _, lead, _, _ = _pca_levels(clip, None, None, patchsize, conf, itr, "nle_pca_frames")
    return lev.float().reshape(lead[0], 1, lead[2], 1, 1)


@functools.lru_cache(maxsize=64)
def _pca_interp_plan(L, window, step, device):
    """(lo, hi, t) on `device` for one axis of L pixels: pixel x takes (1 - t) * cell[lo] + t * cell[hi], piecewise
    linear between the cell centres r0 + (w - 1) / 2, constant beyond the first and the last.  Device ops only."""
    w = min(window, L)
    n = len(cell_starts(L, window, step))
    r0 = (torch.arange(n, device=device) * step).clamp(max=L - w)
    centre = r0.double() + (w - 1) / 2
    x = torch.arange(L, device=device, dtype=torch.float64)
    hi = torch.bucketize(x, centre).clamp(max=n - 1)            # first centre >= x
    lo = (hi - 1).clamp(min=0)
    gap = centre[hi] - centre[lo]
    t = torch.where(gap > 0, (x - centre[lo]) / gap.clamp(min=0.5), torch.zeros_like(x)).clamp(0.0, 1.0)
    return lo, hi, t


def _pca_interpolate(cells, H, W, window, step):
    """cells (B, ny, nx) float64 -> (B, H, W) float64, separable."""
    lo, hi, t = _pca_interp_plan(H, window, step, cells.device)
    rows = torch.lerp(cells.index_select(1, lo), cells.index_select(1, hi), t[:, None])
    lo, hi, t = _pca_interp_plan(W, window, step, cells.device)
    return torch.lerp(rows.index_select(2, lo), rows.index_select(2, hi), t)


def nle_pca_map(y, window=64, step=None, s=1, patchsize=7, conf=1 - 1e-6, itr=3):
    """A blind noise-level map for `net(y, 255 * nle_pca_map(y, s=net.s))` from the weak-texture PCA estimate, which
    texture inside a window does not inflate as it does the MAD estimate of nle_mad_map: the cell levels of
    nle_pca_cells (root mean square over channels) interpolated to the image grid (separable, piecewise linear
    between the cell centres r0 + (window - 1) / 2, constant beyond the outermost), then taken to the code grid of a
    stride-`s` net by utils.sigma_to_code_grid.  float32; y (N,C,H,W) gives (N,1,ceil(H/s),ceil(W/s)), a clip
    (N,C,D,H,W) a map per frame on the clip's code grid.  window=None is one level per image (N,1,1,1) or per frame,
    nle_pca_frames(y) (N,1,D,1,1).  In y's scale."""
    if window is None:
        if torch.is_tensor(y) and y.dim() == 5:
            return nle_pca_frames(y, patchsize, conf, itr)
        lev, _, lead, _, _ = _pca_levels(y, None, None, patchsize, conf, itr, "nle_pca_map")
        return lev.float().reshape(lead[0], 1, 1, 1)
    lev, imgs, lead, window, step = _pca_levels(y, window, step, patchsize, conf, itr, "nle_pca_map")
    H, W = imgs.shape[-2:]
    img_map = _pca_interpolate(lev, H, W, window, step).float()
    return utils.sigma_to_code_grid(img_map.reshape((lead[0], 1) + tuple(lead[2:]) + (H, W)), s)


def noise_level_map(y, method="MAD", **kwargs):
    """The one dispatcher of the two blind map estimators: nle_mad_map(y, **kwargs) for "MAD", nle_pca_map(y, **kwargs)
    for "PCA".  (noise_level itself stays the MAD estimate of a whole image.)"""
    if method == "MAD":
        return nle_mad_map(y, **kwargs)
    if method == "PCA":
        return nle_pca_map(y, **kwargs)
    raise NotImplementedError(f"noise_level_map method {method!r}: expected 'MAD' or 'PCA'")


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
