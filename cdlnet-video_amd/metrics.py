"""SSIM on the device: the evaluation metric and the differentiable loss term of the reference's pipeline.

* `ssim(X, Y, ...)`: pytorch_msssim's `ssim` for (N, C, H, W), differentiable in X, Y and data_range (the SSIM
  term of loss.py's CombinedLossWithSSIM is built on it);
* `ssim_frames(output, target)`: that term for (N, C, D, H, W) clips, every frame in one launch;
* `ms_ssim(X, Y, ...)`: pytorch_msssim's `ms_ssim` (multi-scale SSIM) for (N, C, H, W), differentiable in X, Y and
  data_range; `ms_ssim_frames(output, target)`: mean_t (1 - ms_ssim) of the frames of (N, C, D, H, W) clips, all
  frames in one pyramid (`cdl_msssim_fwd` / `cdl_msssim_bwd`: the SSIM kernels, two launches per level);
* `structural_similarity(x, y, ...)`: skimage's `structural_similarity` (analyzemri.py's metric), per plane;
* `video_ssim(video, denoised)`: analyzemri.py's `ssim_total / frame_count` for one batch, one host sync;
* `perceptual_frames(output, target, weights)`: the VGG16 relu3_3 perceptual term of CombinedLossWithSSIM for
  (N, 1, D, H, W) clips, differentiable in both (`cdl_vgg_forward` / `cdl_vgg_backward`, csrc/cdl_vgg.hip);
  `vgg16_features(frames, weights)`: the relu3_3 features themselves.

The per-plane means of the SSIM map and their reverse sweep run in libcdlnet_hip.so (`cdl_ssim_fwd` /
`cdl_ssim_bwd`, csrc/cdl_ssim.hip).  The host builds the 1-D window and passes it by value; data_range is a device
tensor of one value per plane, so nothing on these paths copies from the device or synchronises.
"""
import ctypes
import math

import torch

from . import _lib, ops

_TAPS_MAX = 15


def _gaussian_window(win_size, win_sigma):
    """pytorch_msssim's _fspecial_gauss_1d: exp(-(i - win_size // 2)^2 / (2 sigma^2)), normalised (in float32, as
    pytorch_msssim builds it)."""
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    return (g / g.sum()).tolist()


def _check_window(win_size, H, W):
    if win_size % 2 != 1 or win_size < 3:
        raise ValueError(f"win_size must be odd and at least 3, got {win_size}")
    if win_size > _TAPS_MAX:
        raise ValueError(f"win_size {win_size}: the device kernel takes windows of up to {_TAPS_MAX} taps")
    if H < win_size or W < win_size:
        raise ValueError(f"win_size {win_size} exceeds the image extent {H} x {W}")


def _window_arg(win):
    return (ctypes.c_float * len(win))(*win)


def _planes_range(data_range, P, like):
    """data_range (number or tensor broadcastable to the P planes) -> contiguous float32 device tensor (P,)."""
    if torch.is_tensor(data_range):
        r = data_range.to(device=like.device, dtype=torch.float32)
        return r.reshape(()).expand(P).contiguous() if r.numel() == 1 else r.reshape(P).contiguous()
    return torch.full((P,), float(data_range), device=like.device, dtype=torch.float32)


class _SSIMPlanes(torch.autograd.Function):
    """(x, y, R) of P planes (P, H, W), R (P,) -> per-plane mean of the SSIM map (P,)."""

    @staticmethod
    def forward(ctx, x, y, R, win, K1, K2, kappa):
        P, H, W = x.shape
        if R.shape != (P,):
            raise ValueError(f"data_range: expected one value per plane, shape ({P},), got {tuple(R.shape)}")
        R = R.contiguous()          # the kernels read R[plane]: an expanded (stride-0) view must not reach them
        n = int(_lib.lib().cdl_ssim_scratch_floats(P, H, W, len(win)))
        scratch = ops._scratch(x.device, n)
        out = torch.empty(P, device=x.device, dtype=torch.float32)
        ops._call("cdl_ssim_fwd", x, y, P, H, W, _window_arg(win), len(win), K1, K2, kappa, R, out, None, scratch, n)
        ctx.save_for_backward(x, y, R)
        ctx.args = (win, K1, K2, kappa)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, R = ctx.saved_tensors
        win, K1, K2, kappa = ctx.args
        nx, ny, nr = ctx.needs_input_grad[:3]
        if not (nx or ny or nr):
            return (None,) * 7
        P, H, W = x.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if nx else None
        dy = torch.empty_like(y) if ny else None
        dr = torch.empty(P, device=x.device, dtype=torch.float32) if nr else None
        n = int(_lib.lib().cdl_ssim_scratch_floats(P, H, W, len(win)))
        scratch = ops._scratch(x.device, n)
        ops._call("cdl_ssim_bwd", x, y, P, H, W, _window_arg(win), len(win), K1, K2, kappa, R, g, dx, dy, dr, scratch, n)
        return dx, dy, dr, None, None, None, None


def _plane_ssim(x, y, R, win, K1, K2, kappa):
    """x, y (..., H, W) device float32, R (P,) -> per-plane SSIM means shaped like the leading dims."""
    lead, (H, W) = x.shape[:-2], x.shape[-2:]
    P = math.prod(lead)
    with torch.cuda.device(x.device):
        out = _SSIMPlanes.apply(x.reshape(P, H, W), y.reshape(P, H, W), R, win, float(K1), float(K2), float(kappa))
    return out.reshape(lead)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """pytorch_msssim.ssim for 4-D (N, C, H, W) input: Gaussian window (win_size, win_sigma), valid filtering.

    Returns ssim_per_channel.mean(), or .mean(1) per image when size_average=False.  Differentiable in X, Y and
    data_range (a python number or a tensor, e.g. `out.max() - out.min()`).

    Deviations from pytorch_msssim, both raised before any device work:
    * a spatial side smaller than the window raises ValueError (pytorch_msssim warns and skips that axis);
    * 5-D input raises NotImplementedError (pytorch_msssim would switch to a 3-D window): per-frame SSIM of a clip is
      `ssim_frames`.
    """
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("ssim: expected tensors")
    if X.shape != Y.shape:
        raise ValueError(f"input images should have the same dimensions, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.dim() == 5:
        raise NotImplementedError("ssim takes (N, C, H, W); pytorch_msssim's 3-D window for 5-D input is not "
                                  "implemented -- for the per-frame SSIM of (N, C, D, H, W) clips use ssim_frames")
    if X.dim() != 4:
        raise ValueError(f"expected 4-D (N, C, H, W) input, got {tuple(X.shape)}")
    _check_window(win_size, X.shape[-2], X.shape[-1])
    X, Y = ops._dev(X, "X"), ops._dev(Y, "Y")
    N, C = X.shape[:2]
    win = _gaussian_window(win_size, win_sigma)
    R = _planes_range(data_range, N * C, X)
    per_channel = _plane_ssim(X, Y, R, win, K[0], K[1], 1.0)
    if nonnegative_ssim:
        per_channel = torch.relu(per_channel)
    return per_channel.mean() if size_average else per_channel.mean(1)


def _frames_range(output, data_range):
    """data_range of the (n, c, t) planes of a clip (N, C, D, H, W) on the device, (N * C * D,): None is the per-frame
    max - min of `output`, a number or a tensor broadcastable to (D,) is used as given."""
    N, C, D = output.shape[:3]
    if data_range is None:
        R_t = output.amax(dim=(0, 1, 3, 4)) - output.amin(dim=(0, 1, 3, 4))
    elif torch.is_tensor(data_range):
        r = data_range.to(device=output.device, dtype=torch.float32)
        R_t = r.reshape(()).expand(D) if r.numel() == 1 else r.reshape(D)
    else:
        R_t = torch.full((D,), float(data_range), device=output.device, dtype=torch.float32)
    return R_t.reshape(1, 1, D).expand(N, C, D).contiguous().reshape(-1)


def ssim_frames(output, target, data_range=None):
    """The SSIM term of loss.py's CombinedLossWithSSIM for (N, C, D, H, W) clips:
    mean_t (1 - ssim(output[:, :, t], target[:, :, t], data_range=R_t)), pytorch_msssim's defaults otherwise.

    data_range=None is the reference's R_t = output[:, :, t].max() - output[:, :, t].min() (over N and C, output only;
    the gradient reaches the max / min elements as torch's max() / min() send it, split evenly among ties).  A number
    or a tensor broadcastable to (D,) is used as given.

    The reference repeats every frame to three channels first (`repeat(1, 3, 1, 1)`).  That changes nothing: the
    three copies have the same SSIM, so their mean is the one-channel value and the same max / min; in the reverse
    pass each copy receives a third of the gradient and repeat's backward adds the three thirds.  All frames run in
    one forward and one backward launch, with no host synchronisation.
    """
    if not (torch.is_tensor(output) and torch.is_tensor(target)):
        raise TypeError("ssim_frames: expected tensors")
    if output.shape != target.shape:
        raise ValueError(f"input clips should have the same dimensions, got {tuple(output.shape)} and "
                         f"{tuple(target.shape)}")
    if output.dim() != 5:
        raise ValueError(f"ssim_frames expects (N, C, D, H, W), got {tuple(output.shape)}")
    _check_window(11, output.shape[-2], output.shape[-1])
    output, target = ops._dev(output, "output"), ops._dev(target, "target")
    R = _frames_range(output, data_range)
    per_plane = _plane_ssim(output, target, R, _gaussian_window(11, 1.5), 0.01, 0.03, 1.0)   # (N, C, D)
    ssim_t = per_plane.mean(dim=(0, 1))
    return (1 - ssim_t).mean()


# ------------------------------------------------------------------------------ MS-SSIM (pytorch_msssim's ms_ssim)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_LEVELS_MAX = 8


def _level_sizes(H, W, levels):
    """[(H_i, W_i)] of the pyramid: avg_pool2d(kernel 2, padding [H % 2, W % 2]) halves an axis rounding up."""
    out = []
    for _ in range(levels):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def _ms_weights(weights):
    w = list(MS_WEIGHTS) if weights is None else [float(v) for v in weights]
    if not 1 <= len(w) <= _LEVELS_MAX:
        raise ValueError(f"weights: expected 1 to {_LEVELS_MAX} levels, got {len(w)}")
    return w


def _check_pyramid(win_size, H, W, levels):
    _check_window(win_size, H, W)
    h, w = _level_sizes(H, W, levels)[-1]
    if min(h, w) < win_size:
        raise ValueError(f"image {H} x {W}: level {levels - 1} of the pyramid is {h} x {w}, smaller than win_size "
                         f"{win_size}; the smaller side should be larger than (win_size - 1) * 2**{levels - 1} = "
                         f"{(win_size - 1) * 2 ** (levels - 1)}")


class _MSSSIMPlanes(torch.autograd.Function):
    """(x, y, R) of P planes (P, H, W), R (P,) -> the (levels, P, 2) table of the raw per-plane means (ssim_i, cs_i) of
    every level of the 2x2 average-pooling pyramid.  Saves the pooled planes of both sides (a third of the input
    again) for the backward, which takes the gradient of the whole table."""

    @staticmethod
    def forward(ctx, x, y, R, win, K1, K2, levels):
        P, H, W = x.shape
        if R.shape != (P,):
            raise ValueError(f"data_range: expected one value per plane, shape ({P},), got {tuple(R.shape)}")
        R = R.contiguous()
        lib = _lib.lib()
        n = int(lib.cdl_msssim_scratch_floats(P, H, W, len(win), levels))
        if n == 0:
            raise ValueError(f"ms_ssim: {levels} levels of {H} x {W} planes with a {len(win)}-tap window not supported")
        npyr = int(lib.cdl_msssim_pyramid_floats(P, H, W, levels))
        scratch = ops._scratch(x.device, n)
        pyr_x = torch.empty(npyr, device=x.device, dtype=torch.float32) if levels > 1 else None
        pyr_y = torch.empty(npyr, device=x.device, dtype=torch.float32) if levels > 1 else None
        vals = torch.empty((levels, P, 2), device=x.device, dtype=torch.float32)
        ops._call("cdl_msssim_fwd", x, y, P, H, W, _window_arg(win), len(win), K1, K2, R, levels, pyr_x, pyr_y, vals,
                  scratch, n)
        ctx.save_for_backward(x, y, R, pyr_x, pyr_y)
        ctx.args = (win, K1, K2, levels, npyr)
        return vals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, y, R, pyr_x, pyr_y = ctx.saved_tensors
        win, K1, K2, levels, npyr = ctx.args
        nx, ny, nr = ctx.needs_input_grad[:3]
        if not (nx or ny or nr):
            return (None,) * 7
        P, H, W = x.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if nx else None
        dy = torch.empty_like(y) if ny else None
        dr = torch.empty(P, device=x.device, dtype=torch.float32) if nr else None
        work = torch.empty(2 * npyr, device=x.device, dtype=torch.float32) if levels > 1 and (nx or ny) else None
        n = int(_lib.lib().cdl_msssim_scratch_floats(P, H, W, len(win), levels))
        scratch = ops._scratch(x.device, n)
        ops._call("cdl_msssim_bwd", x, y, pyr_x, pyr_y, P, H, W, _window_arg(win), len(win), K1, K2, R, levels, g, dx, dy,
                  dr, work, scratch, n)
        return dx, dy, dr, None, None, None, None


def _plane_ms_ssim(x, y, R, win, K1, K2, weights):
    """x, y (..., H, W) device float32, R (P,) -> per-plane MS-SSIM shaped like the leading dims.  The combination is
    pytorch_msssim's, in torch ops on the (levels, P) means: relu, powers, product -- the product as L - 1
    multiplications in level order, because torch.prod's backward counts zeros on the host (a synchronisation)."""
    lead, (H, W) = x.shape[:-2], x.shape[-2:]
    P = math.prod(lead)
    L = len(weights)
    with torch.cuda.device(x.device):
        vals = _MSSSIMPlanes.apply(x.reshape(P, H, W), y.reshape(P, H, W), R, win, float(K1), float(K2), L)
    v = torch.relu(torch.cat([vals[:-1, :, 1], vals[-1:, :, 0]]))               # cs of the finer levels, ssim of the last
    ms = v[0] ** weights[0]
    for i in range(1, L):
        ms = ms * v[i] ** weights[i]
    return ms.reshape(lead)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim for 4-D (N, C, H, W) input: with L = len(weights) levels (default
    [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]), level i + 1 = avg_pool2d(level i, 2, padding=[H_i % 2, W_i % 2]),
        ms = prod_i relu(v_i) ** weights_i,   v_i = cs mean of level i for i < L - 1, SSIM mean of level L - 1,
    per (n, c); returns ms.mean(), or ms.mean(1) per image when size_average=False.  Differentiable (once) in X, Y and
    data_range (a python number or a tensor).  `weights`: a sequence of python numbers (or a CPU tensor).

    Raised before any device work: the refusals of `ssim` (a side smaller than the window, 5-D input -- per-frame
    MS-SSIM of (N, C, D, H, W) clips is `ms_ssim_frames`), and ValueError when the coarsest level's smaller side is below
    win_size.  For five levels that is exactly pytorch_msssim's assertion `smaller_side > (win_size - 1) * 2**4`: an axis
    of length s has ceil(s / 2**k) pixels at level k, and ceil(s / 2**k) >= win_size is s > (win_size - 1) * 2**k; the
    same rule is applied for any number of levels (1 to 8).
    """
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("ms_ssim: expected tensors")
    if X.shape != Y.shape:
        raise ValueError(f"input images should have the same dimensions, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.dim() == 5:
        raise NotImplementedError("ms_ssim takes (N, C, H, W); pytorch_msssim's 3-D window for 5-D input is not "
                                  "implemented -- for the per-frame MS-SSIM of (N, C, D, H, W) clips use ms_ssim_frames")
    if X.dim() != 4:
        raise ValueError(f"expected 4-D (N, C, H, W) input, got {tuple(X.shape)}")
    weights = _ms_weights(weights)
    _check_pyramid(win_size, X.shape[-2], X.shape[-1], len(weights))
    X, Y = ops._dev(X, "X"), ops._dev(Y, "Y")
    N, C = X.shape[:2]
    R = _planes_range(data_range, N * C, X)
    ms = _plane_ms_ssim(X, Y, R, _gaussian_window(win_size, win_sigma), K[0], K[1], weights)    # (N, C)
    return ms.mean() if size_average else ms.mean(1)


def ms_ssim_frames(output, target, data_range=None, weights=None):
    """mean_t (1 - ms_ssim(output[:, :, t], target[:, :, t], data_range=R_t)) for (N, C, D, H, W) clips, pytorch_msssim's
    defaults otherwise: the multi-scale sibling of `ssim_frames`, with its data_range semantics (None: R_t =
    output[:, :, t].max() - output[:, :, t].min(); a number or a tensor broadcastable to (D,) is used as given).  All
    N * C * D planes go through one pyramid, with no host synchronisation."""
    if not (torch.is_tensor(output) and torch.is_tensor(target)):
        raise TypeError("ms_ssim_frames: expected tensors")
    if output.shape != target.shape:
        raise ValueError(f"input clips should have the same dimensions, got {tuple(output.shape)} and "
                         f"{tuple(target.shape)}")
    if output.dim() != 5:
        raise ValueError(f"ms_ssim_frames expects (N, C, D, H, W), got {tuple(output.shape)}")
    weights = _ms_weights(weights)
    _check_pyramid(11, output.shape[-2], output.shape[-1], len(weights))
    output, target = ops._dev(output, "output"), ops._dev(target, "target")
    R = _frames_range(output, data_range)
    ms = _plane_ms_ssim(output, target, R, _gaussian_window(11, 1.5), 0.01, 0.03, weights)        # (N, C, D)
    return (1 - ms.mean(dim=(0, 1))).mean()


# ------------------------------------------------------------------------------ perceptual term (VGG16 relu3_3)
VGG_CONVS = (0, 2, 5, 7, 10, 12, 14)            # torchvision's vgg16().features indices of the seven convolutions
VGG_SHAPES = {0: (64, 3), 2: (64, 64), 5: (128, 64), 7: (128, 128), 10: (256, 128), 12: (256, 256), 14: (256, 256)}
_VGG_DX, _VGG_DY = 1, 2


def vgg16_state(sd):
    """The seven convolutions of VGG16 features[:16] from a state dict in any of three key layouts -- torchvision's
    `features.N.*` (`classifier.*` and the deeper layers ignored), the reference loss module's `vgg.N.*`, bare `N.*` --
    as {"N.weight", "N.bias"} float32 tensors, shapes checked."""
    out = {}
    for key, v in sd.items():
        parts = key.split(".")
        if parts[0] in ("features", "vgg"):
            parts = parts[1:]
        if len(parts) != 2 or not parts[0].isdigit() or parts[1] not in ("weight", "bias"):
            continue
        if int(parts[0]) in VGG_CONVS:
            out[f"{int(parts[0])}.{parts[1]}"] = v
    for i in VGG_CONVS:
        o, c = VGG_SHAPES[i]
        for name, shape in (("weight", (o, c, 3, 3)), ("bias", (o,))):
            k = f"{i}.{name}"
            if k not in out:
                raise KeyError(f"VGG16 weights: {k} (or features.{k} / vgg.{k}) missing")
            if tuple(out[k].shape) != shape:
                raise ValueError(f"VGG16 weights: {k} has shape {tuple(out[k].shape)}, expected {shape}")
            out[k] = out[k].detach().to(torch.float32)
    return {f"{i}.{n}": out[f"{i}.{n}"] for i in VGG_CONVS for n in ("weight", "bias")}


def _vgg_tables(weights, device):
    sd = vgg16_state(weights)
    ws = [sd[f"{i}.weight"].to(device).contiguous() for i in VGG_CONVS]
    bs = [sd[f"{i}.bias"].to(device).contiguous() for i in VGG_CONVS]
    return ws, bs


def _check_planes(H, W):
    if H < 4 or W < 4:
        raise ValueError(f"the VGG16 features need frames of at least 4 x 4, got {H} x {W}")


class _PerceptualPlanes(torch.autograd.Function):
    """(x, y) of P planes (P, H, W) -> mean over all relu3_3 elements of (F(x) - F(y))^2, one forward and one backward
    call into libcdlnet_hip.so (cdl_vgg_forward / cdl_vgg_backward).  The scratch holds the activations the backward
    gates on, so it is owned by this call (not the shared per-stream scratch)."""

    @staticmethod
    def forward(ctx, x, y, ws, bs):
        P, H, W = x.shape
        grads = (_VGG_DX if ctx.needs_input_grad[0] else 0) | (_VGG_DY if ctx.needs_input_grad[1] else 0)
        n = int(_lib.lib().cdl_vgg_scratch_floats(P, H, W, grads))
        if n == 0:
            raise ValueError(f"perceptual loss: {P} planes of {H} x {W} not supported")
        scratch = torch.empty(n, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        ops._call("cdl_vgg_forward", x, y, P, H, W, ws, bs, grads, None, loss, scratch, n)
        ctx.state = (scratch, ws, bs, grads, (P, H, W))
        return loss

    @staticmethod
    def backward(ctx, g):
        scratch, ws, bs, grads, (P, H, W) = ctx.state
        if not grads:
            return None, None, None, None
        g = g.to(torch.float32).contiguous()
        dx = torch.empty((P, H, W), device=g.device, dtype=torch.float32) if grads & _VGG_DX else None
        dy = torch.empty((P, H, W), device=g.device, dtype=torch.float32) if grads & _VGG_DY else None
        ops._call("cdl_vgg_backward", P, H, W, ws, bs, grads, g, dx, dy, scratch, scratch.numel())
        ctx.state = None
        return dx, dy, None, None


def perceptual_frames(output, target, weights):
    """The perceptual term of loss.py's CombinedLossWithSSIM for (N, 1, D, H, W) clips:
    (1/D) sum_t mean((F(o_t) - F(g_t))^2), F = VGG16 features[:16] (relu3_3) of the frame repeated to three channels.
    Every frame has the same number of features, so this is one mean over all N*D planes.  `weights`: a state dict
    in any layout `vgg16_state` reads.  Differentiable in output and target (not in the weights); one forward and one
    backward launch sequence, no host synchronisation."""
    if not (torch.is_tensor(output) and torch.is_tensor(target)):
        raise TypeError("perceptual_frames: expected tensors")
    if output.shape != target.shape:
        raise ValueError(f"input clips should have the same dimensions, got {tuple(output.shape)} and "
                         f"{tuple(target.shape)}")
    if output.dim() != 5:
        raise ValueError(f"perceptual_frames expects (N, 1, D, H, W), got {tuple(output.shape)}")
    if output.shape[1] != 1:
        raise ValueError(f"perceptual_frames takes one-channel clips (the reference repeats each frame to three "
                         f"channels; C = {output.shape[1]} would give {3 * output.shape[1]}), got {tuple(output.shape)}")
    H, W = output.shape[-2:]
    _check_planes(H, W)
    output, target = ops._dev(output, "output"), ops._dev(target, "target")
    P = math.prod(output.shape[:3])
    with torch.cuda.device(output.device):
        ws, bs = _vgg_tables(weights, output.device)
        return _PerceptualPlanes.apply(output.reshape(P, H, W), target.reshape(P, H, W), ws, bs)


def vgg16_features(frames, weights):
    """relu3_3 of VGG16 features[:16] for every one-channel (H, W) plane of `frames` (..., H, W), each repeated to
    three channels: (..., 256, H4, W4), H4 = floor(floor(H/2)/2).  Forward only."""
    if not torch.is_tensor(frames) or frames.dim() < 2:
        raise TypeError("vgg16_features: expected a tensor (..., H, W)")
    H, W = frames.shape[-2:]
    _check_planes(H, W)
    frames = ops._dev(frames, "frames")
    lead = frames.shape[:-2]
    P = math.prod(lead)
    H4, W4 = H // 2 // 2, W // 2 // 2
    with torch.cuda.device(frames.device):
        ws, bs = _vgg_tables(weights, frames.device)
        n = int(_lib.lib().cdl_vgg_scratch_floats(P, H, W, 0))
        if n == 0:
            raise ValueError(f"vgg16_features: {P} planes of {H} x {W} not supported")
        scratch = torch.empty(n, device=frames.device, dtype=torch.float32)
        feat = torch.empty((P, 256, H4, W4), device=frames.device, dtype=torch.float32)
        ops._call("cdl_vgg_forward", None, frames, P, H, W, ws, bs, 0, feat, None, scratch, n)
    return feat.reshape(*lead, 256, H4, W4)


def structural_similarity(x, y, data_range=1.0, win_size=7, K1=0.01, K2=0.03, channel_axis=None):
    """skimage.metrics.structural_similarity with its defaults (uniform window, use_sample_covariance=True, so
    kappa = n / (n - 1) with n = win_size^2), for every trailing (H, W) plane of x and y at once.

    skimage filters with reflect padding and then crops (win_size - 1) // 2 from every side before the mean: what
    remains are exactly the positions a valid filter produces, so the border mode never matters and the kernel filters
    "valid".  Returns a tensor shaped like the leading dims (0-d for one (H, W) image).  `channel_axis` (an axis of the
    leading dims) averages over it, as skimage does for a colour image.  Forward only, no gradient.
    """
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise TypeError("structural_similarity: expected tensors")
    if x.shape != y.shape:
        raise ValueError(f"input images must have the same dimensions, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dim() < 2:
        raise ValueError("structural_similarity expects (..., H, W)")
    if win_size % 2 != 1:
        raise ValueError("Window size must be odd.")
    if win_size > min(x.shape[-2:]):
        raise ValueError(f"win_size {win_size} exceeds the image extent {tuple(x.shape[-2:])}")
    _check_window(win_size, x.shape[-2], x.shape[-1])
    if channel_axis is not None and not (-(x.dim() - 2) <= channel_axis < x.dim() - 2):
        raise ValueError(f"channel_axis {channel_axis} is not a leading axis of {tuple(x.shape)}")
    x, y = ops._dev(x, "x"), ops._dev(y, "y")
    npx = win_size * win_size
    lead = x.shape[:-2]
    R = _planes_range(data_range, math.prod(lead), x)
    with torch.no_grad():
        out = _plane_ssim(x, y, R, [1.0 / win_size] * win_size, K1, K2, npx / (npx - 1.0))
    if channel_axis is not None:
        out = out.mean(dim=channel_axis)
    return out


def video_ssim(video, denoised, data_range=1.0):
    """analyzemri.py's SSIM for one batch (B, C, D, H, W): skimage's structural_similarity of every (b, d) frame,
    averaged over its channels for C > 1, summed and divided by the frame count B * D.  One launch and one host
    sync for the whole batch (the reference copies every frame to the host)."""
    if not (torch.is_tensor(video) and torch.is_tensor(denoised)):
        raise TypeError("video_ssim: expected tensors")
    if video.dim() != 5:
        raise ValueError(f"video_ssim expects (B, C, D, H, W), got {tuple(video.shape)}")
    per_plane = structural_similarity(denoised, video, data_range=data_range)       # (B, C, D)
    return float(per_plane.mean(dim=1).mean())
