"""The reference's CombinedLossWithSSIM (loss.py), used by its 3-D trainers with `fit(..., combmse=True)`:

    total = alpha * mean((output - target)^2) + beta * perceptual + gamma * ssim_loss

for (B, 1, T, H, W) clips, where `perceptual` is the mean squared difference of the VGG16 features[:16] (relu3_3) of
every frame repeated to three channels (`metrics.perceptual_frames`, HIP forward and backward) and `ssim_loss` is
mean_t (1 - SSIM) (`metrics.ssim_frames`).  Gradients reach `output` (and `target` when it requires them), never the
VGG weights.

The reference downloads the ImageNet weights (`vgg16(pretrained=True)`); nothing here downloads.  The weights come
from a local file or a state dict (`load_vgg16_weights`); by default the file torchvision's download would have left
under `torch.hub.get_dir()/checkpoints`.
"""
import os

import torch
import torch.nn as nn

from . import metrics

VGG16_FILE = "vgg16-397923af.pth"


def default_vgg16_path():
    return os.path.join(torch.hub.get_dir(), "checkpoints", VGG16_FILE)


def load_vgg16_weights(src):
    """The seven convolutions of VGG16 features[:16] as {"N.weight", "N.bias"} (N in 0, 2, 5, 7, 10, 12, 14) from a
    file path or a state dict with torchvision's keys (`features.N.*`; `classifier.*` ignored), the reference loss
    module's (`vgg.N.*`) or bare ones (`N.*`)."""
    if isinstance(src, (str, os.PathLike)):
        if not os.path.isfile(src):
            raise FileNotFoundError(f"VGG16 weights {src!s} not found (nothing is downloaded: pass vgg_weights= a local "
                                    f"copy of torchvision's {VGG16_FILE} or a state dict)")
        src = torch.load(src, map_location="cpu", weights_only=True)
    if not hasattr(src, "items"):
        raise TypeError("load_vgg16_weights: expected a file path or a state dict")
    return metrics.vgg16_state(src)


class _Conv(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.register_buffer("weight", weight.detach().clone())
        self.register_buffer("bias", bias.detach().clone())


class _VGG16Features(nn.Module):
    """Frozen buffers named like the reference module's `vgg` (features[:16]): `N.weight`, `N.bias` for the seven
    convolutions, so `state_dict()` keys match and `.to(device)` moves them."""

    def __init__(self, sd):
        super().__init__()
        for i in metrics.VGG_CONVS:
            self.add_module(str(i), _Conv(sd[f"{i}.weight"], sd[f"{i}.bias"]))

    def weights(self):
        return {f"{name}.{k}": v for name, mod in self.named_children() for k, v in mod.named_buffers()}


class CombinedLossWithSSIM(nn.Module):
    """alpha * MSE + beta * VGG16 perceptual + gamma * (1 - SSIM) for (B, 1, T, H, W) clips (the reference's
    defaults 1.0, 0.01, 0.1).  `vgg_weights`: a path or a state dict (`load_vgg16_weights`); None reads
    `default_vgg16_path()` and raises FileNotFoundError when it is missing.  beta == 0 needs no weights."""

    def __init__(self, alpha=1.0, beta=0.01, gamma=0.1, vgg_weights=None):
        super().__init__()
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        if beta != 0:
            sd = load_vgg16_weights(default_vgg16_path() if vgg_weights is None else vgg_weights)
            self.vgg = _VGG16Features(sd)
        else:
            self.vgg = None

    def forward(self, output, target):
        if not (torch.is_tensor(output) and torch.is_tensor(target)):
            raise TypeError("CombinedLossWithSSIM: expected tensors")
        if output.shape != target.shape:
            raise ValueError(f"output and target differ in shape: {tuple(output.shape)} and {tuple(target.shape)}")
        if output.dim() != 5:
            raise ValueError(f"CombinedLossWithSSIM expects (B, 1, T, H, W) clips, got {tuple(output.shape)}")
        if output.shape[1] != 1:
            raise ValueError(f"CombinedLossWithSSIM takes one-channel clips (the reference repeats each frame to three "
                             f"channels, which VGG16's first layer accepts only for C = 1), got {tuple(output.shape)}")
        metrics._check_window(11, output.shape[-2], output.shape[-1])
        mse = torch.mean((output - target) ** 2)
        ssim_loss = metrics.ssim_frames(output, target)
        if self.beta == 0:
            return self.alpha * mse + self.gamma * ssim_loss
        perceptual = metrics.perceptual_frames(output, target, self.vgg.weights())
        return self.alpha * mse + self.beta * perceptual + self.gamma * ssim_loss
