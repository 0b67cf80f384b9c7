"""Trainer-side restatement of the calls that drive the hot path.

`init_model` mirrors the reference's factory (train.py:180-219, train3d.py:174-206,
traincsr.py:281-302) so an `args.json` builds the same net + Adam + StepLR; `train_step` is the
body of the reference's batch loop (train.py:76-103 / train3d.py:90-118) with the data-parallel
gradient exchange added (parallel.py); `fit` is the reference's epoch driver (train.py:35-158: phases,
PSNR logs, divergence backtracking with learning-rate decay, checkpoint rotation, MC-SURE option) around
that step.  Data loading and plotting are outside the hot path and are not re-implemented here.
"""
import json
import os

import numpy as np
import torch
import torch.nn as nn

import torch.distributed as dist

from . import temporal
from .net import CDLNet, CDLNet_CSR, CDLNet_CSRf2, CDLNetVideo, GDLNet
from .parallel import phase_consensus
from .utils import awgn, gen_bayer_mask, sigma_to_code_grid

MODEL_TYPES = {
    "CDLNet": CDLNet,
    "JDD_CDLNet": CDLNet,          # BASELINE config 4: CDLNet with C=3 + Bayer mask
    "CDLNetVideo": CDLNetVideo,
    "GDLNet": GDLNet,
    "CDLNet_CSR": CDLNet_CSR,      # traincsr.py:290-296
    "CDLNet_CSRf2": CDLNet_CSRf2,
}


def build_model(args, init=None):
    """`Cls(**args['model'])` selected by args['type'] (train.py:184-196)."""
    model_type, model_args = args["type"], dict(args["model"])
    if model_type not in MODEL_TYPES:
        raise NotImplementedError(model_type)
    if init is None:
        init = not (args.get("paths", {}) or {}).get("ckpt")
    model_args.setdefault("init", init)
    if "init" in args["model"] and model_type != "CDLNetVideo":
        model_args["init"] = init
    return MODEL_TYPES[model_type](**model_args)


def load_ckpt(path, net, opt=None, sched=None):
    """train.py:232-247: tolerant of missing optimizer/scheduler state and of a missing `g`."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    net.load_state_dict(ckpt["net_state_dict"])
    epoch = ckpt.get("epoch", 0)
    if opt is not None and "opt_state_dict" in ckpt:
        opt.load_state_dict(ckpt["opt_state_dict"])
    if sched is not None and "sched_state_dict" in ckpt:
        sched.load_state_dict(ckpt["sched_state_dict"])
    return net, opt, sched, epoch


def save_ckpt(path, net, epoch=None, opt=None, sched=None):
    """train.py:221-230: same dictionary layout."""
    torch.save({"epoch": epoch, "net_state_dict": net.state_dict(),
                "opt_state_dict": None if opt is None else opt.state_dict(),
                "sched_state_dict": None if sched is None else sched.state_dict()}, path)


def init_model(args, device=torch.device("cpu")):
    """Returns (net, opt, sched, epoch0) like the reference's init_model."""
    net = build_model(args)
    net.to(device)
    train_args = args.get("train", {})
    opt = torch.optim.Adam(net.parameters(), **train_args.get("opt", {"lr": 1e-3}))
    sched = torch.optim.lr_scheduler.StepLR(opt, **train_args.get("sched", {"step_size": 50, "gamma": 0.95}))
    epoch0 = 0
    ckpt = (args.get("paths", {}) or {}).get("ckpt")
    if ckpt:
        net, opt, sched, epoch0 = load_ckpt(ckpt, net, opt, sched)
        net.to(device)
    return net, opt, sched, epoch0


# Noise levels with spatial extent.  The nets take sigma on the CODE grid, the divergence weight
# (level/255)^2 * b * xdot lives on the IMAGE grid: the SURE forms take the image-resolution level as `noise=` beside the
# net's `sigma`, and the steps derive the one from the other (utils.sigma_to_code_grid).
def _has_spatial_extent(level):
    return torch.is_tensor(level) and level.dim() > 2 and any(d > 1 for d in level.shape[2:])


def _divergence_weight(sigma, noise, image):
    """(level/255)^2 of the SURE divergence term, shaped against `image`: from `noise` (the noise standard deviation on the
    255 scale at image resolution) when given, else from the net's `sigma` -- today's expression."""
    if noise is not None:
        return (noise / 255.0) ** 2
    if _has_spatial_extent(sigma) and any(d not in (1, n) for d, n in zip(sigma.shape[2:], image.shape[2:])):
        raise ValueError(f"sigma of shape {tuple(sigma.shape)} is a noise-level map on the code grid of a stride > 1 net; the "
                         f"divergence term needs the level at the image resolution {tuple(image.shape[2:])}: pass it as noise=")
    return (sigma / 255.0) ** 2


def _net_sigma(net, level):
    """What the net takes as `sigma` for a level awgn drew: a level with spatial extent goes onto the net's code grid."""
    return sigma_to_code_grid(level, net.s) if _has_spatial_extent(level) else level


def mcsure_loss(net, obsrv, xhat, sigma, mask=1, h=1e-3, generator=None, b=None, *, noise=None):
    """Monte-Carlo SURE objective of train.py:87-93: data fidelity to the OBSERVATION plus a divergence
    estimate from one extra forward at obsrv + h*b, b ~ N(0, I):
        mean((obsrv - xhat)^2) + 2 * mean((sigma/255)^2 * b * (net(obsrv + h b) - xhat)) / h
    Gradients flow through both forward passes (both run in the HIP kernels).

    The divergence term divides the difference of two forward passes by h = 1e-3, which multiplies every arithmetic
    difference between them by 1e3.  On the matrix-core paths the operands are two-term bf16 splits (16-17 significant
    bits): per-step gradients agree with fp32 autograd to ~1e-4 (tests/test_gpu_nets.py), and over several Adam steps
    weights whose SURE gradient is below that noise drift apart.  `with loop.precision_scope(
    "split4")` adds the lo * lo products on the fused 2-D path; measured, it does not change that (the operand
    truncation, not the dropped product, is the floor), so it is not selected here.  `with loop.precision_scope("fp32")`
    around the training step runs both passes and their backward on the fp32 VALU kernels (6e-6 instead of 7e-5 per step,
    several times slower); the caller chooses.
    noise (keyword-only): the noise standard deviation on the 255 scale at image resolution, used for the divergence weight
    in place of sigma -- needed when sigma is a code-grid map of a stride > 1 net."""
    if b is None:
        dev = generator.device if generator is not None else obsrv.device
        b = torch.randn(obsrv.shape, device=dev, dtype=obsrv.dtype, generator=generator).to(obsrv.device)
    xhat_b, _ = net(obsrv.clone() + h * b, sigma, mask=mask)
    s2 = _divergence_weight(sigma, noise, obsrv)
    div = 2.0 * torch.mean(s2 * b * (xhat_b - xhat)) / h
    return torch.mean((obsrv - xhat) ** 2) + div


def sure_loss(net, obsrv, sigma, mask=1, generator=None, b=None, *, noise=None):
    """SURE objective with the divergence term from the exact directional derivative (net.jvp) instead of a finite
    difference: with (xhat, xdot) = net.jvp(obsrv, b, sigma, mask), b ~ N(0, I) drawn as mcsure_loss draws it,
        mean((obsrv - xhat)^2) + 2 * mean((sigma/255)^2 * b * xdot)
    xdot = J(obsrv) b at the supports of the primal codes: what h -> 0 of mcsure_loss converges to, with no step size,
    no 1/h in the gradient, and the same number of sweeps (two forward, two reverse).
    noise: as mcsure_loss's.  Returns (loss, xhat)."""
    if b is None:
        dev = generator.device if generator is not None else obsrv.device
        b = torch.randn(obsrv.shape, device=dev, dtype=obsrv.dtype, generator=generator).to(obsrv.device)
    xhat, xdot = net.jvp(obsrv, b, sigma, mask=mask)
    s2 = _divergence_weight(sigma, noise, obsrv)
    return torch.mean((obsrv - xhat) ** 2) + 2.0 * torch.mean(s2 * b * xdot), xhat


def train_step(net, opt, batch, noise_std, clip_grad=None, demosaic=False, project=True,
               grad_sync=None, generator=None, mcsure=False, loss_fn=None):
    """One optimiser step: awgn -> forward -> MSE (or MC-SURE) -> backward -> [all-reduce] -> clip -> Adam
    -> project (train.py:76-102).

    `grad_sync` is a callable run between backward and clipping (parallel.GradientBucket.sync).  `loss_fn(xhat, batch)`
    replaces the MSE (trainmri.py's `combmse`: a loss.CombinedLossWithSSIM); `mcsure` takes precedence over it.
    `mcsure`: False, True (the reference's finite-difference MC-SURE, mcsure_loss) or "exact" (sure_loss: the divergence
    from net.jvp).  A `noise_std` tensor with spatial extent (an image-resolution level map, which awgn takes) reaches the
    net on its code grid (utils.sigma_to_code_grid) and the SURE forms as `noise=`.
    Returns (loss tensor, sigma): sigma as awgn returned it.
    """
    if isinstance(mcsure, str) and mcsure != "exact":          # any other value keeps its truthiness
        raise ValueError(f"mcsure must be False, True or 'exact', got {mcsure!r}")
    mask = gen_bayer_mask(batch) if demosaic else 1
    noisy, level = awgn(batch, noise_std, generator)
    sigma = _net_sigma(net, level)
    noise = level if sigma is not level else None
    obsrv = mask * noisy
    opt.zero_grad(set_to_none=True)
    if isinstance(mcsure, str):
        loss, xhat = sure_loss(net, obsrv, sigma, mask=mask, generator=generator, noise=noise)
    else:
        xhat, _ = net(obsrv, sigma, mask=mask)
        if mcsure:
            loss = mcsure_loss(net, obsrv, xhat, sigma, mask=mask, generator=generator, noise=noise)
        elif loss_fn is not None:
            loss = loss_fn(xhat, batch)
        else:
            loss = torch.mean((batch - xhat) ** 2)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    if clip_grad is not None:
        nn.utils.clip_grad_norm_(net.parameters(), clip_grad)
    opt.step()
    if project and hasattr(net, "project"):
        net.project()
    return loss.detach(), level


# ------------------------------------------------------------------------------------------ CSR clip steps
# The frame-recurrent nets are trained on short clips, the code of one frame fed into the call for its neighbour
# (traincsr.py:192-217 for CDLNet_CSR on 2 frames, 247-273 for CDLNet_CSRf2 on 3).  _clip_chain is that call sequence, written
# once over an abstract `call(t, prev, after) -> (out, state)`: the supervised step passes codes as states, the exact SURE
# step (code, tangent) pairs, so both run the reference's calls in the reference's order.
def _clip_chain(call, D):
    """The reference's network calls on a clip of D frames; returns {frame index: out of the call that enters the loss}."""
    if D == 2:                                           # traincsr.py:201-204
        cur = None
        for _ in range(2):
            out0, prev = call(0, cur, None)
            out1, cur = call(1, prev, None)
        return {0: out0, 1: out1}
    if D == 3:                                           # traincsr.py:257-261
        out0, prev = call(0, None, None)
        out1, _ = call(1, prev, None)
        # line 259 reads `after_denoised` as the input of its own defining call (a NameError as written): the noisy
        # third frame is what the sequence evidently means; its z_prev stays as written
        out2, after = call(2, prev, None)
        out1, _ = call(1, prev, after)
        out0, prev = call(0, None, after)
        return {0: out0, 1: out1, 2: out2}
    raise ValueError(f"a CSR clip has 2 frames (CDLNet_CSR) or 3 (CDLNet_CSRf2), got {D}")


def _clip_depth(net, clip):
    if clip.dim() != 5:
        raise ValueError(f"clip: expected (B, C, D, H, W), got {tuple(clip.shape)}")
    D = clip.shape[2]
    want = 2 if isinstance(net, CDLNet_CSR) else 3 if isinstance(net, CDLNet_CSRf2) else D
    if D != want:
        raise ValueError(f"{type(net).__name__} trains on clips of {want} frames, got {D}")
    return D


def _net_call(net, D):
    """forward of a CSR net as `call(y, prev, after, sigma)`: CDLNet_CSR has no `z_after` argument.  A frame whose sigma is
    a noise-level map goes through temporal.csr_step."""
    def call(y, prev, after, sigma):
        codes = (prev,) if D == 2 else (prev, after)
        if temporal._is_sigma_map(sigma, y):
            return temporal.csr_step(net, y, *codes, sigma=sigma)
        return net(y, *codes, sigma)
    return call


def clip_forward(net, frames, sigmas):
    """The supervised chain on the noisy frames: [xhat_t] of the calls that enter the loss."""
    fwd = _net_call(net, len(frames))
    outs = _clip_chain(lambda t, prev, after: fwd(frames[t], prev, after, sigmas[t]), len(frames))
    return [outs[t] for t in range(len(frames))]


def _draw_b(frames, generator):
    dev = generator.device if generator is not None else frames[0].device
    return [torch.randn(y.shape, device=dev, dtype=y.dtype, generator=generator).to(y.device) for y in frames]


def sure_loss_clip(net, frames, sigmas, b=None, generator=None, *, noise=None):
    """Exact SURE objective of a clip step: the chain of clip_forward run with `jvp_recurrent`, one direction b_t ~ N(0, I)
    per distinct frame (drawn as sure_loss draws b, in frame order), the same b_t at every call on frame t, and the code
    tangent zdot carried from call to call next to the code:
        sum_t mean((y_t - xhat_t)^2) + 2 mean((sigma_t/255)^2 b_t xdot_t)
    over the calls that enter the supervised loss.  The chain maps ALL frames to all outputs jointly; sum_t b_t . xdot_t with
    xdot the derivative along (b_0, .., b_{D-1}) at once is the trace estimator of that joint map's Jacobian -- which needs
    the dependence of xhat_t on y_s (s != t) through the neighbour codes, hence zdot.
    A frame whose sigma is a noise-level map goes through temporal.csr_jvp_step (the rule of _net_call; section 38).
    noise: a list per frame of mcsure_loss's `noise`.  Returns (loss, [xhat_t])."""
    D = len(frames)
    if b is None:
        b = _draw_b(frames, generator)

    def jvp(t, prev, after):
        pairs = prev if D == 2 else prev + after
        if temporal._is_sigma_map(sigmas[t], frames[t]):
            return temporal.csr_jvp_step(net, frames[t], b[t], *pairs, sigma=sigmas[t])
        return net.jvp_recurrent(frames[t], b[t], *pairs, sigmas[t])
    none = (None, None)

    def call(t, prev, after):
        xhat, xdot, z, zdot = jvp(t, prev or none, after or none)
        return (xhat, xdot), (z, zdot)

    outs = _clip_chain(call, D)
    loss = 0.0
    for t in range(D):
        xhat, xdot = outs[t]
        s2 = _divergence_weight(sigmas[t], noise[t] if noise is not None else None, frames[t])
        loss = loss + torch.mean((frames[t] - xhat) ** 2) + 2.0 * torch.mean(s2 * b[t] * xdot)
    return loss, [outs[t][0] for t in range(D)]


def mcsure_loss_clip(net, frames, sigmas, xhats, h=1e-3, b=None, generator=None, *, noise=None):
    """The finite-difference form of sure_loss_clip (mcsure_loss over the chain): a second chain at y_t + h b_t.
    noise: as sure_loss_clip's."""
    if b is None:
        b = _draw_b(frames, generator)
    xb = clip_forward(net, [y.clone() + h * bt for y, bt in zip(frames, b)], sigmas)
    loss = 0.0
    for t, (y, s, bt, xhat, xhat_b) in enumerate(zip(frames, sigmas, b, xhats, xb)):
        s2 = _divergence_weight(s, noise[t] if noise is not None else None, y)
        loss = loss + torch.mean((y - xhat) ** 2) + 2.0 * torch.mean(s2 * bt * (xhat_b - xhat)) / h
    return loss


def _clip_noise(clip, noise_std, generator):
    """awgn per frame, in frame order (traincsr.py:196-197, 251-253): (clean, noisy, levels).  A `noise_std` tensor shaped
    like the clip (B,1,D,H,W) holds one level map per frame; any other applies to every frame as awgn takes it."""
    clean = [clip[:, :, d] for d in range(clip.shape[2])]
    per_frame = torch.is_tensor(noise_std) and noise_std.dim() == clip.dim()
    nstd = [noise_std[:, :, d] if per_frame else noise_std for d in range(len(clean))]
    noisy, sigmas = zip(*(awgn(x, n, generator) for x, n in zip(clean, nstd)))
    return clean, list(noisy), list(sigmas)


def _clip_sigmas(net, levels):
    """(sigmas the net takes, `noise=` of the SURE forms) for the levels awgn drew: levels with spatial extent go onto the
    code grid for the net and stay at image resolution for the divergence weight."""
    if not any(_has_spatial_extent(l) for l in levels):
        return levels, None
    return [_net_sigma(net, l) for l in levels], [l if _has_spatial_extent(l) else None for l in levels]


def _clip_mse(xhats, clean):
    per = [torch.mean((xh.detach() - x) ** 2) for xh, x in zip(xhats, clean)]
    return per, sum(per[1:], per[0]) / float(len(per))


def eval_step_clip(net, clip, noise_std, generator=None):
    """The val / test body of traincsr.py's train_model: (loss, sigmas, mse) of the supervised chain, no step."""
    D = _clip_depth(net, clip)
    clean, noisy, levels = _clip_noise(clip, noise_std, generator)
    per, mse = _clip_mse(clip_forward(net, noisy, _clip_sigmas(net, levels)[0]), clean)
    return sum(per[1:], per[0]), levels, mse


def train_step_clip(net, opt, clip, noise_std, clip_grad=None, project=True, grad_sync=None, generator=None, mcsure=False):
    """One optimiser step of a CSR net on a clip (B, C, D, H, W) (traincsr.py:192-217 / 247-273): awgn per frame -> the
    reference's chain of calls -> sum of the per-frame MSEs -> backward -> [all-reduce] -> clip -> Adam -> project.
    `mcsure`: False (supervised), True (finite differences over the chain, mcsure_loss_clip) or "exact" (sure_loss_clip).
    A `noise_std` tensor with spatial extent (image-resolution level maps: _clip_noise) reaches the net on its code grid and
    the SURE forms as `noise=`.
    Returns (loss, sigmas, mse): sigmas as awgn returned them, mse the mean of the per-frame MSEs against the clean frames
    (traincsr.py:217, 273)."""
    if isinstance(mcsure, str) and mcsure != "exact":
        raise ValueError(f"mcsure must be False, True or 'exact', got {mcsure!r}")
    _clip_depth(net, clip)
    clean, noisy, levels = _clip_noise(clip, noise_std, generator)
    sigmas, noise = _clip_sigmas(net, levels)
    opt.zero_grad(set_to_none=True)
    if isinstance(mcsure, str):
        loss, xhats = sure_loss_clip(net, noisy, sigmas, generator=generator, noise=noise)
    else:
        xhats = clip_forward(net, noisy, sigmas)
        if mcsure:
            loss = mcsure_loss_clip(net, noisy, sigmas, xhats, generator=generator, noise=noise)
        else:
            per = [torch.mean((xh - x) ** 2) for xh, x in zip(xhats, clean)]
            loss = sum(per[1:], per[0])
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    if clip_grad is not None:
        nn.utils.clip_grad_norm_(net.parameters(), clip_grad)
    opt.step()
    if project and hasattr(net, "project"):
        net.project()
    return loss.detach(), levels, _clip_mse(xhats, clean)[1]


# ------------------------------------------------------------------------------------------ fit loop
def grad_norm(params):
    """l2 norm of the mini-batch gradient (train.py:161-170)."""
    total = 0.0
    for p in params:
        if p.grad is not None:
            total += float(p.grad.detach().norm(2)) ** 2
    return total ** 0.5


def getlr(opt):
    return [pg["lr"] for pg in opt.param_groups]


def setlr(opt, lr):
    if not isinstance(lr, (list, tuple, np.ndarray)):
        lr = [lr for _ in opt.param_groups]
    for pg, v in zip(opt.param_groups, lr):
        pg["lr"] = float(v)


def save_args(args, ckpt=True):
    """train.py:249-258: args.json next to the checkpoints, pointing `paths.ckpt` at net.ckpt."""
    save_path = args["paths"]["save"]
    if ckpt:
        args["paths"]["ckpt"] = os.path.join(save_path, "net.ckpt")
    with open(os.path.join(save_path, "args.json"), "w") as f:
        f.write(json.dumps(args, indent=4, sort_keys=True))


def fit(net, opt, loaders, sched=None, epochs=1, device=torch.device("cpu"), save_dir=None, start_epoch=1,
        clip_grad=1, noise_std=25, demosaic=False, verbose=True, val_freq=1, save_freq=1, epoch_fun=None,
        mcsure=False, backtrack_thresh=1, grad_sync=None, log=print, group=None, generator=None, combmse=False,
        loss_fn=None):
    """The reference's training driver (train.py:35-158), same arguments and files:

    * phases train / val (every `val_freq` epochs) / test (only at `epoch == epochs`, as written there);
      val and test use the mid-range noise level;
    * per-epoch PSNR = mean over batches of -10 log10(loss), appended to `{phase}.txt`;
    * divergence backtracking: when a phase's PSNR falls `backtrack_thresh` dB below its best, or the loss
      is nan/inf, reload `net.ckpt` (`0.ckpt` while `epoch <= save_freq`), scale every learning rate by 0.8,
      rewind `epoch` to the checkpointed one and log it in `backtrack.txt`;
    * scheduler step per epoch; `net.ckpt` (+ `epoch_fun(epoch)`) every `save_freq` epochs; `0.ckpt` at start.
      Under data parallelism `epoch_fun` runs on RANK 0 ONLY, between the checkpoint write and the barrier: it is
      for rank-0 side effects (plots, copies of the checkpoint).  It must not change the net or the optimiser and
      must not issue a collective -- either would desynchronise or deadlock the replicas.
    * like the reference (train.py:113-142) the backtracking loop has NO bound: when the reloaded checkpoint
      itself cannot recover (e.g. a learning rate that diverges from `0.ckpt` at any scale the decay reaches
      within float range), `fit` repeats the epoch with lr x 0.8 indefinitely.

    `loaders` maps phase -> iterable of clean batches.  `generator` (new): the torch.Generator every noise draw uses;
    a CPU generator (torch.default_generator after torch.manual_seed) reproduces the random stream of the reference's
    CPU run on a GPU run (tests/test_gpu_trainer.py replays a reference-generated trajectory that way).  `grad_sync` (new) is run after backward for data
    parallel training (parallel.GradientBucket.sync).  Under data parallelism (an initialised process
    group; `group` selects it) every rank sees a different shard, so the decisions that change the
    training state are taken on REDUCED values: the phase PSNR is the mean over all ranks' batches and the
    nan / inf flag is the OR over ranks (parallel.phase_consensus) -- every rank backtracks, or none does.
    Rank 0 alone writes logs and checkpoints into `save_dir` (one node: the directory is shared); a
    barrier orders its writes before the other ranks' reads, and a backtrack reloads the SAME file on
    every rank, so replicas, optimiser states and learning rates stay identical.
    `noise_std`: a number, a `(lo, hi)` range, or a tensor -- an image-resolution level map that broadcasts against a batch
    ((B,1,H,W); for clips also (B,1,D,H,W), one map per frame), handed to awgn unwrapped in every phase (no level is drawn);
    the net then takes it on its code grid and the SURE forms as `noise=` (train_step / train_step_clip).
    `combmse` (trainmri.py / train3d.py): the train phase's loss is `loss_fn`, by default
    loss.CombinedLossWithSSIM(1.0, 0.01, 0.1) (VGG16 weights from the default local file); a `loss_fn` given without
    `combmse` is used the same way.  `mcsure` (True: finite differences; "exact": net.jvp, see train_step) takes
    precedence; val and test keep the MSE; the logged train PSNR is -10 log10 of that training loss, as in the reference.
    A CDLNet_CSR / CDLNet_CSRf2 net takes the clip steps instead (train_step_clip; eval_step_clip under no_grad in val / test):
    its batches are clips (B, C, D, H, W) and every phase logs 10 log10(1 / mse) of the frames' mean MSE (traincsr.py:124).
    Returns the history [(epoch, phase, psnr)].
    """
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank0 = (not ddp) or dist.get_rank(group) == 0
    sync_dev = next(net.parameters()).device

    def barrier():
        if ddp:
            dist.barrier(group=group)

    def append(name, text):
        if rank0:
            with open(os.path.join(save_dir, name), "a") as f:
                f.write(text)

    if save_dir is None:
        raise ValueError("fit needs save_dir (checkpoints drive the backtracking)")
    os.makedirs(save_dir, exist_ok=True)
    level_map = torch.is_tensor(noise_std)               # a level map (awgn's tensor form): every phase takes it as it is
    if not level_map and not isinstance(noise_std, (list, tuple)):
        noise_std = (noise_std, noise_std)
    if combmse and loss_fn is None and not isinstance(net, (CDLNet_CSR, CDLNet_CSRf2)):
        from .loss import CombinedLossWithSSIM
        loss_fn = CombinedLossWithSSIM(alpha=1.0, beta=0.01, gamma=0.1).to(device)
    log(f"fit: using device {device}")
    log("Saving initialization to 0.ckpt")
    if rank0:
        save_ckpt(os.path.join(save_dir, "0.ckpt"), net, 0, opt, sched)
    barrier()
    clips = isinstance(net, (CDLNet_CSR, CDLNet_CSRf2))      # traincsr.py: clip steps, PSNR from the frames' MSE
    if clips and (demosaic or combmse or loss_fn is not None):
        raise ValueError(f"fit: {type(net).__name__} trains on clips with the summed per-frame MSE (or SURE); `demosaic`, "
                         "`combmse` and `loss_fn` are not taken")
    top_psnr = {"train": 0, "val": 0, "test": 0}
    history = []
    epoch = start_epoch
    while epoch < start_epoch + epochs:
        diverged, loss = False, 0.0
        for phase in ("train", "val", "test"):
            net.train() if phase == "train" else net.eval()
            if epoch != epochs and phase == "test":
                continue
            if phase == "val" and epoch % val_freq != 0:
                continue
            if phase not in loaders or loaders[phase] is None:
                continue
            phase_nstd = noise_std if (phase == "train" or level_map) else (noise_std[0] + noise_std[1]) / 2.0
            psnr, nb, bad = 0.0, 0, False
            for batch in loaders[phase]:
                batch = batch.to(device)
                if level_map:
                    phase_nstd = phase_nstd.to(device)
                mse_t = None
                if clips and phase == "train":
                    loss_t, _, mse_t = train_step_clip(net, opt, batch, phase_nstd, clip_grad=clip_grad, grad_sync=grad_sync,
                                                       mcsure=mcsure, generator=generator)
                elif clips:
                    with torch.no_grad():
                        loss_t, _, mse_t = eval_step_clip(net, batch, phase_nstd, generator)
                elif phase == "train":
                    loss_t, _ = train_step(net, opt, batch, phase_nstd, clip_grad=clip_grad, demosaic=demosaic,
                                           grad_sync=grad_sync, mcsure=mcsure, generator=generator, loss_fn=loss_fn)
                else:
                    with torch.no_grad():
                        mask = gen_bayer_mask(batch) if demosaic else 1
                        noisy, sigma = awgn(batch, phase_nstd, generator)
                        xhat, _ = net(mask * noisy, _net_sigma(net, sigma), mask=mask)
                        loss_t = torch.mean((batch - xhat) ** 2)
                loss = float(loss_t)
                if verbose and phase == "train":
                    log(f"{phase.upper()}-E{epoch} loss={loss:.1e}|gnorm={grad_norm(net.parameters()):.1e}")
                level = loss if mse_t is None else float(mse_t)      # clips: 10 log10(1 / mse) (traincsr.py:124)
                psnr = psnr - 10 * np.log10(level) if level > 0 else float("nan")
                bad = bad or bool(np.isnan(loss) or np.isinf(loss))
                nb += 1
            # one reduction per phase: mean PSNR over every rank's batches, nan / inf on ANY rank
            psnr, bad = phase_consensus(psnr, nb, bad or bool(np.isnan(psnr)), sync_dev, group)
            if bad:
                psnr = float("nan")
            log(f"{phase.upper()} PSNR: {psnr:.3f} dB")
            history.append((epoch, phase, psnr))
            if psnr > top_psnr[phase]:
                top_psnr[phase] = psnr
            elif (psnr + backtrack_thresh < top_psnr[phase]) or bad:
                diverged = True
                break
            append(f"{phase}.txt", f"{psnr:.3f}, ")
        if diverged:
            ckpt_path = os.path.join(save_dir, "0.ckpt" if epoch <= save_freq else "net.ckpt")
            log(f"Loss has diverged. Backtracking to {ckpt_path} ...")
            append("backtrack.txt", f"{epoch}  ")
            epoch = epoch - save_freq if epoch % save_freq == 0 else epoch - epoch % save_freq
            old_lr = np.array(getlr(opt))
            load_ckpt(ckpt_path, net, opt, sched)
            net.to(device)
            setlr(opt, old_lr * 0.8)
            log(f"Updated Learning Rate(s): {getlr(opt)}")
            epoch = epoch + 1
            continue
        if sched is not None:
            sched.step()
        if epoch % save_freq == 0:
            if rank0:
                save_ckpt(os.path.join(save_dir, "net.ckpt"), net, epoch, opt, sched)
                if epoch_fun is not None:
                    epoch_fun(epoch)
            barrier()                            # the file is complete before any rank may reload it
        epoch = epoch + 1
    return history
