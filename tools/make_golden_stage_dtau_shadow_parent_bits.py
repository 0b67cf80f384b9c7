#!/usr/bin/env python3
"""Bits of the fused 2-D reverse stage, recorded on the commit BEFORE its threshold-gradient partials moved under the
synthesis MFMAs and their per-tile exchange left LDS:

    python tools/make_golden_stage_dtau_shadow_parent_bits.py tests/golden/t2_stage_dtau_shadow_parent_bits.npz   # on that commit, on the device

tests/test_gpu_stage_dtau_shadow.py calls `compute_case()` on the current commit and compares bit for bit.

Geometries (N = 2, C = 1): 20 x 70 with P = 5 and 33 x 65 with P = 7, each with M = 32 and 64 -- a partial tile on both axes
of the 64 x 16 tile (and of the 64 x 32 one).  Cases:

  step/M<M>P<P>/<layout>/<precision>   cdl_fused2d_stage_bwd with and without the dA_k ride, with and without the synthesis half,
                                       once per support/sign map of PATTERNS (the maps are written here, bit by bit, so that a
                                       wrong exchange between lanes c and c ^ 1, 2, 4, 8, 16 shows)
  stepmap/M<M>P<P>/<layout>            the same stage under a noise-level map (weighted partials and dL/dcmap), two patterns
  train/M<M>P<P>/<layout>/<precision>/<grid>   a K = 3 training step through net(y, sigma): both tile directions (every other
                                       launch of a sweep walks the tiles from the last to the first), with CDL_FUSED_GRID=3
                                       several tiles per workgroup; "blocked_bf16" is the 64 x 32 tile
  trainmap/M64P7/blocked               the same with a noise-level map on the fused tier

Code- and patch-sized tensors, the step-wise dA and dcmap and the training steps' dB are recorded as two 64-bit folds of their
int32 bit patterns, sum and xor; the threshold partials, dt, the training steps' dA and dL/dcmap value by value.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, C = 2, 1
GEOMS = [(32, 5, (20, 70)), (64, 5, (20, 70)), (32, 7, (33, 65)), (64, 7, (33, 65))]
SHAPE = {(M, P): sp for (M, P, sp) in GEOMS}
PATTERNS = ("empty", "full", "allneg", "onechannel", "onecolumn", "lanes")
CAPPED = "3"          # CDL_FUSED_GRID of the "g3" cases

STEP_CASES = [f"step/M{M}P{P}/{lay}/{prec}" for (M, P, _) in GEOMS for lay in ("blocked", "nchw") for prec in ("split3", "bf16")]
STEPMAP_CASES = [f"stepmap/M{M}P{P}/{lay}" for (M, P) in ((64, 7), (32, 5)) for lay in ("blocked", "nchw")]
TRAIN_CASES = [f"train/M{M}P{P}/{lay}/{prec}/{grid}" for (M, P, lay, prec, grid) in (
    (64, 7, "blocked", "split3", "g3"), (64, 7, "blocked", "split3", "gdef"), (64, 7, "nchw", "split3", "g3"),
    (64, 7, "blocked", "bf16", "g3"), (64, 7, "blocked_bf16", "split3", "g3"), (32, 5, "blocked", "split3", "g3"),
    (32, 5, "nchw", "bf16", "gdef"), (32, 5, "blocked_bf16", "bf16", "g3"), (64, 5, "blocked", "split3", "g3"),
    (32, 7, "nchw", "split3", "g3"))]
TRAINMAP_CASES = ["trainmap/M64P7/blocked"]
CASES = STEP_CASES + STEPMAP_CASES + TRAIN_CASES + TRAINMAP_CASES


def _fold(t):
    """(sum, xor) of the int32 bit patterns of a float32 or int32 tensor, as int64."""
    import numpy as np
    bits = t.detach().contiguous().cpu().numpy().view(np.int32).astype(np.int64).ravel()
    return np.array([bits.sum(), np.bitwise_xor.reduce(bits)], dtype=np.int64)


def gate_maps(pattern, M, sp, gen):
    """The (N, 4, H, W) int32 words of one support/sign pattern.  Plane 2h holds the support bits and plane 2h + 1 the sign
    bits of lane half h; bit 16R + v of a word is channel 32R + 8(v>>2) + 4h + (v&3) of its pixel."""
    import torch
    H, W = sp
    nb = M // 2                                              # bits per word: 16 per 32 channels
    full = (1 << nb) - 1
    rnd = lambda: torch.randint(0, 1 << 16, (N, 2, H, W), generator=gen) | (torch.randint(0, 1 << 16, (N, 2, H, W), generator=gen) << 16)
    sup, sgn = rnd() & full, rnd() & full
    x = torch.arange(W).reshape(1, 1, 1, W).expand(N, 2, H, W)
    if pattern == "empty":
        sup = torch.zeros_like(sup)
    elif pattern == "full":
        sup = torch.full_like(sup, full)
    elif pattern == "allneg":
        sgn = torch.full_like(sgn, full)
    elif pattern == "onechannel":                            # channel 13: R = 0, h = 1, v = 5
        sup = torch.zeros_like(sup)
        sup[:, 1] = 1 << 5
    elif pattern == "onecolumn":
        sup = torch.where(x == 37, sup, torch.zeros_like(sup))
    elif pattern == "lanes":                                 # bit b follows bit (b mod 5) of the pixel column: lanes c and
        sup, sgn = torch.zeros_like(sup), torch.zeros_like(sgn)   # c ^ (1 << (b mod 5)) differ in it
        for b in range(nb):
            sup |= ((x >> (b % 5)) & 1) << b
            sgn |= ((x >> ((b + 2) % 5)) & 1) << b
    else:
        raise ValueError(pattern)
    words = torch.stack([sup[:, 0], sgn[:, 0], sup[:, 1], sgn[:, 1]], 1)
    words = torch.where(words >= (1 << 31), words - (1 << 32), words)
    return words.to(torch.int32).contiguous()


def _steps(cva, M, P, lay, prec, out, case, with_map):
    import torch
    o = cva.ops
    sp = SHAPE[(M, P)]
    g = o.Geometry.make(N, C, M, sp, (P, P), (P // 2, P // 2), 1)
    assert o.fused_supported(g)
    gen = torch.Generator().manual_seed(7 + M + P)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    wA, wB = 0.1 * rnd(M, C, P, P), 0.1 * rnd(M, C, P, P)
    r, r2 = rnd(*g.image_shape()), rnd(*g.image_shape())
    frags = o.fused_prep(wA, wB)
    base = o.fused_from_nchw(g, rnd(*g.code_shape()), lay)
    tiles = o.fused_tiles(g)
    mapkw = {}
    if with_map:
        cmap = (10.0 + 20.0 * torch.rand(g.image_shape(), generator=gen)).cuda()
        mapkw = dict(cmap=cmap, tslope=(0.02 * torch.rand(M, generator=gen)).cuda())
    for pat in (("full", "lanes") if with_map else PATTERNS):
        bits = gate_maps(pat, M, sp, gen).cuda()
        for name, rider, synth in (("bwd", {}, True), ("bwd_nosynth", {}, False),
                                   ("bwd_da", dict(r2=r2, alpha=-1.0, workspace=o.fused_wgrad_workspace(g, "cuda")), True)):
            if with_map and not synth:
                continue
            patches = o.fused_patches(g, "cuda").zero_()     # sized for the larger tile shape: the tail is never written
            dtp = torch.zeros(((2 if with_map else 1) * tiles, M), device="cuda")
            if with_map:
                mapkw["dcmap"] = rnd(*g.image_shape())
                mapkw["dcmap_add"] = bool(rider)             # written without the ride, added with it
            res = o.fused_stage_bwd(g, r, base, bits, frags, patches, dtp, synth, precision=prec, lay_in=lay, lay_out=lay,
                                    **rider, **mapkw)
            torch.cuda.synchronize()
            du = res[0] if rider else res
            key = f"{case}/{pat}/{name}"
            out[key + "/du"], out[key + "/patches"] = _fold(o.fused_to_nchw(g, du, lay)), _fold(patches)
            out[key + "/dtau_partial"] = dtp.cpu().numpy()
            if rider:
                out[key + "/dA"] = _fold(res[1])
            if with_map:
                out[key + "/dcmap"] = _fold(mapkw["dcmap"])


def _train(cva, M, P, out, case, with_map):
    import torch
    sp = SHAPE[(M, P)]
    net = cva.CDLNet(K=3, M=M, P=P, s=1, C=C, t0=0.0, adaptive=True, init=False)
    gen = torch.Generator().manual_seed(13 + M + P)
    with torch.no_grad():
        for m in list(net.A) + list(net.B):
            m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=gen))
        net.t.copy_(0.3 * torch.rand(net.t.shape, generator=gen) * (0.05 if with_map else 1.0))
    net = net.cuda()
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    y = rnd(N, C, *sp).requires_grad_()
    if with_map:
        sg = (15.0 + 20.0 * torch.rand((N, 1) + sp, generator=gen)).cuda().requires_grad_()
    else:
        sg = (15.0 + 20.0 * torch.rand(N, generator=gen)).cuda().requires_grad_()
    wx, wz = rnd(N, C, *sp), rnd(N, M, *sp)
    xhat, z = net(y, sg)
    ((xhat * wx).sum() + (z * wz).sum()).backward()
    torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"], out[case + "/dy"] = _fold(xhat), _fold(z), _fold(y.grad)
    out[case + "/dcmap" if with_map else case + "/dsigma"] = sg.grad.cpu().numpy()
    out[case + "/dt"] = net.t.grad.detach().cpu().numpy()
    out[case + "/dA"] = torch.stack([m.weight.grad for m in net.A]).cpu().numpy()
    out[case + "/dB"] = _fold(torch.stack([m.weight.grad for m in net.B]))


def compute_case(case, setenv):
    """{name: numpy array} of one case.  `setenv(name, value)` sets a CDL_* switch and reloads the library's options
    (the hip_env fixture of tests/conftest.py; `_setenv` below)."""
    import cdlnet_video_amd as cva
    loop = cva.loop
    assert loop.BACKEND == "auto" and loop.PRECISION == "split3" and loop.CODE_LAYOUT == "blocked" and loop.MAP_TIER == "generic"
    parts = case.split("/")
    M, P = (int(v) for v in parts[1][1:].split("P"))
    out = {}
    if parts[0] == "step":
        _steps(cva, M, P, parts[2], parts[3], out, case, False)
        return out
    if parts[0] == "stepmap":
        _steps(cva, M, P, parts[2], "split3", out, case, True)
        return out
    with_map = parts[0] == "trainmap"
    lay = parts[2]
    prec, grid = (parts[3], parts[4]) if not with_map else ("split3", "g3")
    if grid == "g3":
        setenv("CDL_FUSED_GRID", CAPPED)
    loop.set_code_layout(lay)
    try:
        with loop.precision_scope(prec), loop.map_tier_scope("fused" if with_map else "generic"):
            _train(cva, M, P, out, case, with_map)
    finally:
        loop.set_code_layout("blocked")
    return out


def _setenv(name, value):
    import cdlnet_video_amd as cva
    os.environ[name] = value
    cva._lib.reload_options()


if __name__ == "__main__":
    import numpy as np
    import cdlnet_video_amd as cva
    rec = {}
    for case_ in CASES:
        os.environ.pop("CDL_FUSED_GRID", None)
        cva._lib.reload_options()
        rec.update(compute_case(case_, _setenv))
    np.savez_compressed(sys.argv[1], **rec)
    print("wrote", sys.argv[1], len(rec), "arrays")
