#!/usr/bin/env python3
"""Bits of the fused 2-D tier (cdl_fused2d.hip: k_stage, k_wgrad2d) in every arithmetic mode, code layout and map form
whose kernels share device phases, recorded on the commit BEFORE those phases were folded into one function each (the
transposition product of the filter gradient, the cross-wave sum, the tile decode, the hi/lo split; DESIGN.md
section 34):

    python tools/make_golden_fused2d_shared_phases_parent_bits.py tests/golden/f2d_shared_phases_parent_bits.npz   # on that commit, on the device

tests/test_gpu_fused2d_shared_phases.py calls `compute_case()` on the current commit and compares bit for bit.

Geometry: N = 2, C = 1, 40 x 150 -- 3 x 3 tiles of 64 x 16 per image (the last row 8 tall, the last column 22 wide), or
2 x 3 tiles of 64 x 32 (the bf16 storage layout's stage).  With CDL_FUSED_GRID=4 ("g4") a workgroup walks several tiles,
runs into the next image and past the last tile; with the default grid ("gdef") every workgroup has one tile.  Cases:
  train/M<M>P<P>/<precision>/<layout>/<grid>[/da0]   a K = 3 training step through the net's public call (y and a per-sample
                                                     sigma require grad, the loss on xhat and z_K); da0: CDL_FUSED_DA=0,
                                                     the two-operator form of k_wgrad2d
  map/M<M>P<P>/<layout>/<grid>                       the same step with a noise-level map under map_tier_scope("fused"),
                                                     dL/dcmap recorded as the map's gradient
  step/M<M>P<P>/<precision>/<layout>                 fused_iter, fused_stage_bwd with and without the dA_k ride, fused_wgrad
                                                     with one operator and with two, at the capped grid
  jvp/M<M>P<P>                                       net.jvp at K = 2 (split3, blocked, capped grid) and the parameter
                                                     gradients of a loss on (xhat, xdot)
Image- and code-sized tensors are recorded as two 64-bit folds of their int32 bit patterns, sum and xor; gradients in full.
The record is written as the named file and <stem>.1.npz, <stem>.2.npz, ... (save_parts: whole cases, each file below 1 MiB).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, C, SP = 2, 1, (40, 150)
MP = [(64, 7), (32, 5)]
CAPPED = "4"          # CDL_FUSED_GRID of the "g4" cases
K_TRAIN, K_JVP = 3, 2
CELLS = [("split3", "blocked"), ("split4", "blocked"), ("bf16", "blocked"), ("split3", "nchw"), ("split3", "blocked_bf16")]
GRIDS = ("g4", "gdef")

TRAIN_CASES = [f"train/M{M}P{P}/{prec}/{lay}/{grid}" for (M, P) in MP for (prec, lay) in CELLS for grid in GRIDS] + \
              [f"train/M{M}P{P}/split3/blocked/g4/da0" for (M, P) in MP]
MAP_CASES = [f"map/M{M}P{P}/{lay}/{grid}" for (M, P) in MP for lay in ("blocked", "nchw") for grid in GRIDS]
STEP_CASES = [f"step/M{M}P{P}/{prec}/{lay}" for (M, P) in MP for prec in ("split3", "split4") for lay in ("nchw", "blocked")]
JVP_CASES = [f"jvp/M{M}P{P}" for (M, P) in MP]
CASES = TRAIN_CASES + MAP_CASES + STEP_CASES + JVP_CASES


def _fold(t):
    """(sum, xor) of the int32 bit patterns of a float32 or int32 tensor, as int64."""
    import numpy as np
    bits = t.detach().contiguous().cpu().numpy().view(np.int32).astype(np.int64).ravel()
    return np.array([bits.sum(), np.bitwise_xor.reduce(bits)], dtype=np.int64)


def _net(cva, M, P, K, gen):
    import torch
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=C, t0=0.0, adaptive=True, init=False)
    with torch.no_grad():
        for m in list(net.A) + list(net.B):
            m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=gen))
        net.t.copy_(0.3 * torch.rand(net.t.shape, generator=gen))
    return net.cuda()


def _grads(net, out, case):
    import torch
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    out[case + "/dt"] = zero(net.t).detach().cpu().numpy()
    out[case + "/dA"] = torch.stack([zero(m.weight) for m in net.A]).cpu().numpy()
    out[case + "/dB"] = torch.stack([zero(m.weight) for m in net.B]).cpu().numpy()


def _train(cva, M, P, out, case, with_map):
    import torch
    gen = torch.Generator().manual_seed(11 + M + K_TRAIN)
    net = _net(cva, M, P, K_TRAIN, gen)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    y = rnd(N, C, *SP).requires_grad_()
    if with_map:         # varies inside every tile and differs per sample
        sg = (15.0 + 20.0 * torch.rand((N, 1) + SP, generator=gen)).cuda().requires_grad_()
    else:
        sg = (15.0 + 20.0 * torch.rand(N, generator=gen)).cuda().requires_grad_()
    wx, wz = rnd(N, C, *SP), rnd(N, M, *SP)
    xhat, z = net(y, sg)
    ((xhat * wx).sum() + (z * wz).sum()).backward()
    torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"], out[case + "/dy"] = _fold(xhat), _fold(z), _fold(y.grad)
    out[case + "/dsigma"] = sg.grad.cpu().numpy()
    _grads(net, out, case)


def _jvp(cva, M, P, out, case):
    import torch
    gen = torch.Generator().manual_seed(23 + M)
    net = _net(cva, M, P, K_JVP, gen)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    y, v = rnd(N, C, *SP), rnd(N, C, *SP)
    sg = (15.0 + 20.0 * torch.rand(N, generator=gen)).cuda()
    wx, wd = rnd(N, C, *SP), rnd(N, C, *SP)
    xhat, xdot = net.jvp(y, v, sg)
    ((xhat * wx).sum() + (xdot * wd).sum()).backward()
    torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/xdot"] = _fold(xhat), _fold(xdot)
    _grads(net, out, case)


def _steps(cva, M, P, prec, lay, out, case):
    import torch
    o = cva.ops
    g = o.Geometry.make(N, C, M, SP, (P, P), (P // 2, P // 2), 1)
    assert o.fused_supported(g) and o.fused_tiles(g) == 18
    gen = torch.Generator().manual_seed(5 + M)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    wA, wB = 0.1 * rnd(M, C, P, P), 0.1 * rnd(M, C, P, P)
    r, r2 = rnd(*g.image_shape()), rnd(*g.image_shape())
    zin = rnd(*g.code_shape()) * (torch.rand(g.code_shape(), generator=gen) < 0.4).cuda()
    tau = (0.3 * torch.rand((N, M), generator=gen)).cuda()
    frags = o.fused_prep(wA, wB)
    patches = o.fused_patches(g, "cuda").zero_()             # sized for the larger tile shape: the tail is never written
    bits = o.fused_map(g, "cuda")
    zo = o.fused_iter(g, r, o.fused_from_nchw(g, zin, lay), tau, frags, -1.0, patches, prec, out=None, map_out=bits,
                      lay_in=lay, lay_out=lay)
    torch.cuda.synchronize()
    out[case + "/iter/z"], out[case + "/iter/patches"] = _fold(o.fused_to_nchw(g, zo, lay)), _fold(patches)
    out[case + "/iter/map"] = _fold(bits)
    base = o.fused_from_nchw(g, rnd(*g.code_shape()), lay)
    ws = o.fused_wgrad_workspace(g, "cuda")
    for name, rider in (("bwd", {}), ("bwd_da", dict(r2=r2, alpha=-1.0, workspace=ws))):
        dtp = torch.empty((o.fused_tiles(g), M), device="cuda")
        res = o.fused_stage_bwd(g, r, base, bits, frags, patches, dtp, True, prec, lay_in=lay, lay_out=lay, **rider)
        torch.cuda.synchronize()
        du = res[0] if rider else res
        out[f"{case}/{name}/du"], out[f"{case}/{name}/patches"] = _fold(o.fused_to_nchw(g, du, lay)), _fold(patches)
        out[f"{case}/{name}/dtau_partial"] = dtp.cpu().numpy()
        if rider:
            out[f"{case}/{name}/dA"] = res[1].cpu().numpy()
    X1 = o.fused_from_nchw(g, zin, lay)
    (d0, none) = o.fused_wgrad(g, ws, du, r2, -1.0, precision=prec, layout=lay, tiles_reversed=True)
    assert none is None
    out[case + "/wgrad1/d0"] = d0.cpu().numpy()
    d0, d1 = o.fused_wgrad(g, ws, du, r2, -1.0, X1, r, 1.0, prec, layout=lay)
    out[case + "/wgrad2/d0"], out[case + "/wgrad2/d1"] = d0.cpu().numpy(), d1.cpu().numpy()


def compute_case(case, setenv):
    """{name: numpy array} of one case.  `setenv(name, value)` sets a CDL_* switch and reloads the library's options
    (the hip_env fixture of tests/conftest.py; `_setenv` below)."""
    import cdlnet_video_amd as cva
    loop = cva.loop
    assert loop.BACKEND == "auto" and loop.PRECISION == "split3" and loop.CODE_LAYOUT == "blocked"
    assert loop.MAP_TIER == "generic"
    parts = case.split("/")
    kind = parts[0]
    M, P = (int(v) for v in parts[1][1:].split("P"))
    out = {}
    if kind == "step":
        setenv("CDL_FUSED_GRID", CAPPED)
        _steps(cva, M, P, parts[2], parts[3], out, case)
        return out
    if kind == "jvp":
        setenv("CDL_FUSED_GRID", CAPPED)
        _jvp(cva, M, P, out, case)
        return out
    prec, lay, grid = ("split3", parts[2], parts[3]) if kind == "map" else (parts[2], parts[3], parts[4])
    if grid == "g4":
        setenv("CDL_FUSED_GRID", CAPPED)
    if parts[-1] == "da0":
        setenv("CDL_FUSED_DA", "0")
    loop.set_code_layout(lay)
    try:
        with loop.precision_scope(prec), loop.map_tier_scope("fused" if kind == "map" else "generic"):
            _train(cva, M, P, out, case, kind == "map")
    finally:
        loop.set_code_layout("blocked")
    return out


PART_BYTES = 900 << 10     # of array data per file: the filter gradients are kept in full, and a committed file stays below 1 MiB


def part_paths(path):
    """The files of the record written as `path`: path itself, then <stem>.1.npz, <stem>.2.npz, ... while they exist."""
    stem = path[:-len(".npz")]
    paths, i = [path], 1
    while os.path.exists(f"{stem}.{i}.npz"):
        paths.append(f"{stem}.{i}.npz")
        i += 1
    return paths


def save_parts(path, rec):
    """Write {name: array} as path, <stem>.1.npz, ...: whole cases in the order of CASES, a new file whenever the next
    case would take the current one past PART_BYTES.  Returns {file: names}."""
    import numpy as np
    assert path.endswith(".npz")
    parts, size = [[]], 0
    for case in CASES:
        names = [k for k in rec if k.startswith(case + "/") and (case + "/da0/") not in k]
        nbytes = sum(rec[k].nbytes for k in names)
        if parts[-1] and size + nbytes > PART_BYTES:
            parts.append([])
            size = 0
        parts[-1] += names
        size += nbytes
    assert sorted(k for part in parts for k in part) == sorted(rec)
    stem, out = path[:-len(".npz")], {}
    for i, names in enumerate(parts):
        out[path if i == 0 else f"{stem}.{i}.npz"] = names
        np.savez_compressed(path if i == 0 else f"{stem}.{i}.npz", **{k: rec[k] for k in names})
    return out


def load_parts(path):
    """{name: array} of the record written by save_parts."""
    import numpy as np
    rec = {}
    for part in part_paths(path):
        with np.load(part) as data:
            assert not set(data.files) & set(rec), part
            rec.update({k: data[k] for k in data.files})
    return rec


def _setenv(name, value):
    import cdlnet_video_amd as cva
    os.environ[name] = value
    cva._lib.reload_options()


if __name__ == "__main__":
    import numpy as np
    import cdlnet_video_amd as cva
    rec = {}
    for case_ in CASES:
        for name_ in ("CDL_FUSED_GRID", "CDL_FUSED_DA"):
            os.environ.pop(name_, None)
        cva._lib.reload_options()
        rec.update(compute_case(case_, _setenv))
        print("recorded", case_, flush=True)
    for path_, part_ in save_parts(sys.argv[1], rec).items():
        print("wrote", path_, len(part_), "arrays")
