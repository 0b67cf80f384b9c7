#!/usr/bin/env python3
"""Bits of the fused 2-D tier with SEVERAL tiles per workgroup, recorded on the commit BEFORE the stage kernel's per-tile
phase changed (next tile's thin inputs loaded in front of the row loop, run-wise packed staging stores, 16-byte patch
write-out, no du_0 write in the sweep's last reverse stage):

    python tools/make_golden_stage_tile_phase_parent_bits.py tests/golden/t1_stage_tile_phase_parent_bits.npz   # on that commit, on the device

tests/test_gpu_stage_tile_phase.py calls `compute_case()` on the current commit and compares bit for bit.

Geometry: N = 2, C = 1, 40 x 150 -- 3 tile rows (the last 8 rows tall) x 3 tile columns (the last 22 wide), 18 tiles.
With CDL_FUSED_GRID=4 the workgroups walk 5, 5, 4 and 4 tiles: the prefetch crosses into the next image and runs past
the last tile; with the default grid every workgroup has one tile.  Cases `train/M<M>P<P>/K<K>/<layout>/<grid>[/da0]`:
a training step through the net's public call (y and a per-sample sigma require grad, the loss on xhat and z_K);
`step/M<M>P<P>/<layout>`: cdl_fused2d_iter_fwd and cdl_fused2d_stage_bwd (with and without the dA_k ride) at the capped
grid.  Image- and code-sized tensors are recorded as two 64-bit folds of their int32 bit patterns, sum and xor.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, C, SP = 2, 1, (40, 150)
MP = [(64, 7), (32, 5)]
CAPPED = "4"          # CDL_FUSED_GRID of the "g4" cases

TRAIN_CASES = [f"train/M{M}P{P}/K{K}/{lay}/{grid}" for (M, P) in MP for K in (2, 3) for lay in ("blocked", "nchw")
               for grid in ("g4", "gdef")] + ["train/M64P7/K2/blocked/g4/da0"]
STEP_CASES = [f"step/M{M}P{P}/{lay}" for (M, P) in MP for lay in ("blocked", "nchw")]
CASES = TRAIN_CASES + STEP_CASES


def _fold(t):
    """(sum, xor) of the int32 bit patterns of a float32 or int32 tensor, as int64."""
    import numpy as np
    bits = t.detach().contiguous().cpu().numpy().view(np.int32).astype(np.int64).ravel()
    return np.array([bits.sum(), np.bitwise_xor.reduce(bits)], dtype=np.int64)


def _train(cva, M, P, K, out, case):
    import torch
    net = cva.CDLNet(K=K, M=M, P=P, s=1, C=C, t0=0.0, adaptive=True, init=False)
    gen = torch.Generator().manual_seed(11 + M + K)
    with torch.no_grad():
        for m in list(net.A) + list(net.B):
            m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=gen))
        net.t.copy_(0.3 * torch.rand(net.t.shape, generator=gen))
    net = net.cuda()
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    y = rnd(N, C, *SP).requires_grad_()
    sg = (15.0 + 20.0 * torch.rand(N, generator=gen)).cuda().requires_grad_()
    wx, wz = rnd(N, C, *SP), rnd(N, M, *SP)
    xhat, z = net(y, sg)
    ((xhat * wx).sum() + (z * wz).sum()).backward()
    torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"], out[case + "/dy"] = _fold(xhat), _fold(z), _fold(y.grad)
    out[case + "/dsigma"] = sg.grad.cpu().numpy()
    out[case + "/dt"] = net.t.grad.detach().cpu().numpy()
    out[case + "/dA"] = torch.stack([m.weight.grad for m in net.A]).cpu().numpy()
    out[case + "/dB"] = torch.stack([m.weight.grad for m in net.B]).cpu().numpy()


def _steps(cva, M, P, lay, out, case):
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
    zo = o.fused_iter(g, r, o.fused_from_nchw(g, zin, lay), tau, frags, -1.0, patches, out=None, map_out=bits,
                      lay_in=lay, lay_out=lay)
    torch.cuda.synchronize()
    out[case + "/iter/z"], out[case + "/iter/patches"] = _fold(o.fused_to_nchw(g, zo, lay)), _fold(patches)
    out[case + "/iter/map"] = _fold(bits)
    base = o.fused_from_nchw(g, rnd(*g.code_shape()), lay)
    for name, rider in (("bwd", {}), ("bwd_da", dict(r2=r2, alpha=-1.0, workspace=o.fused_wgrad_workspace(g, "cuda")))):
        dtp = torch.empty((o.fused_tiles(g), M), device="cuda")
        res = o.fused_stage_bwd(g, r, base, bits, frags, patches, dtp, True, lay_in=lay, lay_out=lay, **rider)
        torch.cuda.synchronize()
        du = res[0] if rider else res
        out[f"{case}/{name}/du"], out[f"{case}/{name}/patches"] = _fold(o.fused_to_nchw(g, du, lay)), _fold(patches)
        out[f"{case}/{name}/dtau_partial"] = dtp.cpu().numpy()
        if rider:
            out[f"{case}/{name}/dA"] = res[1].cpu().numpy()


def compute_case(case, setenv):
    """{name: numpy array} of one case.  `setenv(name, value)` sets a CDL_* switch and reloads the library's options
    (the hip_env fixture of tests/conftest.py; `_setenv` below)."""
    import cdlnet_video_amd as cva
    loop = cva.loop
    assert loop.BACKEND == "auto" and loop.PRECISION == "split3" and loop.CODE_LAYOUT == "blocked"
    parts = case.split("/")
    M, P = (int(v) for v in parts[1][1:].split("P"))
    out = {}
    if parts[0] == "step":
        setenv("CDL_FUSED_GRID", CAPPED)
        _steps(cva, M, P, parts[2], out, case)
        return out
    K, lay, grid = int(parts[2][1:]), parts[3], parts[4]
    if grid == "g4":
        setenv("CDL_FUSED_GRID", CAPPED)
    if parts[-1] == "da0":
        setenv("CDL_FUSED_DA", "0")
    loop.set_code_layout(lay)
    try:
        _train(cva, M, P, K, out, case)
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
        for name_ in ("CDL_FUSED_GRID", "CDL_FUSED_DA"):
            os.environ.pop(name_, None)
        cva._lib.reload_options()
        rec.update(compute_case(case_, _setenv))
    np.savez_compressed(sys.argv[1], **rec)
    print("wrote", sys.argv[1], len(rec), "arrays")
