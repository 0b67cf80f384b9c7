#!/usr/bin/env python3
"""Bits and launch order of what tools/make_golden_sweep_tiers_parent_bits.py does not reach -- the CSR sweeps, the
matrix-core rungs of the generic tier, the residual block, the VGG backward and the single-bank filter calls -- recorded on
the commit BEFORE the `_ws` pairs and the single-bank forms were folded into one entry point per operator (DESIGN.md
section 32):

    python tools/make_golden_entry_points_parent_bits.py tests/golden/t1_entry_points_parent_bits.npz   # on that commit, on the device

tests/test_gpu_entry_points.py calls `compute()` on the current commit and compares bit for bit, and the launch lists
(`<case>/launches`) as lists.  Public Python calls only, so the same tool runs on both commits.  Fat tensors are recorded
as folds (`_fold` of the sweep-tiers tool).  Of the `mfma/*` cases `<case>/ana` also holds the (PROX, REV) pairs the
matrix-core analysis ran with, one row per launch.
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_golden_sweep_tiers_parent_bits",
                                               os.path.join(ROOT, "tools", "make_golden_sweep_tiers_parent_bits.py"))
_t0 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_t0)
_fold, _site_ids, _param_grads = _t0._fold, _t0._site_ids, _t0._param_grads

N, K = 2, 3
CSR_GEOM = (2, 5, (13, 11), 3)                       # C, M, spatial, P: the `generic` geometry of the sweep-tiers record
# the smallest shapes of tests/test_gpu_dispatch.py on the matrix cores (at 256 compute units): 2-D, 64 filter-gradient
# tiles and 128 analysis workgroups -- k_ana_m, k_synth_m and k_wgm; 3-D, the 96-workgroup minimum of k_ana_m
MFMA_2D = (16, 1, 8, (60, 121), 5)                   # N, C, M, spatial, P
MFMA_3D = (4, 1, 16, (6, 30, 61), (3, 5, 5))
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
GABOR = [(1, 6, 1, 5, False), (2, 4, 1, 7, True), (3, 5, 3, 9, False)]     # tests/test_gpu_ops.py::test_gabor_bank_and_adjoint


def _detie(net, seed):
    """Distinct filters per iteration, thresholds that zero about half of every code; same bits on every call."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(net.named_parameters()):
            if name.split(".")[0] in ("t", "t2"):
                p.copy_(0.3 * torch.rand(p.shape, generator=gen))
            elif name.split(".")[0] in ("g", "g1", "g2"):
                p.copy_(0.2 + 1.2 * torch.rand(p.shape, generator=gen))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    return net.cuda()


def _grads(net, out, case):
    """Every parameter's gradient under its own name (a parameter the case does not use: zeros)."""
    import torch
    for name, p in sorted(net.named_parameters()):
        out[f"{case}/d.{name}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy()
    net.zero_grad(set_to_none=True)


def _finish(tr, out, case, ana=False):
    import numpy as np
    out[case + "/launches"] = np.array(_site_ids(tr))
    if ana:
        rows = [[int(r.template()["PROX"]), int(r.template()["REV"])] for r, s in zip(tr, _site_ids(tr)) if s == K_ANA]
        out[case + "/ana"] = np.array(rows, dtype=np.int64).reshape(-1, 2)


def _csr_data(n, C, M, sp, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    sparse = lambda: (0.3 * torch.randn((n, M) + sp, generator=gen) * (torch.rand((n, M) + sp, generator=gen) > 0.5)).cuda()
    return dict(y=rnd(n, C, *sp), v=rnd(n, C, *sp), sigma=(15.0 + 20.0 * torch.rand(n, generator=gen)).cuda(),
                smap=(15.0 + 20.0 * torch.rand((n, 1) + sp, generator=gen)).cuda(), zp=sparse(), za=sparse(),
                zdp=sparse(), zda=sparse(), wx=rnd(n, C, *sp), wxd=rnd(n, C, *sp), wz=rnd(n, M, *sp), wzd=rnd(n, M, *sp))


def _csr_train(cva, net, d, out, case, both, sigma="sigma", ana=False):
    """temporal.csr_step with y, sigma and the neighbour codes requiring grad; the loss on xhat and z_K.  `ana`: a
    matrix-core case, whose images are fat too (recorded as folds)."""
    import torch
    thin = _fold if ana else (lambda t: t.detach().cpu().numpy())
    leaves = {k: d[k].clone().requires_grad_() for k in ("y", sigma, "zp") + (("za",) if both else ())}
    with cva.ops.trace() as tr:
        xhat, z = cva.temporal.csr_step(net, leaves["y"], leaves["zp"], leaves.get("za"), leaves[sigma])
        ((xhat * d["wx"]).sum() + (z * d["wz"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"] = thin(xhat), _fold(z)
    for k, t in leaves.items():
        g = t.grad
        out[f"{case}/d{'sigma' if k == sigma else k}"] = _fold(g) if k in ("zp", "za") else thin(g) if k == "y" else g.cpu().numpy()
    _grads(net, out, case)
    _finish(tr, out, case, ana)


def _csr_tangent(cva, net, d, out, case):
    """jvp_recurrent with both neighbours and their tangents, forward and backward."""
    import torch
    leaves = {k: d[k].clone().requires_grad_() for k in ("zp", "zdp", "za", "zda")}
    with cva.ops.trace() as tr:
        xhat, xdot, z, zd = net.jvp_recurrent(d["y"], d["v"], leaves["zp"], leaves["zdp"], leaves["za"], leaves["zda"],
                                              d["sigma"])
        ((xhat * d["wx"]).sum() + (xdot * d["wxd"]).sum() + (z * d["wz"]).sum() + (zd * d["wzd"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/xdot"] = xhat.detach().cpu().numpy(), xdot.detach().cpu().numpy()
    out[case + "/z"], out[case + "/zd"] = _fold(z), _fold(zd)
    for k, t in leaves.items():
        out[f"{case}/d{k}"] = _fold(t.grad)
    _grads(net, out, case)
    _finish(tr, out, case)


def _plain_data(n, C, M, sp, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    return dict(y=rnd(n, C, *sp), v=rnd(n, C, *sp), sigma=(15.0 + 20.0 * torch.rand(n, generator=gen)).cuda(),
                wx=rnd(n, C, *sp), wxd=rnd(n, C, *sp), wz=rnd(n, M, *sp), wzd=rnd(n, M, *sp))


def _train(cva, net, d, out, case):
    import torch
    y, sg = d["y"].clone().requires_grad_(), d["sigma"].clone().requires_grad_()
    with cva.ops.trace() as tr:
        xhat, z = net(y, sg)
        ((xhat * d["wx"]).sum() + (z * d["wz"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"] = _fold(xhat), _fold(z)
    out[case + "/dy"], out[case + "/dsigma"] = _fold(y.grad), sg.grad.cpu().numpy()
    _param_grads(net, out, case)
    _finish(tr, out, case, True)


def _tangent(cva, net, d, out, case):
    import torch
    A, B = net._filters()
    with cva.ops.trace() as tr:
        xhat, xdot, z, zd = cva.loop.run_tangent(d["y"], d["v"], None, d["sigma"] / 255.0, net.t, A, B, net.s, codes=True)
        ((xhat * d["wx"]).sum() + (xdot * d["wxd"]).sum() + (z * d["wz"]).sum() + (zd * d["wzd"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/xdot"] = _fold(xhat), _fold(xdot)
    out[case + "/z"], out[case + "/zd"] = _fold(z), _fold(zd)
    _param_grads(net, out, case)
    _finish(tr, out, case, True)


def _residual(cva, out, case):
    """One training step of CDLNetVideo(residual=True), K 2, M 16, on a clip of three frames."""
    import torch
    net = _detie(cva.CDLNetVideo(K=2, M=16, P=[3, 3, 3], s=1, C=1, t0=0.0, adaptive=True, init=False, residual=True), 41)
    with torch.no_grad():
        net.t.mul_(0.1)                              # the blocks' codes are small: keep about half of them
    gen = torch.Generator().manual_seed(42)
    y = torch.randn((1, 1, 3, 13, 22), generator=gen).cuda()
    wx = torch.randn(y.shape, generator=gen).cuda()
    wz = torch.randn((1, 16, 3, 13, 22), generator=gen).cuda()
    with cva.ops.trace() as tr:
        xhat, z = net(y, 25.0)
        ((xhat * wx).sum() + (z * wz).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"] = xhat.detach().cpu().numpy(), _fold(z)
    _grads(net, out, case)
    _finish(tr, out, case)


def _vgg(cva, out, case):
    """metrics.perceptual_frames forward and backward on the smallest frame of tests/test_gpu_perceptual.py."""
    import torch
    gen = torch.Generator().manual_seed(51)
    sd = {}
    for i in cva.metrics.VGG_CONVS:
        o, c = cva.metrics.VGG_SHAPES[i]
        sd[f"{i}.weight"] = torch.randn((o, c, 3, 3), generator=gen) * (2.0 / (o * 9)) ** 0.5
        sd[f"{i}.bias"] = torch.randn((o,), generator=gen) * 0.05
    x = cva.utils.synthetic_clip((1, 1, 3, 37, 50), seed=52)
    o_ = (x + 0.1 * torch.randn(x.shape, generator=gen)).clamp(0, 1).cuda().requires_grad_()
    t_ = x.cuda().requires_grad_()
    with cva.ops.trace() as tr:
        val = cva.metrics.perceptual_frames(o_, t_, sd)
        val.backward(torch.tensor(0.7, device="cuda"))
        torch.cuda.synchronize()
    out[case + "/value"] = val.detach().cpu().numpy().reshape(1)
    out[case + "/doutput"], out[case + "/dtarget"] = o_.grad.cpu().numpy(), t_.grad.cpu().numpy()
    _finish(tr, out, case)


def _single_banks(cva, out):
    import torch
    o = cva.ops
    for i, (order, M, C, P, tr_) in enumerate(GABOR):
        gen = torch.Generator().manual_seed(5)
        alpha = torch.randn(order, M, C, 1, 1, generator=gen).cuda()
        a = (torch.randn(order, M, C, 2, generator=gen) * 0.4).cuda()
        w0 = torch.randn(order, M, C, 2, generator=gen).cuda()
        psi = torch.randn(order, M, C, generator=gen).cuda()
        up = torch.randn((M, C, P, P), generator=gen).cuda()
        case = f"gabor/{i}"
        with o.trace() as tr:
            w = o.gabor_filters(alpha, a, w0, psi, P, tr_)
            grads = o.gabor_filters_bwd(alpha, a, w0, psi, up, P, tr_)
            torch.cuda.synchronize()
        out[case + "/w"] = w.cpu().numpy()
        for name, g in zip(("dalpha", "da", "dw0", "dpsi"), grads):
            out[f"{case}/{name}"] = g.cpu().numpy()
        _finish(tr, out, case)
    gen = torch.Generator().manual_seed(6)
    w = torch.randn((6, 2, 5, 5), generator=gen)
    w *= torch.tensor([0.02, 0.1, 0.14, 0.2, 1.0, 0.0]).reshape(6, 1, 1, 1)      # norms on both sides of 1, and a zero filter
    norms = w.flatten(1).norm(dim=1)
    assert int((norms < 1).sum()) >= 2 and int((norms > 1).sum()) >= 2 and float(norms[5]) == 0.0
    w = w.cuda()
    with o.trace() as tr:
        got = o.project_filters_(w)
        torch.cuda.synchronize()
    assert got is w
    out["project/w"] = w.cpu().numpy()
    _finish(tr, out, "project")


def compute():
    """{name: numpy array} of every recorded quantity."""
    import cdlnet_video_amd as cva
    loop = cva.loop
    assert loop.BACKEND == "auto" and loop.PRECISION == "split3" and loop.CODE_LAYOUT == "blocked"
    out = {}
    C, M, sp, P = CSR_GEOM
    d = _csr_data(N, C, M, sp, 61)
    mk = lambda cls, seed: _detie(cls(K=K, M=M, P=P, s=1, C=C, t0=0.0, adaptive=True, init=False), seed)
    f1, f2 = mk(cva.CDLNet_CSR, 62), mk(cva.CDLNet_CSRf2, 63)
    _csr_train(cva, f1, d, out, "csr/f1/train", False)
    _csr_train(cva, f2, d, out, "csr/f2/train", True)
    _csr_train(cva, f2, d, out, "csr/f2/map", True, sigma="smap")
    _csr_tangent(cva, f2, d, out, "csr/f2/tangent")

    loop.set_backend("generic")
    try:
        n2, C2, M2, sp2, P2 = MFMA_2D
        net = _detie(cva.CDLNet(K=K, M=M2, P=P2, s=1, C=C2, t0=0.0, adaptive=True, init=False), 71)
        _train(cva, net, _plain_data(n2, C2, M2, sp2, 72), out, "mfma/train")
        n3, C3, M3, sp3, P3 = MFMA_3D
        vid = _detie(cva.CDLNetVideo(K=K, M=M3, P=list(P3), s=1, C=C3, t0=0.0, adaptive=True, init=False), 73)
        _tangent(cva, vid, _plain_data(n3, C3, M3, sp3, 74), out, "mfma/tangent")
        csr = _detie(cva.CDLNet_CSRf2(K=K, M=M2, P=P2, s=1, C=C2, t0=0.0, adaptive=True, init=False), 75)
        _csr_train(cva, csr, _csr_data(n2, C2, M2, sp2, 76), out, "mfma/csr", True, ana=True)
    finally:
        loop.set_backend("auto")

    _residual(cva, out, "residual/dense")
    old = os.environ.get("CDL_MFMA_DENSE")
    os.environ["CDL_MFMA_DENSE"] = "0"
    cva._lib.reload_options()
    try:
        _residual(cva, out, "residual/valu")
    finally:
        if old is None:
            del os.environ["CDL_MFMA_DENSE"]
        else:
            os.environ["CDL_MFMA_DENSE"] = old
        cva._lib.reload_options()

    _vgg(cva, out, "vgg/step")
    _single_banks(cva, out)
    return out


if __name__ == "__main__":
    import numpy as np
    np.savez_compressed(sys.argv[1], **compute())
    print("wrote", sys.argv[1])
