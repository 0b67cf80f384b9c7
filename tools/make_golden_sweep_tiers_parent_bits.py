#!/usr/bin/env python3
"""Bits and launch order of the sweep tiers through the nets' public calls, recorded on the commit BEFORE the tiers got one
routing rule, one table and one host loop:

    python tools/make_golden_sweep_tiers_parent_bits.py tests/golden/t0_sweep_tiers_parent_bits.npz   # on that commit, on the device

tests/test_gpu_sweep_tiers.py calls `compute()` on the current commit and compares bit for bit, and the launch lists
(`<case>/launches`: the launch sites of the case in order, as tools/launch_coverage.py names them) as lists.

Cases: the four geometries of tests/test_gpu_host_plumbing.py (N = 2, K = 3: a partial tile in both axes of each tier's
kernel).  On each a training step (y and a per-sample sigma require grad, the loss on xhat and z_K) and the tangent sweep
with codes, forward and backward; on `generic` also a noise-level map and a step on the fp32 VALU kernels, on `fused` both
code layouts, on `strip` forward_generator (handed-out codes force the "nchw" layout).  Fat tensors (codes) are recorded
as two 64-bit folds of their int32 bit patterns, sum and xor.
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, K = 2, 3
# tier -> (C, M, spatial, P, stride): tests/test_gpu_host_plumbing.py::GEOMS
GEOMS = {
    "generic": (2, 5, (13, 11), (3, 3), 1),
    "fused": (1, 32, (20, 70), (5, 5), 1),
    "tile": (1, 24, (3, 17, 33), (3, 3, 3), 1),
    "strip": (1, 24, (20, 36), (3, 3), 2),
}
_SITES = None


def _site_ids(trace):
    """The launch sites of a trace's records, in order (tests/gpu_util.py::launch_sites keeps no order)."""
    global _SITES
    if _SITES is None:
        spec = importlib.util.spec_from_file_location("launch_coverage", os.path.join(ROOT, "tools", "launch_coverage.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _SITES = (mod, mod.index(mod.scan_sources()))
    mod, by_check = _SITES
    ids = [mod.site_of(by_check, (r.file, r.line, r.func, r.note)) for r in trace]
    assert None not in ids, [r for r, i in zip(trace, ids) if i is None]
    return ids


def _fold(t):
    """(sum, xor) of the int32 bit patterns of a float32 tensor, as int64."""
    import numpy as np
    bits = t.detach().contiguous().cpu().numpy().view(np.int32).astype(np.int64).ravel()
    return np.array([bits.sum(), np.bitwise_xor.reduce(bits)], dtype=np.int64)


def _net(cva, tier):
    """The tier's net with de-tied filters and thresholds that zero about half of every code; same bits on every call."""
    import torch
    C, M, sp, P, s = GEOMS[tier]
    if len(sp) == 3:
        net = cva.CDLNetVideo(K=K, M=M, P=list(P), s=s, C=C, t0=0.0, adaptive=True, init=False)
    else:
        net = cva.CDLNet(K=K, M=M, P=P[0], s=s, C=C, t0=0.0, adaptive=True, init=False)
    gen = torch.Generator().manual_seed(7 + len(tier))
    with torch.no_grad():
        for m in list(net.A) + list(net.B):
            m.weight.copy_(0.1 * torch.randn(m.weight.shape, generator=gen))
        net.t.copy_(0.3 * torch.rand(net.t.shape, generator=gen))
    return net.cuda()


def _data(tier):
    """y, v, sigma (N,), a sigma map on the code grid, and the loss weights of xhat / xdot (image) and z / zd (code)."""
    import torch
    C, M, sp, P, s = GEOMS[tier]
    gen = torch.Generator().manual_seed(31 + len(tier))
    grid = tuple(-(-d // s) for d in sp)
    rnd = lambda *shape: torch.randn(shape, generator=gen).cuda()
    return dict(y=rnd(N, C, *sp), v=rnd(N, C, *sp), sigma=(15.0 + 20.0 * torch.rand(N, generator=gen)).cuda(),
                smap=(15.0 + 20.0 * torch.rand((N, 1) + grid, generator=gen)).cuda(),
                wx=rnd(N, C, *sp), wxd=rnd(N, C, *sp), wz=rnd(N, M, *grid), wzd=rnd(N, M, *grid))


def _param_grads(net, out, case):
    import torch
    out[case + "/dt"] = net.t.grad.detach().cpu().numpy()
    out[case + "/dA"] = torch.stack([m.weight.grad for m in net.A]).cpu().numpy()
    out[case + "/dB"] = torch.stack([m.weight.grad for m in net.B]).cpu().numpy()
    net.zero_grad(set_to_none=True)


def _train_step(cva, net, d, out, case, sigma="sigma"):
    import numpy as np
    import torch
    y, sg = d["y"].clone().requires_grad_(), d[sigma].clone().requires_grad_()
    with cva.ops.trace() as tr:
        xhat, z = net(y, sg)
        ((xhat * d["wx"]).sum() + (z * d["wz"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/z"] = xhat.detach().cpu().numpy(), _fold(z)
    out[case + "/dy"], out[case + "/dsigma"] = y.grad.cpu().numpy(), sg.grad.cpu().numpy()
    _param_grads(net, out, case)
    out[case + "/launches"] = np.array(_site_ids(tr))


def _tangent_step(cva, net, d, out, case):
    import numpy as np
    import torch
    A, B = net._filters()
    c = d["sigma"] / 255.0
    with cva.ops.trace() as tr:
        xhat, xdot, z, zd = cva.loop.run_tangent(d["y"], d["v"], None, c, net.t, A, B, net.s, codes=True)
        ((xhat * d["wx"]).sum() + (xdot * d["wxd"]).sum() + (z * d["wz"]).sum() + (zd * d["wzd"]).sum()).backward()
        torch.cuda.synchronize()
    out[case + "/xhat"], out[case + "/xdot"] = xhat.detach().cpu().numpy(), xdot.detach().cpu().numpy()
    out[case + "/z"], out[case + "/zd"] = _fold(z), _fold(zd)
    _param_grads(net, out, case)
    out[case + "/launches"] = np.array(_site_ids(tr))


def _generator_step(cva, net, d, out, case):
    import numpy as np
    import torch
    with cva.ops.trace() as tr:
        *codes, xhat = net.forward_generator(d["y"], d["sigma"])
        (xhat * d["wx"]).sum().backward()
        torch.cuda.synchronize()
    assert len(codes) == K and all(tuple(z.shape) == tuple(d["wz"].shape) for z in codes)
    out[case + "/xhat"] = xhat.detach().cpu().numpy()
    out[case + "/codes"] = np.stack([_fold(z) for z in codes])
    _param_grads(net, out, case)
    out[case + "/launches"] = np.array(_site_ids(tr))


def compute():
    """{name: numpy array} of every recorded quantity."""
    import cdlnet_video_amd as cva
    loop = cva.loop
    assert loop.BACKEND == "auto" and loop.PRECISION == "split3" and loop.CODE_LAYOUT == "blocked"
    out = {}
    for tier in GEOMS:
        net, d = _net(cva, tier), _data(tier)
        if tier == "fused":
            for lay in ("blocked", "nchw"):
                loop.set_code_layout(lay)
                try:
                    _train_step(cva, net, d, out, f"fused/{lay}/train")
                    _tangent_step(cva, net, d, out, f"fused/{lay}/tangent")
                finally:
                    loop.set_code_layout("blocked")
            continue
        _train_step(cva, net, d, out, tier + "/train")
        _tangent_step(cva, net, d, out, tier + "/tangent")
        if tier == "generic":
            _train_step(cva, net, d, out, "generic/map", sigma="smap")
            with loop.precision_scope("fp32"):
                _train_step(cva, net, d, out, "generic/fp32")
        if tier == "strip":
            _generator_step(cva, net, d, out, "strip/generator")
    return out


if __name__ == "__main__":
    import numpy as np
    np.savez_compressed(sys.argv[1], **compute())
    print("wrote", sys.argv[1])
