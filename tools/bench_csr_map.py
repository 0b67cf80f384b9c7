#!/usr/bin/env python3
"""Timings of the CSR nets with a noise-level map, device events, forms alternated in one process
after warming all of them (the protocol of tools/bench_csr_tangent.py).  Geometry of argscsr.json (CDLNet_CSRf2, K = 30,
M = 169, P = 9, s = 2), one and eight 256 x 256 frames, both neighbours, forward and forward + backward:

    map          temporal.csr_step with an (N,1,128,128) map: one autograd node over the one-call sweeps
    blocks       the same loop composed from cva.functional (analysis, synthesis, prox_csr_f2), its thresholds formed by
                 torch as t0 + c * t1: what there was before csr_step
    per_sample   temporal.csr_step with one level per sample (no map)

    python tools/bench_csr_map.py --steps 7 --warmup 2 [--out profiles/csr_map.json]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from bench_csr_tangent import timed          # noqa: E402

SIZES = [(1, 256), (8, 256)]


def forms_for(cva, net, n, size):
    import torch
    F = cva.functional
    K, s = net.K, net.s
    y = torch.rand(n, 1, size, size, device="cuda")
    with torch.no_grad():
        _, z0 = net(y, None, None, 25.0)
    gen = torch.Generator().manual_seed(n)
    sig_map = (10.0 + 30.0 * torch.rand((n, 1, size // s, size // s), generator=gen)).cuda()
    sig_n = (10.0 + 30.0 * torch.rand((n, 1, 1, 1), generator=gen)).cuda()
    A, B = [m.weight for m in net.A], [m.weight for m in net.B]

    def from_blocks():
        c = sig_map / 255.0
        thr = lambda p, k: p[k, :1] + c * p[k, 1:2]
        yp, params, _ = F.pre_process(y, s)
        z = None
        for k in range(K):
            if k == 0:
                u = F.analysis(yp, A[0], s)
            else:
                u = F.analysis(F.synthesis(z, B[k], s, sub=yp), A[k], s, alpha=-1.0, add=z)
            z = F.prox_csr_f2(u, z0, z0, thr(net.t, k), thr(net.g1, k), thr(net.g2, k))
        return F.post_process(F.synthesis(z, B[0], s), params), z

    calls = {"map": lambda: cva.temporal.csr_step(net, y, z0, z0, sig_map), "blocks": from_blocks,
             "per_sample": lambda: cva.temporal.csr_step(net, y, z0, z0, sig_n)}

    def fwd(call):
        with torch.no_grad():
            call()

    def fwd_bwd(call):
        for p in net.parameters():
            p.grad = None
        xhat, z = call()
        (xhat.square().mean() + 0.05 * z.abs().mean()).backward()

    out = {}
    for name, call in calls.items():
        out[f"fwd_{name}_{n}x{size}"] = lambda call=call: fwd(call)
        out[f"fwd_bwd_{name}_{n}x{size}"] = lambda call=call: fwd_bwd(call)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    import cdlnet_video_amd as cva

    torch.manual_seed(1)
    net = cva.CDLNet_CSRf2(K=30, M=169, P=9, s=2, C=1, t0=5e-3, adaptive=True, init=False).cuda()
    with torch.no_grad():
        for k in range(30):
            net.A[k].weight.mul_(0.02)
            net.B[k].weight.mul_(0.02)
        net.g1.fill_(0.5)
        net.g2.fill_(0.5)
        for p in (net.t, net.g1, net.g2):
            p[:, 1] = 0.2 * p[:, 0]
    times = {}
    for n, size in SIZES:
        times.update(timed(forms_for(cva, net, n, size), a.steps, a.warmup))
    ms = {f: round(statistics.median(t), 3) for f, t in times.items()}
    res = {"workload": "CDLNet_CSRf2 K30 M169 P9 s2, both neighbours, 256 x 256", "steps": a.steps, "warmup": a.warmup,
           "ms": ms,
           "spread_pct": {f: round(100.0 * (max(t) - min(t)) / statistics.median(t), 2) for f, t in times.items()},
           "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}
    res["blocks_over_map"] = {k.replace("_map_", "_"): round(ms[k.replace("_map_", "_blocks_")] / v, 3)
                              for k, v in ms.items() if "_map_" in k}
    res["map_over_per_sample"] = {k.replace("_map_", "_"): round(v / ms[k.replace("_map_", "_per_sample_")], 3)
                                  for k, v in ms.items() if "_map_" in k}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
