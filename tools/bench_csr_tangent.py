#!/usr/bin/env python3
"""Timings of the CSR nets' tangent sweep and clip steps, device events, forms alternated in one
process after warming all of them (the protocol of tools/bench_sure.py):

    primal       the CSR forward of tools/profile_csr.py's net (argscsr.json geometry: K = 30, M = 169, P = 9, s = 2),
                 both-neighbour call, at 1x1x128x128 and at 8x1x256x256
    tangent      jvp_recurrent of the same call (primal + tangent sweep), under no_grad
    supervised   one supervised clip step (train_step_clip) of CDLNet_CSR on a 2-frame clip of 128 x 128 crops
    exact        the same step with mcsure="exact"

    python tools/bench_csr_tangent.py --steps 7 --warmup 2 [--out profiles/csr_tangent.json]
    python tools/bench_csr_tangent.py --primal-only                   # what a tree without jvp_recurrent can run: the
                                                                      # primal forms and the supervised step
    python tools/bench_csr_tangent.py --parent PATH --pairs 5 --out profiles/csr_tangent.json
        # additionally: `--primal-only` children of this tree and of the tree at PATH, alternated, `pairs` of them; the
        # gate is: the medians of the two trees differ by no more than the parent's own run-to-run spread
    python tools/bench_csr_tangent.py --blocks ...
        # additionally (no gate): the both-neighbour CSR-f2 forward + backward at 1x1x128x128 written from the blocks of
        # cva.functional against the net's own sweep

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 128), (8, 256)]


def timed(forms, steps, warmup):
    import torch
    names = list(forms)
    for _ in range(warmup):
        for f in names:
            forms[f]()
    torch.cuda.synchronize()
    times = {f: [] for f in names}
    for i in range(steps):
        for f in (names if i % 2 == 0 else names[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            forms[f]()
            t1.record()
            t1.synchronize()
            times[f].append(t0.elapsed_time(t1))
    return times


def measure(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
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
    forms = {}
    with torch.no_grad():
        for n, size in SIZES:
            y = torch.rand(n, 1, size, size, device="cuda")
            _, z0 = net(y, None, None, 25.0)
            forms[f"primal_{n}x{size}"] = lambda y=y, z0=z0: net(y, z0, z0, 25.0)
            if not a.primal_only:
                v, zd = torch.randn_like(y), torch.randn_like(z0)
                forms[f"tangent_{n}x{size}"] = lambda y=y, z0=z0, v=v, zd=zd: net.jvp_recurrent(y, v, z0, zd, z0, zd, 25.0)
        times = timed(forms, a.steps, a.warmup)
    if a.blocks:
        times.update(timed(block_forms(cva, net), a.steps, a.warmup))
    # the supervised step also under --primal-only: k_prox_bwd is then on the clock of the comparison with a parent tree
    torch.manual_seed(2)
    csr = cva.CDLNet_CSR(K=30, M=169, P=9, s=2, C=1, t0=5e-3, adaptive=True, init=False).cuda()
    with torch.no_grad():
        for bank in (csr.A, csr.B, csr.A2, csr.B2):
            for m in bank:
                m.weight.mul_(0.02)
        csr.t.fill_(2e-3)
        csr.t2.fill_(2e-3)
        csr.g.fill_(0.5)
    opt = torch.optim.Adam(csr.parameters(), lr=1e-4)
    clip = torch.stack([cva.utils.synthetic_clip((4, 1, 128, 128), seed=t) for t in range(2)], dim=2).cuda()
    gen = torch.Generator().manual_seed(3)
    step = lambda mode: cva.train_step_clip(csr, opt, clip, (20, 30), clip_grad=5e-2, generator=gen, mcsure=mode)
    steps = {"supervised": lambda: step(False)}
    if not a.primal_only:
        steps["exact"] = lambda: step("exact")
    times.update(timed(steps, a.steps, a.warmup))
    return {"ms": {f: round(statistics.median(t), 3) for f, t in times.items()},
            "spread_pct": {f: round(100.0 * (max(t) - min(t)) / statistics.median(t), 2) for f, t in times.items()},
            "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}


def block_forms(cva, net):
    """Forward + backward of the both-neighbour CDLNet_CSRf2 call at 1x1x128x128: the net's sweep, and the same loop written
    from cva.functional (per-sample sigma, so that both compute the same thing)."""
    import torch
    F = cva.functional
    y = torch.rand(1, 1, 128, 128, device="cuda")
    with torch.no_grad():
        _, z0 = net(y, None, None, 25.0)
    K, s, c = net.K, net.s, 25.0 / 255.0
    A, B = [m.weight for m in net.A], [m.weight for m in net.B]
    thr = lambda p, k: p[k, :1] + c * p[k, 1:2]

    def from_blocks():
        yp, params, _ = F.pre_process(y, s)
        z = None
        for k in range(K):
            if k == 0:
                u = F.analysis(yp, A[0], s)
            else:
                u = F.analysis(F.synthesis(z, B[k], s, sub=yp), A[k], s, alpha=-1.0, add=z)
            z = F.prox_csr_f2(u, z0, z0, thr(net.t, k), thr(net.g1, k), thr(net.g2, k))
        return F.post_process(F.synthesis(z, B[0], s), params), z

    def step(fwd):
        for p in net.parameters():
            p.grad = None
        xhat, z = fwd()
        (xhat.square().mean() + 0.05 * z.abs().mean()).backward()

    return {"csrf2_fwd_bwd_net_1x128": lambda: step(lambda: net(y, z0, z0, 25.0)),
            "csrf2_fwd_bwd_blocks_1x128": lambda: step(from_blocks)}


def child(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--primal-only", "--root", root, "--steps", str(a.steps), "--warmup",
           str(a.warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child on {root} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--primal-only", action="store_true")
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": "CDLNet_CSRf2 / CDLNet_CSR K30 M169 P9 s2", "steps": a.steps, "warmup": a.warmup}
    if a.parent:                                       # children first: one process with the device open at a time
        runs = {"parent": [], "this": []}
        for i in range(a.pairs):
            for tag, root in ((("parent", a.parent), ("this", HERE)) if i % 2 == 0 else (("this", HERE), ("parent", a.parent))):
                runs[tag].append(child(root, a))
        gate = {}
        for f in runs["parent"][0]:
            p, t = [r[f] for r in runs["parent"]], [r[f] for r in runs["this"]]
            mp, mt = statistics.median(p), statistics.median(t)
            gate[f] = {"parent_ms": p, "this_ms": t, "parent_median": mp, "this_median": mt,
                       "parent_spread_ms": round(max(p) - min(p), 3), "diff_ms": round(mt - mp, 3),
                       "within_parent_spread": abs(mt - mp) <= max(p) - min(p)}
        res["primal_vs_parent"] = gate
        res["gate_passed"] = all(v["within_parent_spread"] for v in gate.values())
    res.update(measure(a))
    if not a.primal_only:
        ms = res["ms"]
        res["tangent_over_primal"] = {f"{n}x{s}": round(ms[f"tangent_{n}x{s}"] / ms[f"primal_{n}x{s}"], 3) for n, s in SIZES}
        res["exact_over_supervised"] = round(ms["exact"] / ms["supervised"], 3)
    if a.blocks:
        ms = res["ms"]
        res["blocks_over_net"] = round(ms["csrf2_fwd_bwd_blocks_1x128"] / ms["csrf2_fwd_bwd_net_1x128"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
