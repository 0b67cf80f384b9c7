#!/usr/bin/env python3
"""Timings around the CSR tangent under a noise-level map: the sibling of tools/bench_csr_tangent.py,
same net (argscsr.json geometry: K = 30, M = 169, P = 9, s = 2), same sizes (1x1x128x128 and 8x1x256x256), device events,
forms alternated in one process after warming all of them.

Gated against a parent tree (`--parent PATH --pairs 5`): fresh child processes of the two trees, alternated, each measuring

    primal       the both-neighbour CDLNet_CSRf2 forward, per-sample sigma
    tangent      jvp_recurrent of the same call, per-sample sigma (k_prox_fwd's row form: the kernel the map branch was added to)

and the medians of the two trees may differ by no more than the parent's own run-to-run spread (the rule of section 22).

Recorded without a gate, this tree only:

    jvp_map      csr_jvp_step of the same call with a (N,1,*code grid) map, against `tangent`
    exact / exact_map
                 train_step_clip(mcsure="exact") of CDLNet_CSR on a 2-frame clip of 4 x 128 x 128 crops with a (20, 30) range,
                 and with one image-resolution level map per frame as noise_std
    bench        `bench.py --gpus 1` of both trees (with --parent), the flagship workload

    python tools/bench_csr_tangent_map.py --parent PATH --pairs 5 --out profiles/csr_tangent_map.json

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_csr_tangent import SIZES, timed          # noqa: E402


def summary(times):
    return {"ms": {f: round(statistics.median(t), 3) for f, t in times.items()},
            "spread_pct": {f: round(100.0 * (max(t) - min(t)) / statistics.median(t), 2) for f, t in times.items()},
            "all_ms": {f: [round(v, 3) for v in t] for f, t in times.items()}}


def level_map(shape, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.0, 1.0, shape[-1]).reshape((1,) * (len(shape) - 1) + (shape[-1],))
    return (12.0 + 20.0 * (0.7 * ramp + 0.3 * torch.rand(shape, generator=gen))).cuda()


def measure(a):
    """The forms of one tree (`--root`); `--with-map`: the map forms beside the gated ones."""
    sys.path.insert(0, os.path.abspath(a.root))
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
            v, zd = torch.randn_like(y), torch.randn_like(z0)
            forms[f"primal_{n}x{size}"] = lambda y=y, z0=z0: net(y, z0, z0, 25.0)
            forms[f"tangent_{n}x{size}"] = lambda y=y, z0=z0, v=v, zd=zd: net.jvp_recurrent(y, v, z0, zd, z0, zd, 25.0)
            if a.with_map:
                sig = level_map((n, 1, size // 2, size // 2), n)
                forms[f"jvp_map_{n}x{size}"] = lambda y=y, z0=z0, v=v, zd=zd, sig=sig: \
                    cva.temporal.csr_jvp_step(net, y, v, z0, zd, z0, zd, sigma=sig)
        times = timed(forms, a.steps, a.warmup)
    if a.with_map:
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
        nstd = torch.stack([level_map((4, 1, 128, 128), 10 + t) for t in range(2)], dim=2)
        gen = torch.Generator().manual_seed(3)
        step = lambda level: cva.train_step_clip(csr, opt, clip, level, clip_grad=5e-2, generator=gen, mcsure="exact")
        times.update(timed({"exact": lambda: step((20, 30)), "exact_map": lambda: step(nstd)}, a.steps, a.warmup))
    return summary(times)


def child(root, a, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--steps", str(a.steps), "--warmup",
           str(a.warmup), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child on {root} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def flagship(root, a):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "2"], cwd=root,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py in {root} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    r = json.loads(out.stdout.strip().splitlines()[-1])
    return {k: r[k] for k in ("value", "unit", "ms_per_step", "steps") if k in r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--with-map", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return
    res = {"workload": "CDLNet_CSRf2 / CDLNet_CSR K30 M169 P9 s2", "steps": a.steps, "warmup": a.warmup}
    if a.parent:                                       # fresh processes, one with the device open at a time, alternated
        runs = {"parent": [], "this": []}
        for i in range(a.pairs):
            for tag, root in ((("parent", a.parent), ("this", HERE)) if i % 2 == 0 else (("this", HERE), ("parent", a.parent))):
                runs[tag].append(child(root, a)["ms"])
        gate = {}
        for f in runs["parent"][0]:
            p, t = [r[f] for r in runs["parent"]], [r[f] for r in runs["this"]]
            mp, mt = statistics.median(p), statistics.median(t)
            gate[f] = {"parent_ms": p, "this_ms": t, "parent_median": mp, "this_median": mt,
                       "parent_spread_ms": round(max(p) - min(p), 3), "diff_ms": round(mt - mp, 3),
                       "within_parent_spread": abs(mt - mp) <= max(p) - min(p)}
        res["vs_parent"] = gate
        res["gate_passed"] = all(v["within_parent_spread"] for v in gate.values())
        res["bench_py"] = {"parent": flagship(a.parent, a), "this": flagship(HERE, a)}
    a.root = HERE
    res.update(child(HERE, a, ("--with-map",)))
    ms = res["ms"]
    res["jvp_map_over_tangent"] = {f"{n}x{s}": round(ms[f"jvp_map_{n}x{s}"] / ms[f"tangent_{n}x{s}"], 3) for n, s in SIZES}
    res["exact_map_over_exact"] = round(ms["exact_map"] / ms["exact"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
