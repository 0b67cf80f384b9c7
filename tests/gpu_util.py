"""Shared helpers for the -m gpu parity tests (they call the product through its C ABI)."""
import os

import torch

from conftest import ROOT, load_golden, rel_err   # noqa: F401

LOG = os.path.join(ROOT, "gpurun_out", "parity_log.txt")


def log(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


_SITES = None


def launch_sites(trace):
    """{launch-site id: [records]} of a cva.ops.trace(): the records mapped onto the `kernel<<<...>>>` sites of the
    sources by tools/launch_coverage.py (ids like "cdl_synth_mfma.hip:k_synth_m<PH,PW,SW,4>").  A record that fits no
    site, or several, is an error of the trace notes."""
    global _SITES
    if _SITES is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location("launch_coverage", os.path.join(ROOT, "tools", "launch_coverage.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _SITES = (mod, mod.index(mod.scan_sources()))
    mod, by_check = _SITES
    out = {}
    for r in trace:
        sid = mod.site_of(by_check, (r.file, r.line, r.func, r.note))
        assert sid is not None, f"trace record that names no single launch site: {r}"
        out.setdefault(sid, []).append(r)
    return out


def check(name, got, ref, tol):
    """Assert max|got-ref|/max|ref| < tol and record the measured value."""
    err = rel_err(got.detach().float().cpu(), ref.detach().float().cpu())
    log(f"{name:60s} rel_err={err:.3e} tol={tol:.1e}")
    assert err < tol, f"{name}: rel_err {err:.3e} >= {tol:.1e}"
    return err


def hyper(g):
    K, M, P, s, C = g["hyper"]
    P = tuple(g["P3"]) if "P3" in g else P
    return K, M, P, s, C


def build_from_golden(g, kind, **extra):
    """Construct the product module for a fixture and load the reference's state_dict into it."""
    import cdlnet_video_amd as cva
    K, M, P, s, C = hyper(g)
    if kind == "2d":
        net = cva.CDLNet(K=K, M=M, P=P, s=s, C=C, t0=0.0, adaptive=True, init=False)
    elif kind == "3d":
        net = cva.CDLNetVideo(K=K, M=M, P=list(P), s=s, C=C, t0=0.0, adaptive=True, init=False)
    else:
        net = cva.GDLNet(K=K, M=M, P=P, s=s, C=C, t0=0.0, order=g["order"], shared=g["shared"],
                         init=False, **extra)
    net.load_state_dict(g["sd"])
    return net.cuda()
