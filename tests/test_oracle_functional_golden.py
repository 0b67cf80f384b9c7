"""The CPU oracle with thresholds shaped like a noise-level map (oracle/cdl_oracle.py: prox_csr, prox_csr_f2, ista_csr with
`sigma` a map) replayed against fixtures generated from the unmodified reference (tools/make_golden_functional.py).  Pins
the oracle for what tests/test_gpu_functional.py compares the building blocks with."""
import torch

from conftest import load_golden, rel_err
from oracle import cdl_oracle as O

TOL = 2e-6


def prox_leaves(g):
    return {k: g[k].clone().requires_grad_(True) for k in ("u", "zp", "za", "c", "t", "g1", "g2")}


def prox_call(name, v):
    thr = lambda p: p[0] + v["c"] * p[1]
    if name == "csr":
        return O.prox_csr(v["u"], v["zp"], thr(v["t"]), thr(v["g1"]))
    return O.prox_csr_f2(v["u"], v["zp"], v["za"], thr(v["t"]), thr(v["g1"]), thr(v["g2"]))


def test_prox_maps_with_map_shaped_thresholds():
    g = load_golden("p0_prox_map_thresholds")
    assert bool((g["t"][0] < 0).any() or (g["g1"][0] < 0).any() or (g["g2"][0] < 0).any())
    for name in ("csr", "f2"):
        v = prox_leaves(g)
        out = prox_call(name, v)
        assert torch.equal(out.detach(), g[f"{name}_out"]), name
        (out * g["G"]).sum().backward()
        seen = 0
        for key, leaf in v.items():
            ref = g.get(f"{name}_d{key}")
            if ref is None:
                assert leaf.grad is None, (name, key)
                continue
            assert leaf.grad.shape == ref.shape
            assert rel_err(leaf.grad, ref) < TOL, (name, key)
            seen += 1
        assert seen == (5 if name == "csr" else 7)


def test_csrf2_call_with_a_sigma_map():
    g = load_golden("p1_csrf2_sigma_map")
    K, M, P, s, C = g["hyper"]
    sd = {k: v.clone().requires_grad_(True) for k, v in g["sd"].items() if k != "D.weight"}
    sd["D.weight"] = sd["B.0.weight"]
    y, sg, zp, za = (g[k].clone().requires_grad_(True) for k in ("y", "sigma", "zp", "za"))
    xhat, z = O.ista_csr(sd, y, zp, za, K=K, P=P, s=s, sigma=sg, adaptive=True, variant="f2")
    assert rel_err(xhat, g["xhat"]) < TOL and rel_err(z, g["z"]) < TOL
    assert int(((z != 0) != (g["z"] != 0)).sum()) == 0
    loss = torch.mean((g["x"] - xhat) ** 2) + 0.05 * z.abs().mean()
    assert abs(float(loss.detach()) - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"]))
    loss.backward()
    for key, leaf in (("dy", y), ("dsigma", sg), ("dzp", zp), ("dza", za)):
        assert leaf.grad.shape == g[key].shape
        assert rel_err(leaf.grad, g[key]) < 5e-5, key
    seen = 0
    for key, ref in g["grad"].items():
        assert rel_err(sd[key].grad, ref) < 5e-5, key
        seen += 1
    assert seen == 2 * K + 3
