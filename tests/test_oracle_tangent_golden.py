"""CPU: the oracle's fixed-support difference -- the reference value of every tangent test on the device -- against the
reference's own Jacobian-vector product (fixtures j1..j3, tools/make_golden_tangent.py: the unmodified reference under
torch.autograd.forward_ad) and against torch.func.jvp of the oracle in float64."""
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import cdl_oracle as O
from tangent_util import func_jvp_and_grads, tangent_and_grads

FIXTURES = ["j1_2d_s2_odd", "j2_jdd_c3_mask", "j3_3d_p555"]


def _setup(name):
    g = load_golden(name)
    K, M, P, s, C = g["hyper"]
    P = tuple(g["P3"]) if "P3" in g else P
    nd = g["y"].dim() - 2
    kw = dict(K=K, P=P, s=s, sigma=g["sigma"], adaptive=True, mask=g.get("mask"), ndim=nd)
    with torch.no_grad():
        _, codes = O.ista(g["sd"], g["y"], all_codes=True, **kw)      # fp32 supports: those of the reference's run
    y, w = g["y"].double(), g["w"].double()
    loss_fn = lambda xhat, xdot: torch.mean(w * xdot) + torch.mean((xhat - y) ** 2)
    return g, kw, codes, loss_fn


@pytest.fixture(scope="module", params=FIXTURES)
def case(request):
    g, kw, codes, loss_fn = _setup(request.param)
    return request.param, g, kw, loss_fn, tangent_and_grads(g["sd"], g["y"], g["v"], codes, loss_fn, **kw)


def test_fixed_support_difference_equals_the_reference_jvp(case):
    name, g, kw, loss_fn, (xhat, xdot, loss, grads) = case
    assert rel_err(xhat.float(), g["xhat"]) < 2e-6
    assert rel_err(xdot.float(), g["xdot"]) < 2e-6, name
    assert abs(loss - g["loss"]) < 2e-6 * max(1.0, abs(g["loss"]))
    assert set(g["grad"]) >= {k for k in grads if k != "g"}
    for k, ref in g["grad"].items():
        assert rel_err(grads[k].float(), ref) < 2e-6, f"{name} grad {k}"


def test_fixed_support_difference_equals_func_jvp_in_float64(case):
    name, g, kw, loss_fn, (xhat, xdot, loss, grads) = case
    xh, xd, lo, gr = func_jvp_and_grads(g["sd"], g["y"], g["v"], loss_fn, **kw)
    assert rel_err(xhat, xh) < 1e-12 and rel_err(xdot, xd) < 1e-12, name
    assert abs(loss - lo) < 1e-12 * max(1.0, abs(lo))
    for k in grads:
        if k != "g":
            assert rel_err(grads[k], gr[k]) < 1e-12, f"{name} grad {k}"


def test_thresholds_get_no_gradient_from_the_tangent(case):
    """The thresholds do not appear in the tangent recursion: d mean(w xdot) / dt = 0 exactly."""
    name, g, kw, loss_fn, _ = case
    with torch.no_grad():
        _, codes = O.ista(g["sd"], g["y"], all_codes=True, **kw)
    w = g["w"].double()
    _, _, _, grads = tangent_and_grads(g["sd"], g["y"], g["v"], codes, lambda xhat, xdot: torch.mean(w * xdot), **kw)
    assert float(grads["t"].abs().max()) < 1e-15
