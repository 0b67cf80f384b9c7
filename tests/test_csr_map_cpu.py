"""Noise-level maps and data gradients of the CSR nets without a GPU: the CPU oracle against the
fixtures of tools/make_golden_csr_map.py, the C ABI of the entry points that gained arguments, and the refusals of the new
surface that need no device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cdlnet_video_amd as cva
from conftest import ROOT, load_golden, rel_err
from csr_map_util import FIXTURES, VARIANT, replay
from oracle import cdl_oracle as O

TOL = 1e-5


@pytest.mark.parametrize("kind", sorted(FIXTURES))
def test_oracle_reproduces_the_fixture(kind):
    """oracle.ista_csr with the map (or the per-sample tensor) as `sigma` and autograd: every recorded value."""
    g = load_golden(FIXTURES[kind])
    K, M, P, s, C = g["hyper"]
    assert g["margin"] > 1e-6
    sd = {k: v.clone().requires_grad_(True) for k, v in g["sd"].items()}
    call = lambda y, zp, za, sigma: O.ista_csr(sd, y, zp, za, K=K, P=P, s=s, sigma=sigma, adaptive=True,
                                               variant=VARIANT[kind])
    loss, outs, leaves = replay(kind, g, call)
    for name, got in outs.items():
        assert rel_err(got, g[name]) < TOL, name
    assert abs(float(loss.detach()) - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"]))
    loss.backward()
    for name, t in leaves.items():
        assert t.grad.shape == g[name].shape, name            # dsigma in the shape sigma was given
        assert rel_err(t.grad, g[name]) < TOL, name
    n = 0
    for key, ref in g["grad"].items():                         # (a parameter the reference left without a gradient is absent)
        if sd[key].grad is None:                               # a parameter no call of the chain uses
            assert float(ref.abs().max()) == 0.0, key
            continue
        assert rel_err(sd[key].grad, ref) < TOL, key
        n += 1
    assert n >= 5


# ------------------------------------------------------------------------------------------ the C ABI
NEW_ARGS = {  # entry point: (its argument count before, the pointers it gained in front of the stream)
    "cdl_analysis_prox": (15, ("cmap", "tslope")),
    "cdl_prox_csr_bwd": (18, ("cmap", "tslope", "dcmap", "dsum_n")),
}
SAME_ARGC = {"cdl_ista_forward": 20, "cdl_ista_backward": 35}       # the sweeps reuse their nullable arguments


def _decl(header, name):
    return re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1))


def test_the_map_and_the_data_gradients_are_nullable_arguments_of_the_existing_entry_points():
    from cdlnet_video_amd import _lib
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    for name, (argc, args) in NEW_ARGS.items():
        sig = _lib.SIGNATURES[name]
        assert len(sig) == argc + len(args), name
        assert all(a is ctypes.c_void_p for a in sig[-1 - len(args):]), name       # the new pointers, then the stream
        names = [re.search(r"(\w+)\s*$", a).group(1) for a in _decl(header, name).split(",")]
        assert len(names) == len(sig), name
        assert tuple(names[-1 - len(args):]) == args + ("stream",), (name, names)
    for name, argc in SAME_ARGC.items():
        assert len(_lib.SIGNATURES[name]) == argc == len(_decl(header, name).split(",")), name
    for base in list(NEW_ARGS) + list(SAME_ARGC):                                  # no suffixed sibling
        for suffix in ("_map", "_cmap", "_smap", "_sigma"):
            name = base + suffix
            assert name not in _lib.SIGNATURES and name not in _lib.SIZE_T_FUNCS, name
            assert not re.search(rf"\b{name}\b", header), name
    src = open(os.path.join(ROOT, "cdlnet-video_amd", "csrc", "cdl_sweep.hip")).read()
    assert "plain loop only" not in src


def test_ops_gain_keyword_only_arguments():
    from cdlnet_video_amd import ops
    for fn, kws in ((ops.analysis_prox, ("cmap", "tslope")), (ops.prox_csr_bwd, ("cmap", "tslope", "dcmap", "dsum_n"))):
        params = inspect.signature(fn).parameters
        for kw in kws:
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None, (fn.__name__, kw)


# ------------------------------------------------------------------------------------------ refusals without a device
def _net(cls):
    return cls(K=2, M=4, P=5, s=1, C=1, t0=5e-3, adaptive=True, init=False)


@pytest.mark.parametrize("cls", [cva.CDLNet_CSR, cva.CDLNet_CSRf2])
def test_csr_step_refuses_cpu_tensors(cls):
    net = _net(cls)
    y, z = torch.rand(1, 1, 12, 12), torch.zeros(1, 4, 12, 12)
    for prev in (None, z):
        with pytest.raises(RuntimeError, match="no CPU compute path"):
            cva.temporal.csr_step(net, y, prev, sigma=torch.full((1, 1, 12, 12), 25.0))
    with pytest.raises(RuntimeError, match="no CPU"):
        cva.functional.ista_csr(y, z, None, 25.0, 1, net.t, net.t, None, [m.weight for m in net.A],
                                [m.weight for m in net.B], 1)


def test_a_mask_that_requires_grad_is_refused_before_any_device_work():
    net = _net(cva.CDLNet_CSRf2)
    y, z = torch.rand(1, 1, 12, 12), torch.zeros(1, 4, 12, 12)
    mask = torch.ones_like(y).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="mask"):
        cva.temporal.csr_step(net, y, z, z, sigma=25.0, mask=mask)
    with pytest.raises(NotImplementedError, match="mask"):
        cva.functional.ista_csr(y, z, None, 25.0, mask, net.t, net.g1, None, [m.weight for m in net.A],
                                [m.weight for m in net.B], 1)


def test_sigma_is_classified_as_the_nets_classify_it():
    """A map that does not broadcast to the code grid is net._noise_scale's ValueError, raised by the drivers' splitter
    and csr_step alike -- checked here on the classification itself, which needs no device."""
    from cdlnet_video_amd import temporal
    y = torch.rand(2, 1, 12, 12)
    assert temporal._is_sigma_map(torch.rand(2, 1, 12, 12), y) and temporal._is_sigma_map(torch.rand(1, 1, 12, 12), y)
    assert not temporal._is_sigma_map(torch.rand(2, 1, 1, 1), y) and not temporal._is_sigma_map(25.0, y)
    frames = [torch.rand(1, 1, 12, 12)] * 3
    split = temporal._per_frame_sigma(torch.rand(3, 1, 12, 12), frames)
    assert isinstance(split, list) and [tuple(s.shape) for s in split] == [(1, 1, 12, 12)] * 3
    with pytest.raises(ValueError, match="ambiguous"):                              # T equal to the batch size
        temporal._per_frame_sigma(torch.rand(3, 1, 12, 12), [torch.rand(3, 1, 12, 12)] * 3)
    one = torch.rand(1, 1, 12, 12)
    assert temporal._per_frame_sigma(one, frames) is one and temporal._per_frame_sigma(25.0, frames) == 25.0
