"""Noise-level maps (sigma per code pixel / per frame) on the CPU side: the oracle against the reference's s-fixtures
(tools/make_golden_sigmamap.py), the sigma classifier of the nets, the image-grid -> code-grid helper, and the C ABI
rule -- the map is a nullable argument of the existing entry points, not a suffixed sibling."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden, rel_err
from oracle import cdl_oracle as O
from sigmamap_util import FIXTURES, RESIDUAL_FIXTURE, fixture_args, loss_of, oracle_grads

TOL = 1e-5           # tests/test_datagrad_cpu.py


@pytest.mark.parametrize("name,kind", FIXTURES)
def test_oracle_matches_reference_with_a_map(name, kind):
    g = load_golden(name)
    assert g["sigma"].numel() not in (1, g["x"].shape[0])            # a map, not a per-sample form
    assert 10.0 <= float(g["sigma"].min()) and float(g["sigma"].max()) <= 40.0
    xhat, z, loss, grads, dy, ds = oracle_grads(g["sd"], g["x"], g["y"], g["w"], g["sigma"], **fixture_args(g, kind))
    assert rel_err(xhat, g["xhat"]) < TOL
    assert rel_err(z, g["z"]) < TOL
    assert abs(loss - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"]))
    assert rel_err(dy, g["dy"]) < TOL
    assert ds.shape == g["dsigma"].shape == g["sigma"].shape
    assert rel_err(ds, g["dsigma"]) < TOL
    for key, ref in g["grad"].items():
        if key == "g":                                               # unused parameter: no gradient on either side
            continue
        assert rel_err(grads[key], ref) < TOL, key


def test_oracle_matches_reference_residual_chain_with_a_map():
    g = load_golden(RESIDUAL_FIXTURE)
    K, M, Pd, Ph, Pw, s, C = g["hyper"]
    sd = {k: v.clone().requires_grad_(True) for k, v in g["sd"].items()}
    xhat, z = O.ista_video_residual(sd, g["y"], K=K, P=(Pd, Ph, Pw), s=s, sigma=g["sigma"], adaptive=True)
    assert rel_err(xhat, g["xhat"]) < TOL and rel_err(z, g["z"]) < TOL
    loss = loss_of(xhat, g["x"], g["w"])
    assert abs(float(loss.detach()) - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"]))
    loss.backward()
    for key, ref in g["grad"].items():
        assert rel_err(sd[key].grad, ref) < TOL, key


# ------------------------------------------------------------------------------------------ the classifier
def test_sigma_classifier_per_sample_forms_are_untouched():
    from cdlnet_video_amd.net import _noise_scale, _is_map
    N, grid = 3, (4, 5)
    for sigma in (25.0, torch.tensor(25.0), torch.tensor([25.0]), torch.full((1, 1, 1, 1), 25.0)):
        c = _noise_scale(sigma, True, N, "cpu", grid)
        assert not _is_map(c) and c.shape == (N,) and torch.equal(c, torch.full((N,), 25.0 / 255.0))
    per = torch.tensor([10.0, 20.0, 30.0])
    for sigma in (per, per.reshape(N, 1, 1, 1), per.reshape(1, N), per.reshape(N, 1)):
        c = _noise_scale(sigma, True, N, "cpu", grid)
        assert not _is_map(c) and torch.equal(c, per / 255.0)
    assert _noise_scale(None, True, N, "cpu", grid) is None
    assert _noise_scale(torch.rand(N, 1, 4, 5), False, N, "cpu", grid) is None      # adaptive=False ignores a map too
    # the documented ambiguity: a (1,1,H,W) map with H*W == N is N per-sample levels
    c = _noise_scale(torch.rand(1, 1, 4, 5), True, 20, "cpu", grid)
    assert not _is_map(c) and c.shape == (20,)


@pytest.mark.parametrize("shape,grid", [((3, 1, 4, 5), (4, 5)), ((1, 1, 4, 5), (4, 5)), ((3, 1, 4, 1), (4, 5)),
                                        ((4, 5), (4, 5)), ((1, 4, 5), (4, 5)), ((3, 1, 6, 1, 1), (6, 4, 5)),
                                        ((3, 1, 6, 4, 5), (6, 4, 5)), ((1, 1, 1, 4, 5), (6, 4, 5))])
def test_sigma_classifier_maps(shape, grid):
    from cdlnet_video_amd.net import _noise_scale, _is_map
    N = 3
    sigma = 10.0 + 30.0 * torch.rand(shape)
    c = _noise_scale(sigma, True, N, "cpu", grid)
    assert _is_map(c) and c.shape == (N, 1) + grid and c.is_contiguous()
    lead = (1,) * (2 + len(grid) - len(shape)) + tuple(shape)
    assert torch.equal(c, (sigma / 255.0).reshape(lead).expand((N, 1) + grid))
    # differentiable back to the shape sigma was given in (expand's adjoint is the sum)
    s2 = sigma.clone().requires_grad_(True)
    _noise_scale(s2, True, N, "cpu", grid).sum().backward()
    assert s2.grad.shape == sigma.shape


def test_sigma_classifier_refusals():
    from cdlnet_video_amd.net import _noise_scale, _code_grid
    with pytest.raises(ValueError, match="channel"):
        _noise_scale(torch.rand(3, 8, 4, 5), True, 3, "cpu", (4, 5))
    with pytest.raises(ValueError, match=r"\(3, 1, 4, 5\)"):                        # names the code grid it expected
        _noise_scale(torch.rand(3, 1, 8, 10), True, 3, "cpu", (4, 5))
    with pytest.raises(ValueError, match=r"\(3, 1, 4, 5\)"):
        _noise_scale(torch.rand(2, 1, 4, 5), True, 3, "cpu", (4, 5))
    with pytest.raises(ValueError):
        _noise_scale(torch.rand(3, 1, 2, 4, 5), True, 3, "cpu", (4, 5))
    assert _code_grid((23, 21), 2) == (12, 11) and _code_grid((7, 13, 11), 2) == (4, 7, 6) and _code_grid((9, 8), 1) == (9, 8)


@pytest.mark.parametrize("shape,s", [((2, 1, 23, 21), 2), ((2, 1, 24, 20), 2), ((1, 1, 7, 13, 11), 2), ((2, 1, 10, 11), 3),
                                     ((2, 1, 9, 8), 1)])
def test_sigma_to_code_grid(shape, s):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd.net import _code_grid
    m = 10.0 + 30.0 * torch.rand(shape, generator=torch.Generator().manual_seed(3))
    got = cva.utils.sigma_to_code_grid(m, s)
    assert got.shape == (shape[0], 1) + _code_grid(shape[2:], s)
    if s == 1:
        assert torch.equal(got, m)
        return
    pool = F.avg_pool2d if len(shape) == 4 else F.avg_pool3d
    ref = pool(F.pad(m, O.stride_pads(shape[2:], s), mode="reflect"), s)
    assert rel_err(got, ref) < 1e-6
    with pytest.raises(ValueError):
        cva.utils.sigma_to_code_grid(torch.rand(2, 3, 8, 8), 2)


# ------------------------------------------------------------------------------------------ the C ABI
MAP_ARGS = {  # entry point: arguments it gained (pointers, in front of the stream)
    "cdl_analysis": ("cmap", "tslope"), "cdl_analysis_rev": ("cmap",),
    "cdl_tau_grad": ("cmap",), "cdl_tau_grad_gate": ("cmap",), "cdl_ista_forward": ("cmap", "tslope"),
    "cdl_ista_backward": ("cmap", "tslope", "dcmap"),
}
PARENT_ARGC = {"cdl_analysis": 11, "cdl_analysis_rev": 14, "cdl_tau_grad": 9,
               "cdl_tau_grad_gate": 9, "cdl_ista_forward": 18, "cdl_ista_backward": 32}


def test_map_is_a_nullable_argument_of_the_existing_entry_points():
    import ctypes
    from cdlnet_video_amd import _lib
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    for name, args in MAP_ARGS.items():
        sig = _lib.SIGNATURES[name]
        assert len(sig) == PARENT_ARGC[name] + len(args), name
        assert all(a is ctypes.c_void_p for a in sig[-1 - len(args):]), name       # the new pointers, then the stream
        decl = re.sub(r"/\*.*?\*/", "", re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1))   # no comments
        assert len(decl.split(",")) == len(sig), name
        for a in args:
            assert re.search(rf"\*{a}\b", decl), (name, a)
    # one new entry point, for the channel reduction behind dL/dsigma
    assert "cdl_sigma_grad" in _lib.SIGNATURES and re.search(r"\bint cdl_sigma_grad\(", header)
    # no suffixed sibling, in the bindings or in the header
    for base in MAP_ARGS:
        for suffix in ("_map", "_cmap", "_smap", "_sigma", "_ws"):
            name = base + suffix
            assert name not in _lib.SIGNATURES and name not in _lib.SIZE_T_FUNCS, name
            assert not re.search(rf"\b{name}\b", header), name


def test_ops_gain_trailing_keyword_arguments_only():
    import inspect
    from cdlnet_video_amd import ops
    for fn, kws in ((ops.analysis, ("cmap", "tslope")), (ops.analysis_rev, ("cmap",)), (ops.tau_grad, ("cmap",)),
                    (ops.ista_forward, ("cmap", "tslope")), (ops.ista_backward, ("cmap", "tslope", "dcmap"))):
        params = inspect.signature(fn).parameters
        for kw in kws:
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None, (fn.__name__, kw)
