"""CPU: the CSR tangent under a noise-level map -- the float64 restatement (tests/csr_tangent_restate.py,
which takes a map as it stands: its thresholds are the reference's broadcast) against the reference's own forward-mode
derivatives (fixtures c6m / c7m, tools/make_golden_csr_tangent_map.py), the C ABI and `ops` signatures the map arguments
were added to, the argument checks of `csr_jvp_step`, and the `noise=` rules of the SURE forms."""
import inspect
import os
import re

import pytest
import torch

import cdlnet_video_amd as cva
import csr_tangent_restate as R
from cdlnet_video_amd import _lib, ops, temporal, train
from conftest import ROOT, load_golden, rel_err

FIXTURES = [("c6m_csr_jvp_chain_map", "csr", 2), ("c7m_csrf2_jvp_chain_map", "f2", 3)]


# ---------------------------------------------------------------------------------- the clip chains under a map
@pytest.mark.parametrize("name,variant,D", FIXTURES)
def test_restated_chain_equals_the_reference_jvp_under_a_map(name, variant, D):
    """Stride 2 on an odd frame, one code-grid map per frame (another one for every sample), the SURE loss weighted at image
    resolution: outputs, loss and every gradient to 2e-6, as for c6 / c7."""
    g = load_golden(name)
    K, M, P, s, C = g["hyper"]
    assert s == 2 and any(d % 2 for d in g["y0"].shape[2:])
    work = {k: v.double() for k, v in g["sd"].items()}
    leaves = {k: v.requires_grad_(True) for k, v in work.items()}
    ys, bs = [g[f"y{t}"].double() for t in range(D)], [g[f"b{t}"].double() for t in range(D)]
    sigmas, noise = [g[f"sigma{t}"].double() for t in range(D)], [g[f"noise{t}"].double() for t in range(D)]
    for t in range(D):
        assert tuple(noise[t].shape) == (ys[t].shape[0], 1) + tuple(ys[t].shape[2:])
        assert torch.equal(cva.utils.sigma_to_code_grid(g[f"noise{t}"], s), g[f"sigma{t}"])
        assert tuple(sigmas[t].shape[2:]) == tuple(-(-d // s) for d in ys[t].shape[2:])
    outs = R.chain(work, variant, ys, bs, sigmas, K=K, P=P, s=s)
    for t in range(D):
        assert rel_err(outs[t][0].float(), g[f"xhat{t}"]) < 2e-6, f"{name} xhat{t}"
        assert rel_err(outs[t][1].float(), g[f"xdot{t}"]) < 2e-6, f"{name} xdot{t}"
    loss = R.sure(outs, ys, bs, noise)                                   # the divergence weight at image resolution
    assert abs(float(loss.detach()) - g["loss"]) < 2e-6 * max(1.0, abs(g["loss"]))
    loss.backward()
    assert g["gate_margin"] > 0
    seen = 0
    for k, ref in g["grad"].items():
        assert rel_err(leaves[k].grad.float(), ref) < 2e-6, f"{name} grad {k}"
        seen += 1
    assert seen >= 2 * K + 2


def test_fixtures_are_no_larger_than_their_per_sample_twins():
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz"))
    assert size("c6m_csr_jvp_chain_map") <= size("c6_csr_jvp_chain")
    assert size("c7m_csrf2_jvp_chain_map") <= size("c7_csrf2_jvp_chain")


# ---------------------------------------------------------------------------------- signatures
def _header_params(name):
    text = open(os.path.join(ROOT, "include", "cdlnet_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in body.split(",")]


@pytest.mark.parametrize("name,before", [("cdl_prox_csr_tangent", "out"), ("cdl_analysis_prox_tangent", "workspace_floats"),
                                         ("cdl_csr_tangent_forward", "scratch_floats")])
def test_entry_points_gained_cmap_and_tslope_in_front_of_stream(name, before):
    params = _header_params(name)
    assert params[-4:] == [before, "cmap", "tslope", "stream"], params
    assert params.count("cmap") == 1 and params.count("tslope") == 1
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(params)
    assert sig[-3:] == [_lib._P, _lib._P, _lib._P]
    assert not [k for k in _lib.SIGNATURES if k.startswith(name + "_")], "no suffixed sibling entry points"


@pytest.mark.parametrize("fn", [ops.prox_csr_tangent, ops.analysis_prox_tangent, ops.csr_tangent_forward])
def test_ops_map_keywords_are_keyword_only_and_default_to_none(fn):
    ps = inspect.signature(fn).parameters
    for k in ("cmap", "tslope"):
        assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__name__, k)
    assert [k for k, p in ps.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["cmap", "tslope"]


def test_loop_twins_pass_the_map_on():
    from cdlnet_video_amd import loop
    for fn in (loop._tangent_csr, loop._tangent_csr_stepwise, loop._tangent_backward_csr):
        ps = inspect.signature(fn).parameters
        assert ps["cmap"].default is None and ps["tslope"].default is None, fn.__name__


# ---------------------------------------------------------------------------------- csr_jvp_step's refusals
def _net(cls, s=1):
    torch.manual_seed(0)
    return cls(K=2, M=4, P=3, s=s, C=1, t0=1e-2, adaptive=True, init=False)


@pytest.mark.parametrize("cls", [cva.CDLNet_CSR, cva.CDLNet_CSRf2])
def test_csr_jvp_step_refusals(cls):
    net = _net(cls)
    y = torch.rand(1, 1, 8, 8)
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        temporal.csr_jvp_step(net, y, torch.ones_like(y), sigma=25.0)
    with pytest.raises(RuntimeError, match="no CPU"):                 # a map is no reason to go elsewhere
        temporal.csr_jvp_step(net, y, torch.ones_like(y), sigma=torch.full((1, 1, 8, 8), 25.0))
    with pytest.raises(NotImplementedError, match="mask"):
        temporal.csr_jvp_step(net, y, torch.ones_like(y), sigma=25.0, mask=torch.ones_like(y).requires_grad_(True))
    with pytest.raises(TypeError):
        temporal.csr_jvp_step(net, y, 1.0, sigma=25.0)
    with pytest.raises(TypeError, match="CDLNet_CSR"):
        temporal.csr_jvp_step(cva.CDLNet(K=2, M=4, P=3, s=1, C=1, t0=1e-2, adaptive=True, init=False), y, y, sigma=25.0)
    if cls is cva.CDLNet_CSR:
        with pytest.raises(ValueError, match="no z_after"):
            temporal.csr_jvp_step(net, y, torch.ones_like(y), z_prev=z, z_after=z, sigma=25.0)
    # the nets themselves keep refusing a map (one contract per variant)
    with pytest.raises((RuntimeError, NotImplementedError)):
        net.jvp_recurrent(y, torch.ones_like(y), sigma=torch.full((1, 1, 8, 8), 25.0))


# ---------------------------------------------------------------------------------- the noise= rules
class _Stub(torch.nn.Module):
    """xhat = w y, xdot = w v: enough to read the SURE expressions back."""

    def __init__(self, s=1):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((), 0.5))
        self.s, self.sigmas = s, []

    def forward(self, y, sigma=None, mask=1):
        self.sigmas.append(sigma)
        return self.w * y, None

    def jvp(self, y, v, sigma=None, mask=1):
        self.sigmas.append(sigma)
        return self.w * y, self.w * v

    def jvp_recurrent(self, y, v, *rest):
        self.sigmas.append(rest[-1])
        return self.w * y, self.w * v, torch.zeros(1), torch.zeros(1)


@pytest.mark.parametrize("sigma", [25.0, torch.tensor([15.0, 30.0]).reshape(2, 1, 1, 1)])
def test_without_noise_the_sure_forms_keep_their_expression(sigma):
    net = _Stub()
    gen = torch.Generator().manual_seed(1)
    y, b = torch.rand(2, 1, 6, 5, generator=gen), torch.randn(2, 1, 6, 5, generator=gen)
    s2 = (sigma / 255.0) ** 2
    loss, xhat = train.sure_loss(net, y, sigma, b=b)
    assert torch.equal(loss, torch.mean((y - xhat) ** 2) + 2.0 * torch.mean(s2 * b * (net.w * b)))
    xh = net.w * y
    got = train.mcsure_loss(net, y, xh, sigma, b=b)
    want = torch.mean((y - xh) ** 2) + 2.0 * torch.mean(s2 * b * (net.w * (y.clone() + 1e-3 * b) - xh)) / 1e-3
    assert torch.equal(got, want)
    lc, _ = train.sure_loss_clip(net, [y, y], [sigma, sigma], b=[b, b])
    mse, div = torch.mean((y - xh) ** 2), 2.0 * torch.mean(s2 * b * (net.w * b))
    assert torch.equal(lc, 0.0 + mse + div + mse + div)
    fd = 2.0 * torch.mean(s2 * b * (net.w * (y.clone() + 1e-3 * b) - xh)) / 1e-3
    assert torch.equal(train.mcsure_loss_clip(_Clip(net), [y, y], [sigma, sigma], [xh, xh], b=[b, b]), 0.0 + mse + fd + mse + fd)


class _Clip:
    """clip_forward over the stub: mcsure_loss_clip's second chain."""

    def __init__(self, net):
        self.net = net

    def __call__(self, y, *rest):
        return self.net(y, rest[-1])


def test_noise_replaces_sigma_in_the_divergence_weight_and_a_code_grid_map_needs_it(monkeypatch):
    net = _Stub(s=2)
    gen = torch.Generator().manual_seed(2)
    y, b = torch.rand(2, 1, 13, 11, generator=gen), torch.randn(2, 1, 13, 11, generator=gen)
    noise = 10.0 + 30.0 * torch.rand(2, 1, 13, 11, generator=gen)
    sigma = cva.utils.sigma_to_code_grid(noise, 2)
    assert tuple(sigma.shape) == (2, 1, 7, 6)
    for call in (lambda **kw: train.sure_loss(net, y, sigma, b=b, **kw)[0],
                 lambda **kw: train.mcsure_loss(net, y, net.w * y, sigma, b=b, **kw)):
        with pytest.raises(ValueError, match="noise="):
            call()
        assert bool(torch.isfinite(call(noise=noise)))
    loss, xhat = train.sure_loss(net, y, sigma, b=b, noise=noise)
    assert torch.equal(loss, torch.mean((y - xhat) ** 2) + 2.0 * torch.mean((noise / 255.0) ** 2 * b * (net.w * b)))
    assert net.sigmas[-1] is sigma                                   # the net still takes the code-grid map

    # the steps: a level with spatial extent reaches the net on the code grid and the SURE form as noise=
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    net.sigmas.clear()
    loss, level = train.train_step(net, opt, y, noise, mcsure="exact", generator=torch.Generator().manual_seed(3))
    assert level is noise and torch.equal(net.sigmas[-1], sigma) and bool(torch.isfinite(loss))
    net.sigmas.clear()
    train.train_step(net, opt, y, 25, mcsure="exact", generator=torch.Generator().manual_seed(3))
    assert net.sigmas == [25]                                        # scalars go the way they went


# ---------------------------------------------------------------------------------- the restatement on prescribed pieces
@pytest.mark.parametrize("both", [False, True])
def test_the_call_restated_on_its_own_pieces_is_the_call(both):
    """tests/csr_tangent_map_restate.py (what the device tests compare with): on the pieces of a float64 run the restated
    call returns that run's (xhat, z), and its tangent is the central difference of the oracle's call -- stride 2, an odd
    frame, a map that differs per sample, a mask."""
    import csr_tangent_map_restate as RM
    from oracle import cdl_oracle as O
    gen = torch.Generator().manual_seed(11 + both)
    K, M, P, s, N = 2, 4, 5, 2, 2
    rnd = lambda *sh: torch.randn(sh, generator=gen, dtype=torch.float64)
    A, B = [0.3 * rnd(M, 1, P, P) for _ in range(K)], [0.3 * rnd(M, 1, P, P) for _ in range(K)]
    t, g1, g2 = (sc * torch.rand(K, 2, M, 1, 1, generator=gen, dtype=torch.float64) for sc in (1.5, 1.0, 1.0))
    t[0, 0, 0] = -0.3                                               # a negative threshold row
    y, v = rnd(N, 1, 13, 11), rnd(N, 1, 13, 11)
    mask = (torch.rand(N, 1, 13, 11, generator=gen) > 0.3).double()
    code = lambda: 0.3 * rnd(N, M, 7, 6) * (torch.rand(N, M, 7, 6, generator=gen) > 0.4)
    zp, za = code(), (code() if both else None)
    # (tangents on the neighbours' supports: off them sign(z) jumps under a finite step, which autograd does not see)
    zdp, zda = rnd(N, M, 7, 6) * (zp != 0), (rnd(N, M, 7, 6) * (za != 0) if both else None)
    c = (10.0 + 30.0 * torch.rand(N, 1, 7, 6, generator=gen, dtype=torch.float64)) / 255.0
    kw = dict(s=s, P=P, mask=mask)
    pcs, xhat, z = RM.run_pieces(A, B, t, g1, g2 if both else None, y, zp, za, c, **kw)
    for pc in pcs:
        assert all(0.02 < float(G.float().mean()) < 0.98 for G in pc["G"]), [float(G.float().mean()) for G in pc["G"]]
    got = RM.call_at(pcs, A, B, t, g1, g2 if both else None, y, v, zp, zdp, za, zda, c, **kw)
    assert rel_err(got[0], xhat) < 1e-12 and rel_err(got[2], z) < 1e-12
    sd = {f"A.{k}.weight": A[k] for k in range(K)}
    sd.update({f"B.{k}.weight": B[k] for k in range(K)})
    sd.update(t=t, g1=g1, g2=g2)
    h = 1e-7
    run = lambda e: O.ista_csr(sd, y + e * v, zp + e * zdp, za + e * zda if both else None, K=K, P=P, s=s, sigma=255.0 * c,
                               adaptive=True, mask=mask, variant="f2")
    (xu, zu), (xd, zd) = run(h), run(-h)
    assert rel_err(got[1], (xu - xd) / (2 * h)) < 1e-6 and rel_err(got[3], (zu - zd) / (2 * h)) < 1e-6


def test_fit_hands_a_level_map_through_unwrapped_in_every_phase(tmp_path):
    """fit(noise_std=<tensor>): no (lo, hi) range is made of it and no level is drawn; train, val and test give the net the
    map on its code grid (the SURE form the image-resolution one)."""
    net = _Stub(s=2)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    gen = torch.Generator().manual_seed(4)
    batches = [torch.rand(2, 1, 13, 11, generator=gen) for _ in range(2)]
    noise = 10.0 + 30.0 * torch.rand(2, 1, 13, 11, generator=gen)
    sigma = cva.utils.sigma_to_code_grid(noise, 2)
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    hist = cva.fit(net, opt, {"train": batches, "val": batches[:1], "test": batches[:1]}, epochs=1, save_dir=str(tmp_path),
                   noise_std=noise, verbose=False, log=lambda *_: None, generator=g1, mcsure="exact")
    assert [h[1] for h in hist] == ["train", "val", "test"]
    assert len(net.sigmas) == 4 and all(torch.equal(s_, sigma) for s_ in net.sigmas)
    for _ in range(2):                                              # train: awgn's randn, then sure_loss's b; nothing else
        torch.randn(2, 1, 13, 11, generator=g2), torch.randn(2, 1, 13, 11, generator=g2)
    for _ in range(2):                                              # val, test: awgn's randn
        torch.randn(2, 1, 13, 11, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
