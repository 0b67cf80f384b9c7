"""CPU: the float64 restatement of the CSR tangent (tests/csr_tangent_restate.py) against the reference's own forward-mode
derivatives (fixtures c5..c7, tools/make_golden_csr_tangent.py), the argument checks of jvp_recurrent, and the call
sequences of the clip steps (train_step_clip / sure_loss_clip) on a counting stub net."""
import pytest
import torch

import cdlnet_video_amd as cva
import csr_tangent_restate as R
from cdlnet_video_amd import train
from conftest import load_golden, rel_err


# ---------------------------------------------------------------------------------- the two maps
def test_gates_and_select_equal_the_reference_jvp_pointwise():
    """c5: exact zeros, ties, negative thresholds; with and without neighbour tangents."""
    g = load_golden("c5_csr_tangent_pointwise")
    u, zp, za = g["u"], g["zp"], g["za"]
    ud, zpd, zad = (g[k].double() for k in ("ud", "zpd", "zad"))
    T = torch.tensor
    for i, (lam, g1, g2) in enumerate(g["cases"].reshape(-1, 3).tolist()):
        G1 = R.gates(u, zp, None, T(lam), T(g1))
        G2 = R.gates(u, zp, za, T(lam), T(g1), T(g2))
        for name, got in (("jvp_csr", R.prox_tangent(G1, ud, zpd)), ("jvp_csr_u", R.prox_tangent(G1, ud)),
                          ("jvp_csr_f2", R.prox_tangent(G2, ud, zpd, zad)), ("jvp_csr_f2_u", R.prox_tangent(G2, ud))):
            ref = g[name][i]
            err = float((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            assert err <= 1e-6, f"{name} case {i}: {err:.2e}"
        assert 0 < float(G2[2].float().mean()) < 1, "a case whose outer gate is constant checks nothing"


# ---------------------------------------------------------------------------------- the clip chains
def _leaves(sd):
    work = {k: v.double() for k, v in sd.items()}
    leaves = {k: v.requires_grad_(True) for k, v in work.items()}
    return work, leaves


@pytest.mark.parametrize("name,variant,D", [("c6_csr_jvp_chain", "csr", 2), ("c7_csrf2_jvp_chain", "f2", 3)])
def test_restated_chain_equals_the_reference_jvp(name, variant, D):
    g = load_golden(name)
    K, M, P, s, C = g["hyper"]
    work, leaves = _leaves(g["sd"])
    sig = g["sigma"].double() if torch.is_tensor(g["sigma"]) else g["sigma"]
    ys, bs = [g[f"y{t}"].double() for t in range(D)], [g[f"b{t}"].double() for t in range(D)]
    outs = R.chain(work, variant, ys, bs, [sig] * D, K=K, P=P, s=s)
    for t in range(D):
        assert rel_err(outs[t][0].float(), g[f"xhat{t}"]) < 2e-6, f"{name} xhat{t}"
        assert rel_err(outs[t][1].float(), g[f"xdot{t}"]) < 2e-6, f"{name} xdot{t}"
    loss = R.sure(outs, ys, bs, [sig] * D)
    assert abs(float(loss.detach()) - g["loss"]) < 2e-6 * max(1.0, abs(g["loss"]))
    loss.backward()
    assert g["gate_margin"] > 0
    seen = 0
    for k, ref in g["grad"].items():
        assert rel_err(leaves[k].grad.float(), ref) < 2e-6, f"{name} grad {k}"
        seen += 1
    assert seen >= 2 * K + 2


def test_thresholds_get_no_gradient_through_the_tangent():
    """The gates are piecewise constant: a loss on (xdot, zdot) alone has zero threshold gradients."""
    g = load_golden("c6_csr_jvp_chain")
    K, M, P, s, C = g["hyper"]
    work, leaves = _leaves(g["sd"])
    ys, bs = [g[f"y{t}"].double() for t in range(2)], [g[f"b{t}"].double() for t in range(2)]
    outs = R.chain(work, "csr", ys, bs, [g["sigma"].double()] * 2, K=K, P=P, s=s)
    sum(torch.mean(b * xd) for b, (_, xd) in zip(bs, outs.values())).backward()
    for k in ("t", "t2", "g"):
        assert leaves[k].grad is None or float(leaves[k].grad.abs().max()) == 0.0, k
    assert float(leaves["A.1.weight"].grad.abs().max()) > 0


# ---------------------------------------------------------------------------------- argument checks
def _net(cls):
    torch.manual_seed(0)
    return cls(K=2, M=4, P=3, s=1, C=1, t0=1e-2, adaptive=True, init=False)


@pytest.mark.parametrize("cls", [cva.CDLNet_CSR, cva.CDLNet_CSRf2])
def test_jvp_recurrent_refusals(cls):
    net = _net(cls)
    y = torch.rand(1, 1, 8, 8)
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):                 # as forward does
        net.jvp_recurrent(y, torch.ones_like(y), sigma=25.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        net(y, sigma=25.0)
    with pytest.raises(ValueError, match="zdot_prev given without z_prev"):
        net.jvp_recurrent(y, torch.ones_like(y), None, z, sigma=25.0)
    with pytest.raises(TypeError):
        net.jvp_recurrent(y, 1.0, sigma=25.0)
    with pytest.raises(NotImplementedError, match="CSR"):             # jvp keeps refusing, and names the new method
        net.jvp(y, torch.ones_like(y), 25.0)
    with pytest.raises(NotImplementedError, match="jvp_recurrent"):
        net.jvp(y, torch.ones_like(y), 25.0)
    if cls is cva.CDLNet_CSRf2:
        with pytest.raises(ValueError, match="zdot_after given without z_after"):
            net.jvp_recurrent(y, torch.ones_like(y), zdot_after=z, sigma=25.0)


# ---------------------------------------------------------------------------------- clip steps on a counting stub
class _Stub(torch.nn.Module):
    """Records every call; outputs are tagged by the call's number so that what feeds what can be read back."""

    def __init__(self, f2):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.f2, self.calls = f2, []

    def _frame(self, y):
        return int(round(float(y.detach().reshape(-1)[0]) // 10))

    def _tag(self, z):
        return None if z is None else int(z.detach().reshape(-1)[0])

    def _out(self, y):
        n = len(self.calls)
        return self.w * y, torch.full((1,), float(n))

    def forward(self, y, z_prev=None, *rest):
        z_after, sigma = (rest[0], rest[1]) if self.f2 else (None, rest[0])
        self.calls.append(("fwd", self._frame(y), self._tag(z_prev), self._tag(z_after), float(sigma)))
        return self._out(y)

    def jvp_recurrent(self, y, v, z_prev=None, zdot_prev=None, *rest):
        z_after, zdot_after, sigma = (rest[0], rest[1], rest[2]) if self.f2 else (None, None, rest[0])
        for z, zd in ((z_prev, zdot_prev), (z_after, zdot_after)):
            assert (z is None) == (zd is None) and self._tag(z) == self._tag(zd), "a code travels with its own tangent"
        self.calls.append(("jvp", self._frame(y), self._tag(z_prev), self._tag(z_after), float(sigma), v))
        xhat, z = self._out(y)
        return xhat, self.w * v, z, z.clone()


def _frames(D):
    """Clean frames whose first element encodes the frame index (10 t + 5) -- the stub reads it back."""
    return torch.stack([torch.full((1, 1, 4, 4), 10.0 * t + 5.0) for t in range(D)], dim=2)


CSR_ORDER = [(0, None, None), (1, 1, None), (0, 2, None), (1, 3, None)]
F2_ORDER = [(0, None, None), (1, 1, None), (2, 1, None), (1, 1, 3), (0, None, 3)]


@pytest.mark.parametrize("f2,order", [(False, CSR_ORDER), (True, F2_ORDER)])
def test_supervised_clip_step_follows_the_reference_sequence(f2, order, monkeypatch):
    D = 3 if f2 else 2
    net = _Stub(f2)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    draws = []

    def awgn(x, noise_std, generator=None):
        draws.append(int(round(float(x.reshape(-1)[0]) // 10)))
        return x.clone(), float(20 + len(draws))

    monkeypatch.setattr(train, "awgn", awgn)
    loss, sigmas, mse = train.train_step_clip(net, opt, _frames(D), (20, 30))
    assert draws == list(range(D)), "one noise draw per frame, in frame order, before any call"
    assert sigmas == [21.0, 22.0, 23.0][:D]
    assert [c[:4] for c in net.calls] == [("fwd",) + o for o in order]
    assert [c[4] for c in net.calls] == [sigmas[o[0]] for o in order], "each call gets its own frame's sigma"
    assert float(mse) == pytest.approx(float(loss) / D) and float(loss) == 0.0
    assert net.w.grad is not None


@pytest.mark.parametrize("f2,order", [(False, CSR_ORDER), (True, F2_ORDER)])
def test_exact_sure_clip_loss_runs_the_same_chain_with_one_direction_per_frame(f2, order):
    D = 3 if f2 else 2
    net = _Stub(f2)
    frames = [_frames(D)[:, :, t] for t in range(D)]
    gen = torch.Generator().manual_seed(3)
    loss, xhats = train.sure_loss_clip(net, frames, [25.0] * D, generator=gen)
    assert [c[:4] for c in net.calls] == [("jvp",) + o for o in order]
    ref = torch.Generator().manual_seed(3)
    b = [torch.randn(frames[0].shape, generator=ref) for _ in range(D)]          # drawn as sure_loss draws b, frame order
    for c in net.calls:
        assert torch.equal(c[5], b[c[1]]), "the same b_t at every call on frame t"
    want = sum(torch.mean((y - y) ** 2) + 2.0 * torch.mean((25.0 / 255.0) ** 2 * bt * bt) for y, bt in zip(frames, b))
    assert float(loss) == pytest.approx(float(want), rel=1e-6)
    assert len(xhats) == D


def test_finite_difference_clip_step_runs_a_second_chain_at_the_perturbed_frames(monkeypatch):
    net = _Stub(False)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    monkeypatch.setattr(train, "awgn", lambda x, noise_std, generator=None: (x.clone(), 25.0))
    gen = torch.Generator().manual_seed(8)
    loss, _, _ = train.train_step_clip(net, opt, _frames(2), 25, generator=gen, mcsure=True)
    assert [c[:4] for c in net.calls] == [("fwd",) + o for o in CSR_ORDER] + [("fwd", o[0], o[1] + 4 if o[1] else None, None)
                                                                             for o in CSR_ORDER]
    ref = torch.Generator().manual_seed(8)
    b = [torch.randn(1, 1, 4, 4, generator=ref) for _ in range(2)]
    # the stub is the identity: (xhat_b - xhat) / h = b, so the divergence term is 2 mean(s2 b b) per frame
    want = sum(2.0 * torch.mean((25.0 / 255.0) ** 2 * bt * bt) for bt in b)
    assert float(loss) == pytest.approx(float(want), rel=1e-3)


def test_clip_steps_check_their_arguments():
    net = _Stub(False)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    with pytest.raises(ValueError, match="mcsure"):
        train.train_step_clip(net, opt, _frames(2), 25, mcsure="fd")
    with pytest.raises(ValueError, match="2 frames"):
        train.train_step_clip(net, opt, _frames(4), 25)
    with pytest.raises(ValueError, match="trains on clips of 2"):
        train.train_step_clip(_net(cva.CDLNet_CSR), opt, _frames(3), 25)
    with pytest.raises(ValueError, match=r"\(B, C, D, H, W\)"):
        train.train_step_clip(net, opt, _frames(2)[:, :, 0], 25)
