"""CPU: what net.jvp / sure_loss / train_step(mcsure="exact") promise that needs no device -- the refusals, the SURE
formula, which objective each `mcsure` value reaches, and the C entry points of the tangent sweeps."""
import pytest
import torch
import torch.nn as nn

import cdlnet_video_amd as cva
from cdlnet_video_amd import train as T


class Scale(nn.Module):
    """xhat = w * y, so J v = w * v: a CPU stand-in with the jvp contract of the HIP nets."""

    def __init__(self, w=0.7):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(float(w)))
        self.forwards, self.jvps = 0, 0

    def forward(self, y, sigma=None, mask=1):
        self.forwards += 1
        return self.w * y, None

    def jvp(self, y, v, sigma=None, mask=1):
        self.jvps += 1
        return self.w * y, self.w * v


def _net(cls=None, **kw):
    cls = cls or cva.CDLNet
    return cls(K=2, M=4, P=3, s=1, C=1, t0=1e-2, adaptive=True, init=False, **kw)


@pytest.mark.parametrize("cls", [cva.CDLNet_CSR, cva.CDLNet_CSRf2])
def test_csr_nets_refuse_jvp(cls):
    y = torch.rand(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="CSR"):
        _net(cls).jvp(y, torch.ones_like(y), 25.0)


def test_residual_video_net_refuses_jvp():
    y = torch.rand(1, 1, 4, 8, 8)
    net = cva.CDLNetVideo(K=2, M=4, P=[3, 3, 3], s=1, C=1, t0=1e-2, adaptive=True, init=False, residual=True)
    with pytest.raises(NotImplementedError, match="residual"):
        net.jvp(y, torch.ones_like(y), 25.0)


@pytest.mark.parametrize("cls", [cva.CDLNet, cva.GDLNet, cva.CDLNetVideo])
def test_jvp_on_a_cpu_tensor_raises_as_forward_does(cls):
    shape = (1, 1, 4, 8, 8) if cls is cva.CDLNetVideo else (1, 1, 8, 8)
    net = _net(cls)
    y = torch.rand(shape)
    with pytest.raises(RuntimeError, match="no CPU"):
        net.jvp(y, torch.ones_like(y), 25.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        net(y, 25.0)


def test_sure_loss_formula_and_probe_draw():
    net = Scale(0.7)
    g = torch.Generator().manual_seed(3)
    y = torch.rand(2, 1, 6, 6, generator=g)
    sigma = torch.tensor([20.0, 30.0]).reshape(2, 1, 1, 1)
    b = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    loss, xhat = cva.sure_loss(net, y, sigma, b=b)
    want = torch.mean((y - 0.7 * y) ** 2) + 2.0 * torch.mean((sigma / 255) ** 2 * b * (0.7 * b))
    assert abs(loss.item() - want.item()) < 1e-7 and torch.equal(xhat, 0.7 * y)
    loss.backward()
    assert net.w.grad is not None
    # the probe is drawn exactly as mcsure_loss draws it: same generator state -> same b -> h -> 0 limit of the same value
    l1, _ = cva.sure_loss(net, y, sigma, generator=torch.Generator().manual_seed(5))
    assert l1.item() == loss.item()
    fd = cva.mcsure_loss(net, y, net(y, sigma)[0], sigma, generator=torch.Generator().manual_seed(5))
    assert abs(fd.item() - loss.item()) < 1e-4          # a linear net: the finite difference is exact up to rounding / h


@pytest.mark.parametrize("mcsure,reaches", [("exact", "sure"), (True, "mcsure"), (False, "mse"), (1, "mcsure"), (0, "mse"),
                                            (None, "mse")])    # non-strings keep their truthiness
def test_train_step_routes_the_mcsure_switch(monkeypatch, mcsure, reaches):
    calls = []
    real_sure, real_mc = T.sure_loss, T.mcsure_loss
    monkeypatch.setattr(T, "sure_loss", lambda *a, **k: (calls.append("sure"), real_sure(*a, **k))[1])
    monkeypatch.setattr(T, "mcsure_loss", lambda *a, **k: (calls.append("mcsure"), real_mc(*a, **k))[1])
    net = Scale(0.5)
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    batch = torch.rand(2, 1, 6, 6, generator=torch.Generator().manual_seed(1))
    loss, sigma = T.train_step(net, opt, batch, (20, 30), generator=torch.Generator().manual_seed(2), mcsure=mcsure)
    assert calls == ([] if reaches == "mse" else [reaches])
    assert (net.jvps, net.forwards) == {"sure": (1, 0), "mcsure": (0, 2), "mse": (0, 1)}[reaches]
    assert torch.isfinite(loss) and float(net.w.detach()) != 0.5


def test_train_step_rejects_an_unknown_mcsure_value():
    net = Scale()
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    with pytest.raises(ValueError, match="mcsure"):
        T.train_step(net, opt, torch.rand(1, 1, 4, 4), 25, mcsure="exakt")


def test_fit_passes_exact_through(tmp_path):
    net = Scale(0.5)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(0)
    data = {"train": [torch.rand(2, 1, 8, 8, generator=g) for _ in range(2)]}
    T.fit(net, opt, data, epochs=1, save_dir=str(tmp_path), noise_std=25, verbose=False, mcsure="exact",
          log=lambda *_: None)
    assert net.jvps == 2 and net.forwards == 0


def test_tangent_entry_points_are_exported_and_bound():
    lib = cva._lib.lib()
    for name in ("cdl_tangent_forward", "cdl_tangent_backward", "cdl_fused2d_tangent", "cdl_fusedg_tangent"):
        assert hasattr(lib, name) and name in cva._lib.SIGNATURES
    assert cva.sure_loss is T.sure_loss and "sure_loss" in cva.__all__
