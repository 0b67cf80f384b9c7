"""The perceptual term without a GPU: the float64 restatement on its own, the VGG16 weight loading, the shape refusals
of CombinedLossWithSSIM, the trainer's new keywords and the host-side refusals of the cdl_vgg_* entry points."""
import ctypes
import inspect
import os

import pytest
import torch

import cdlnet_video_amd as cva
import perceptual_restate as R

_FAKE = ctypes.c_void_p(256)        # never dereferenced: every call below is refused on its host-side arguments


def _small_weights(seed=0):
    return R.random_weights(seed)


def test_conv1_summed_equals_three_channel_repeat():
    sd = _small_weights(1)
    x = torch.rand((3, 1, 20, 23), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    a = R.features(x, sd, sum_conv1=True)
    b = R.features(x, sd, sum_conv1=False)
    assert a.shape == (3, 256, 5, 5)
    assert torch.allclose(a, b, rtol=0, atol=1e-12 * b.abs().max())


def test_per_frame_loop_equals_single_mean():
    sd = _small_weights(3)
    g = torch.Generator().manual_seed(4)
    o = torch.rand((2, 1, 3, 17, 21), generator=g, dtype=torch.float64)
    t = torch.rand((2, 1, 3, 17, 21), generator=g, dtype=torch.float64)
    a = R.perceptual(o, t, sd, per_frame=True, sum_conv1=False)
    b = R.perceptual(o, t, sd)
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))


def test_restatement_gradcheck():
    sd = {k: v.double() * 0.5 for k, v in _small_weights(5).items()}
    g = torch.Generator().manual_seed(6)
    o = torch.rand((1, 1, 1, 8, 9), generator=g, dtype=torch.float64).requires_grad_()
    t = torch.rand((1, 1, 1, 8, 9), generator=g, dtype=torch.float64).requires_grad_()
    trace = []
    R.features(o.detach().reshape(1, 1, 8, 9), sd, trace=trace)
    pre = [tr for tr in trace if tr.dtype == torch.float64]
    codes = [tr for tr in trace if tr.dtype == torch.uint8]
    trace_t = []
    R.features(t.detach().reshape(1, 1, 8, 9), sd, trace=trace_t)
    pre_t = [tr for tr in trace_t if tr.dtype == torch.float64]
    codes_t = [tr for tr in trace_t if tr.dtype == torch.uint8]
    gates = [(p > 0).double() for p in pre]
    gates_t = [(p > 0).double() for p in pre_t]

    def f(a, b):                    # fixed gates and argmaxes: a smooth (quadratic) function of the two images
        fa = R.features(a.reshape(1, 1, 8, 9), sd, gates=gates, codes=[c.long() for c in codes])
        fb = R.features(b.reshape(1, 1, 8, 9), sd, gates=gates_t, codes=[c.long() for c in codes_t])
        return torch.mean((fa - fb) ** 2)

    assert torch.autograd.gradcheck(f, (o, t), eps=1e-6, atol=1e-8, rtol=1e-5)
    # the prescribed gates reproduce the free evaluation
    with torch.no_grad():
        assert float(f(o, t)) == pytest.approx(float(R.perceptual(o, t, sd)), rel=1e-12)


def _layouts(sd):
    tv = {f"features.{k}": v for k, v in sd.items()}
    tv["features.16.weight"] = torch.zeros(512, 256, 3, 3)     # deeper layers and the classifier are ignored
    tv["classifier.0.weight"] = torch.zeros(4, 4)
    tv["classifier.0.bias"] = torch.zeros(4)
    return {"torchvision": tv, "reference": {f"vgg.{k}": v for k, v in sd.items()}, "bare": dict(sd)}


@pytest.mark.parametrize("layout", ["torchvision", "reference", "bare"])
def test_weight_layouts(layout, tmp_path):
    sd = _small_weights(7)
    src = _layouts(sd)[layout]
    for given in (src, str(tmp_path / "w.pth")):
        if isinstance(given, str):
            torch.save(src, given)
        got = cva.load_vgg16_weights(given)
        assert list(got) == [f"{i}.{n}" for i in R.CONVS for n in ("weight", "bias")]
        for k, v in sd.items():
            assert torch.equal(got[k], v)


def test_missing_and_malformed_weights(tmp_path, monkeypatch):
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        cva.load_vgg16_weights(str(tmp_path / "absent.pth"))
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        cva.CombinedLossWithSSIM()
    sd = _small_weights(8)
    del sd["14.bias"]
    with pytest.raises(KeyError):
        cva.load_vgg16_weights(sd)
    sd = _small_weights(8)
    sd["5.weight"] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(ValueError):
        cva.load_vgg16_weights(sd)


def test_default_path_and_state_dict_keys(tmp_path, monkeypatch):
    sd = _small_weights(9)
    os.makedirs(tmp_path / "hub" / "checkpoints")
    torch.save({f"features.{k}": v for k, v in sd.items()}, tmp_path / "hub" / "checkpoints" / "vgg16-397923af.pth")
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    loss = cva.CombinedLossWithSSIM()
    assert (loss.alpha, loss.beta, loss.gamma) == (1.0, 0.01, 0.1)
    keys = list(loss.state_dict())
    assert keys == [f"vgg.{i}.{n}" for i in R.CONVS for n in ("weight", "bias")]
    assert torch.equal(loss.state_dict()["vgg.12.weight"], sd["12.weight"])
    assert all(not p.requires_grad for p in loss.state_dict().values()) and not list(loss.parameters())


def test_beta_zero_needs_no_weights(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "nowhere"))
    loss = cva.CombinedLossWithSSIM(alpha=1.0, beta=0.0, gamma=0.1)
    assert loss.state_dict() == {} or len(loss.state_dict()) == 0


@pytest.mark.parametrize("shape,what", [((1, 3, 2, 32, 32), "one-channel"), ((1, 1, 32, 32), "expects"),
                                        ((1, 1, 2, 10, 32), "win_size"), ((1, 1, 2, 32, 10), "win_size")])
def test_shape_refusals(shape, what):
    loss = cva.CombinedLossWithSSIM(vgg_weights=_small_weights(10))
    x = torch.zeros(shape)
    with pytest.raises(ValueError, match=what):
        loss(x, x)
    if len(shape) == 5 and shape[1] == 3:
        with pytest.raises(ValueError, match="one-channel"):
            cva.metrics.perceptual_frames(x, x, _small_weights(10))


def test_trainer_keywords():
    ts = inspect.signature(cva.train_step).parameters
    assert ts["loss_fn"].default is None and ts["mcsure"].default is False
    fs = inspect.signature(cva.fit).parameters
    assert fs["combmse"].default is False and fs["loss_fn"].default is None
    from cdlnet_video_amd import CombinedLossWithSSIM
    assert CombinedLossWithSSIM is cva.loss.CombinedLossWithSSIM


def _ptrs(n=7):
    return (ctypes.c_void_p * n)(*([256] * n))


def test_vgg_abi_refusals():
    lib = cva._lib.lib()
    E = cva._lib.CDL_EINVAL
    n = int(lib.cdl_vgg_scratch_floats(2, 32, 32, 3))
    assert n > int(lib.cdl_vgg_scratch_floats(2, 32, 32, 1)) >= int(lib.cdl_vgg_scratch_floats(2, 32, 32, 0)) > 0
    assert lib.cdl_vgg_scratch_floats(2, 3, 32, 0) == 0 and lib.cdl_vgg_scratch_floats(2, 32, 3, 0) == 0
    assert lib.cdl_vgg_scratch_floats(0, 32, 32, 0) == 0 and lib.cdl_vgg_scratch_floats(1, 32, 32, 4) == 0
    w, b = _ptrs(), _ptrs()
    fwd = lambda *a: lib.cdl_vgg_forward(*a)                                   # noqa: E731
    # each call below is refused before any launch
    assert fwd(_FAKE, None, 2, 32, 32, w, b, 3, None, _FAKE, _FAKE, n, None) == E            # no target
    assert fwd(_FAKE, _FAKE, 2, 32, 32, None, b, 3, None, _FAKE, _FAKE, n, None) == E        # no weight table
    wn = (ctypes.c_void_p * 7)(*([256] * 6 + [0]))
    assert fwd(_FAKE, _FAKE, 2, 32, 32, wn, b, 3, None, _FAKE, _FAKE, n, None) == E          # a null weight
    assert fwd(_FAKE, _FAKE, 2, 32, 32, w, b, 3, None, None, _FAKE, n, None) == E            # no loss output
    assert fwd(None, _FAKE, 2, 32, 32, w, b, 0, None, None, _FAKE, n, None) == E             # no x and no feat
    assert fwd(None, _FAKE, 2, 32, 32, w, b, 1, _FAKE, None, _FAKE, n, None) == E            # grads without x
    assert fwd(_FAKE, _FAKE, 2, 3, 32, w, b, 3, None, _FAKE, _FAKE, n, None) == E            # plane < 4 x 4
    assert fwd(_FAKE, _FAKE, 2, 32, 32, w, b, 3, None, _FAKE, _FAKE, n - 1, None) == E       # scratch too small
    assert fwd(_FAKE, _FAKE, 2, 32, 32, w, b, 3, None, _FAKE, None, n, None) == E            # no scratch
    bwd = lambda *a: lib.cdl_vgg_backward(*a)                                  # noqa: E731
    assert bwd(2, 32, 32, w, b, 3, None, _FAKE, _FAKE, _FAKE, n, None) == E                  # no upstream gradient
    assert bwd(2, 32, 32, w, b, 3, _FAKE, None, None, _FAKE, n, None) == E                   # nothing to write
    assert bwd(2, 32, 32, w, b, 1, _FAKE, _FAKE, _FAKE, _FAKE, n, None) == E                 # dy not kept
    assert bwd(2, 32, 32, w, b, 3, _FAKE, _FAKE, _FAKE, _FAKE, n - 1, None) == E             # scratch too small
    assert bwd(2, 3, 32, w, b, 3, _FAKE, _FAKE, _FAKE, _FAKE, n, None) == E                  # plane < 4 x 4
    assert bwd(2, 32, 32, w, None, 3, _FAKE, _FAKE, _FAKE, _FAKE, n, None) == E              # no bias table
