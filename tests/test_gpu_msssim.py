"""cva.ms_ssim / ms_ssim_frames on the device (cdl_msssim_fwd / cdl_msssim_bwd) against the float64 restatement
(tests/msssim_restate.py).

Every gate is the rule of tests/test_gpu_ssim.py: max(1e-6, 2 x the error the same restatement makes in fp32), relative
to the float64 maximum, measured per comparison.  The restatements of a case are computed once and shared."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msssim_restate as M
from arena_util import Arena
from conftest import ROOT
from gpu_util import check, launch_sites

pytestmark = pytest.mark.gpu

W3 = [w / sum(M.WEIGHTS[:3]) for w in M.WEIGHTS[:3]]                # three levels, weights normalised
# (N, C, H, W), win, weights: odd and even axes at every level, partial tiles, more than one 16 x 64 tile per axis
CASES = [((2, 1, 177, 162), 11, None),                               # coarsest level 12 x 11: one position along W
         ((2, 2, 67, 75), 5, None),
         ((1, 1, 35, 33), 3, None),                                  # coarsest level 3 x 3: a single position
         ((3, 1, 23, 30), 3, W3),
         ((2, 1, 44, 41), 11, W3)]
IDS = ["177x162-win11", "67x75-win5", "35x33-win3", "23x30-win3-L3", "44x41-win11-L3"]


def _cva():
    import cdlnet_video_amd as cva
    return cva


def _images(shape, seed, noise=0.1):
    x = _cva().utils.synthetic_clip(shape, seed=seed)
    y = x + noise * torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 100))
    return x, y


def R_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _gate(name, got, ref64, ref32):
    return check(name, got.double(), ref64, max(1e-6, 2 * R_err(ref32, ref64)))


def _weights(w):
    return M.WEIGHTS if w is None else w


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and restatements (float64, float32) of CASES[i]: values at data_range 1, gradients at a data_range tensor
    of 1.2 with a random weight per image."""
    shape, win, weights = CASES[i]
    weights = _weights(weights)
    x, y = _images(shape, seed=sum(shape) + win)
    w = torch.rand(shape[0], generator=torch.Generator().manual_seed(5)) + 0.5
    rng = torch.tensor(1.2)
    out = {"x": x, "y": y, "w": w, "rng": rng}
    for dt, key in ((torch.float64, "64"), (torch.float32, "32")):
        tab = M.table(x.to(dt), y.to(dt), 1.0, win, 1.5, len(weights))
        v, ms = M.combine(tab, weights)
        a, b, r = (t.detach().to(dt).requires_grad_() for t in (x, y, rng))
        tab_g = M.table(a, b, r, win, 1.5, len(weights))
        v_g, ms_g = M.combine(tab_g, weights)
        (ms_g.mean(1) * w.to(dt)).sum().backward()
        out[key] = {"tab": tab, "v": v, "ms": ms.mean(1), "v_g": v_g.detach(), "dx": a.grad, "dy": b.grad, "dR": r.grad}
    return out


def _assert_off_the_kink(v):
    """On these inputs the float64 restatement keeps every level's mean at or above 0.58: the relu is inactive and every
    gradient finite.  A changed input must not move a case onto the kink silently."""
    assert float(v.min()) > 0.3, float(v.min())


def _table(x, y, rng, win, levels):
    cva = _cva()
    P = x.shape[0] * x.shape[1]
    H, W = x.shape[-2:]
    R = cva.metrics._planes_range(rng, P, x)
    return cva.metrics._MSSSIMPlanes.apply(x.reshape(P, H, W), y.reshape(P, H, W), R,
                                           cva.metrics._gaussian_window(win, 1.5), 0.01, 0.03, levels)


# --------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_values(i):
    cva = _cva()
    shape, win, weights = CASES[i]
    c = _case(i)
    _assert_off_the_kink(c["64"]["v"])
    got = cva.ms_ssim(c["x"].cuda(), c["y"].cuda(), data_range=1.0, size_average=False, win_size=win, weights=weights)
    assert got.shape == (shape[0],)
    _gate(f"ms_ssim per image {shape} win {win}", got.cpu(), c["64"]["ms"], c["32"]["ms"])
    L = len(_weights(weights))
    tab = _table(c["x"].cuda(), c["y"].cuda(), 1.0, win, L)
    assert tab.shape == (L, shape[0] * shape[1], 2)
    _gate(f"ms_ssim raw table {shape} win {win}", tab.cpu().reshape(c["64"]["tab"].shape), c["64"]["tab"], c["32"]["tab"])
    mean = cva.ms_ssim(c["x"].cuda(), c["y"].cuda(), data_range=1.0, win_size=win, weights=weights)
    assert mean.dim() == 0
    _gate(f"ms_ssim mean {shape} win {win}", mean.cpu().reshape(1), c["64"]["ms"].mean().reshape(1),
          c["32"]["ms"].mean().reshape(1))


# ------------------------------------------------------------------------------------------------ 2. gradients
@pytest.mark.parametrize("i", range(3), ids=IDS[:3])
def test_gradients(i):
    cva = _cva()
    shape, win, weights = CASES[i]
    c = _case(i)
    _assert_off_the_kink(c["64"]["v_g"])
    xd, yd, rd = (t.cuda().requires_grad_() for t in (c["x"], c["y"], c["rng"]))
    out = cva.ms_ssim(xd, yd, data_range=rd, size_average=False, win_size=win, weights=weights)
    (out * c["w"].cuda()).sum().backward()
    for name, got in (("dx", xd.grad), ("dy", yd.grad), ("dR", rd.grad)):
        assert torch.isfinite(got).all()
        _gate(f"ms_ssim {name} {shape} win {win}", got.cpu().reshape(c["64"][name].shape), c["64"][name], c["32"][name])


def test_gradient_one_side():
    """Only X requires grad: dy is not computed (three coefficient planes, no y-side pyramid) and dx keeps its bits."""
    cva = _cva()
    shape, win, weights = CASES[1]
    c = _case(1)
    xa = c["x"].cuda().requires_grad_()
    (cva.ms_ssim(xa, c["y"].cuda(), data_range=1.2, size_average=False, win_size=win) * c["w"].cuda()).sum().backward()
    _gate("ms_ssim dx alone", xa.grad.cpu(), c["64"]["dx"], c["32"]["dx"])
    xb, yb = c["x"].cuda().requires_grad_(), c["y"].cuda().requires_grad_()
    (cva.ms_ssim(xb, yb, data_range=1.2, size_average=False, win_size=win) * c["w"].cuda()).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    ya = c["y"].cuda().requires_grad_()
    (cva.ms_ssim(c["x"].cuda(), ya, data_range=1.2, size_average=False, win_size=win) * c["w"].cuda()).sum().backward()
    assert torch.equal(ya.grad, yb.grad)


# -------------------------------------------------------------------------------------------------- 3. pyramid
def _abi_forward(x, y, win_size, levels, rng=1.0, alloc=None):
    """cdl_msssim_fwd through ops._call on (P, H, W) device planes -> (vals, pyr_x, pyr_y, R)."""
    cva = _cva()
    m, lib = cva.metrics, cva._lib.lib()
    P, H, W = x.shape
    alloc = alloc or (lambda name, n: torch.empty(n, device="cuda"))
    win = m._gaussian_window(win_size, 1.5)
    n = int(lib.cdl_msssim_scratch_floats(P, H, W, win_size, levels))
    npyr = int(lib.cdl_msssim_pyramid_floats(P, H, W, levels))
    assert n > 0
    R = torch.full((P,), float(rng), device="cuda")
    scratch = torch.empty(n, device="cuda")
    px, py = (alloc("pyr_x", npyr), alloc("pyr_y", npyr)) if levels > 1 else (None, None)
    vals = alloc("vals", levels * P * 2).reshape(levels, P, 2)
    cva.ops._call("cdl_msssim_fwd", x, y, P, H, W, m._window_arg(win), win_size, 0.01, 0.03, R, levels, px, py, vals,
                  scratch, n)
    return vals, px, py, R


@pytest.mark.parametrize("i", [0, 1, 2], ids=IDS[:3])
def test_pyramid_is_avg_pool2d_bit_for_bit(i):
    """The pooled planes the forward launches write, level by level from the device's own previous level, against
    torch's avg_pool2d on the device: the kernel sums the four pixels in torch's order, so the bits agree."""
    shape, win, _ = CASES[i]
    c = _case(i)
    P, (H, W) = shape[0] * shape[1], shape[2:]
    x, y = c["x"].cuda().reshape(P, H, W), c["y"].cuda().reshape(P, H, W)
    _, px, py, _ = _abi_forward(x, y, win, 5)
    sizes = M.level_sizes(H, W, 5)
    assert px.numel() == P * sum(h * w for h, w in sizes[1:])
    for side, first, pyr in (("x", x, px), ("y", y, py)):
        prev, off = first, 0
        for lvl in range(1, 5):
            h, w = sizes[lvl]
            got = pyr[off:off + P * h * w].reshape(P, h, w)
            want = F.avg_pool2d(prev[None], 2, padding=[prev.shape[-2] % 2, prev.shape[-1] % 2])[0]
            assert want.shape == got.shape
            assert torch.equal(got, want), (side, lvl, float((got - want).abs().max()))
            prev, off = got, off + P * h * w


# ------------------------------------------------------------------------------------- 4. same kernels, same bits
def test_same_kernels_same_bits():
    cva = _cva()
    m, lib = cva.metrics, cva._lib.lib()
    shape, win_size, _ = CASES[0]
    c = _case(0)
    P, (H, W) = shape[0] * shape[1], shape[2:]
    x, y = c["x"].cuda().reshape(P, H, W), c["y"].cuda().reshape(P, H, W)
    win = m._window_arg(m._gaussian_window(win_size, 1.5))
    R = torch.full((P,), 1.2, device="cuda")
    n = int(lib.cdl_ssim_scratch_floats(P, H, W, win_size))
    scratch = torch.empty(n, device="cuda")
    s, cs = torch.empty(P, device="cuda"), torch.empty(P, device="cuda")
    cva.ops._call("cdl_ssim_fwd", x, y, P, H, W, win, win_size, 0.01, 0.03, 1.0, R, s, cs, scratch, n)
    for levels in (1, 5):
        vals, _, _, _ = _abi_forward(x, y, win_size, levels, rng=1.2)
        assert torch.equal(vals[0, :, 0], s) and torch.equal(vals[0, :, 1], cs), levels

    g = torch.rand(P, generator=torch.Generator().manual_seed(2)).cuda() + 0.5
    dx, dy, dr = torch.empty_like(x), torch.empty_like(y), torch.empty(P, device="cuda")
    cva.ops._call("cdl_ssim_bwd", x, y, P, H, W, win, win_size, 0.01, 0.03, 1.0, R, g, dx, dy, dr, scratch, n)
    gv = torch.stack([g, torch.zeros_like(g)], -1).reshape(1, P, 2).contiguous()
    n1 = int(lib.cdl_msssim_scratch_floats(P, H, W, win_size, 1))
    scratch1 = torch.empty(n1, device="cuda")
    dx1, dy1, dr1 = torch.empty_like(x), torch.empty_like(y), torch.empty(P, device="cuda")
    cva.ops._call("cdl_msssim_bwd", x, y, None, None, P, H, W, win, win_size, 0.01, 0.03, R, 1, gv, dx1, dy1, dr1, None,
                  scratch1, n1)
    assert torch.equal(dx1, dx) and torch.equal(dy1, dy) and torch.equal(dr1, dr)


# ------------------------------------------------------------------------- 5. parent bits of the existing surface
def test_ssim_surface_keeps_the_parent_commits_bits():
    """`ssim` and `ssim_frames` (values and input gradients) bit for bit against the record made on the commit before the
    SSIM kernels grew their MS-SSIM forms (tools/make_golden_ssim_parent_bits.py)."""
    spec = importlib.util.spec_from_file_location("make_golden_ssim_parent_bits",
                                                  os.path.join(ROOT, "tools", "make_golden_ssim_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = np.load(os.path.join(ROOT, "tests", "golden", "ms0_ssim_parent_bits.npz"))
    got = mod.compute()
    assert sorted(got) == sorted(want.files) and len(got) == 14
    differ = {}
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == np.float32 and a.shape == b.shape, k
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            differ[k] = float(np.abs(a - b).max())
    assert not differ, differ


# --------------------------------------------------------------------------------------------------- 6. frames
@pytest.mark.parametrize("kind", ["None", "per frame"])
def test_ms_ssim_frames(kind):
    cva = _cva()
    shape = (1, 1, 2, 177, 162)
    o, t = _images(shape, seed=21)
    r = None if kind == "None" else torch.tensor([0.9, 1.3])

    def run(dt):
        a, b = o.detach().to(dt).requires_grad_(), t.detach().to(dt).requires_grad_()      # detach: .to() may return o itself
        rr = None if r is None else r.detach().to(dt).requires_grad_()
        v = M.ms_ssim_frames(a, b, data_range=rr)
        v.backward()
        return v.detach(), a.grad, b.grad, None if rr is None else rr.grad

    r64, r32 = run(torch.float64), run(torch.float32)
    for k in range(shape[2]):
        rk = float(o[:, :, k].max() - o[:, :, k].min()) if r is None else float(r[k])
        _assert_off_the_kink(M.combine(M.table(o[:, :, k].double(), t[:, :, k].double(), rk), M.WEIGHTS)[0])
    od, td = o.cuda().requires_grad_(), t.cuda().requires_grad_()
    rd = None if r is None else r.cuda().requires_grad_()
    loss = cva.metrics.ms_ssim_frames(od, td, data_range=rd)
    loss.backward()
    _gate(f"ms_ssim_frames ({kind}) value", loss.detach().cpu().reshape(1), r64[0].reshape(1), r32[0].reshape(1))
    _gate(f"ms_ssim_frames ({kind}) d output", od.grad.cpu(), r64[1], r32[1])
    _gate(f"ms_ssim_frames ({kind}) d target", td.grad.cpu(), r64[2], r32[2])
    if rd is not None:
        _gate(f"ms_ssim_frames ({kind}) dR", rd.grad.cpu(), r64[3], r32[3])


# ------------------------------------------------------------------------------------------------- 7. clipping
def test_clipping_semantics():
    """One level, weights [1]: a single launch decides.  A negative raw mean gives 0 and an all-zero dx, as in the
    restatement.  (x, -x) does NOT get there -- luminance and cs both change sign, the raw mean is +0.97 -- so it is
    checked against the restatement as it is, and (x, 1 - x), whose raw mean is -0.95, is the clipped case."""
    cva = _cva()
    x = cva.utils.synthetic_clip((1, 1, 16, 16), seed=3)
    for name, y, clipped in (("-x", -x, False), ("1 - x", 1 - x, True)):
        a64 = x.double().requires_grad_()
        r64 = M.ms_ssim(a64, y.double(), data_range=1.0, win_size=3, weights=[1.0])
        r64.backward()
        a32 = x.clone().requires_grad_()
        r32 = M.ms_ssim(a32, y, data_range=1.0, win_size=3, weights=[1.0])
        r32.backward()
        xd = x.cuda().requires_grad_()
        got = cva.ms_ssim(xd, y.cuda(), data_range=1.0, win_size=3, weights=[1.0])
        got.backward()
        raw = _table(x.cuda(), y.cuda(), 1.0, 3, 1)[0, 0, 0]
        if clipped:
            assert float(raw) < -0.5 and float(r64) == 0.0 and not a64.grad.any()
            assert float(got) == 0.0 and not xd.grad.any()
        else:
            assert float(raw) > 0.5
            _gate(f"ms_ssim one level (x, {name})", got.detach().cpu().reshape(1), r64.detach().reshape(1),
                  r32.detach().reshape(1))
            _gate(f"ms_ssim one level (x, {name}) dx", xd.grad.cpu(), a64.grad, a32.grad)


# ---------------------------------------------------------------------------------------------- 8. determinism
def test_determinism():
    cva = _cva()
    c = _case(1)
    runs = []
    for _ in range(2):
        xd, yd, rd = (t.cuda().requires_grad_() for t in (c["x"], c["y"], c["rng"]))
        v = cva.ms_ssim(xd, yd, data_range=rd, win_size=5, size_average=False)
        v.sum().backward()
        runs.append((v.detach(), xd.grad, yd.grad, rd.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------- 9. launch trace
def _kernels(trace):
    return sorted((site, len(recs)) for site, recs in launch_sites(trace).items())


@pytest.mark.parametrize("range_grad", [False, True])
def test_launch_trace(range_grad):
    """Pooling and the gradient up-sampling ride in the existing launches: five levels are five k_ssim_fwd and five
    k_ssim_reduce forward, five k_ssim_bwd in reverse, and five more reduces only for dL/dR."""
    cva = _cva()
    c = _case(2)
    xd, yd = c["x"].cuda().requires_grad_(), c["y"].cuda().requires_grad_()
    rd = torch.tensor(1.2, device="cuda", requires_grad=range_grad)
    cva.ms_ssim(xd, yd, data_range=rd, win_size=3).backward()           # first call: allocations
    torch.cuda.synchronize()
    with cva.ops.trace() as tf:
        v = cva.ms_ssim(xd, yd, data_range=rd, win_size=3)
    assert _kernels(tf) == [("cdl_ssim.hip:k_ssim_fwd", 5), ("cdl_ssim.hip:k_ssim_reduce", 5)]
    assert [r.values()["level"] for r in tf] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    with cva.ops.trace() as tb:
        v.backward()
        torch.cuda.synchronize()
    want = [("cdl_ssim.hip:k_ssim_bwd", 5)] + ([("cdl_ssim.hip:k_ssim_reduce#2", 5)] if range_grad else [])
    assert _kernels(tb) == want
    assert [r.values()["level"] for r in tb if "k_ssim_bwd" in r.note] == [4, 3, 2, 1, 0]


# ---------------------------------------------------------------------------------------- 10. no host sync
def test_ms_ssim_frames_no_host_sync():
    cva = _cva()
    o, t = _images((1, 1, 2, 44, 41), seed=6)
    od, td = o.cuda().requires_grad_(), t.cuda()
    kw = dict(weights=W3)                                            # 44 x 41 -> 11 x 11 at level 2: three levels of win 11
    cva.metrics.ms_ssim_frames(od, td, **kw).backward()              # first call: library load, scratch allocation
    od.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                            # the hook is live: a device-to-host read is refused
            torch.ones(1, device="cuda").item()
        loss = cva.metrics.ms_ssim_frames(od, td, **kw)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert od.grad is not None and torch.isfinite(od.grad).all()


# ------------------------------------------------------------------------------- 11. guard-banded, misaligned views
def test_guard_banded_misaligned_views():
    """(1, 1, 35, 33), win 3, five levels: `ms_ssim` on 4-byte aligned views of x and y, and the entry points with
    every caller buffer (pyr_*, vals, work, dx, dy, d_range) carved at element offset 1: the bits of the aligned calls,
    every output element written, no guard word touched."""
    cva = _cva()
    m, lib = cva.metrics, cva._lib.lib()
    shape, win_size, _ = CASES[2]
    c = _case(2)
    P, (H, W) = 1, shape[2:]
    xa, ya, ra = (t.cuda().requires_grad_() for t in (c["x"], c["y"], c["rng"]))
    va = cva.ms_ssim(xa, ya, data_range=ra, win_size=win_size)
    va.backward()

    A = Arena("cuda")
    xv, yv = A.put(c["x"], 1, "x"), A.put(c["y"], 1, "y")
    assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 4
    xg, yg, rg = xv.detach().requires_grad_(), yv.detach().requires_grad_(), c["rng"].cuda().requires_grad_()
    vg = cva.ms_ssim(xg, yg, data_range=rg, win_size=win_size)
    vg.backward()
    torch.cuda.synchronize()
    A.check()
    assert torch.equal(vg.detach(), va.detach())
    assert torch.equal(xg.grad, xa.grad) and torch.equal(yg.grad, ya.grad) and torch.equal(rg.grad, ra.grad)

    # the entry points themselves, every caller buffer misaligned
    B = Arena("cuda")
    xp, yp = B.put(c["x"].reshape(P, H, W), 1, "x"), B.put(c["y"].reshape(P, H, W), 1, "y")
    vals, px, py, R = _abi_forward(xp, yp, win_size, 5, rng=1.2, alloc=lambda name, n: B.out((n,), 1, name=name))
    ref_vals, ref_px, ref_py, _ = _abi_forward(c["x"].cuda().reshape(P, H, W), c["y"].cuda().reshape(P, H, W), win_size, 5,
                                               rng=1.2)
    g = torch.rand(5, P, 2, generator=torch.Generator().manual_seed(4)) + 0.5
    n = int(lib.cdl_msssim_scratch_floats(P, H, W, win_size, 5))
    win = m._window_arg(m._gaussian_window(win_size, 1.5))

    def bwd(x_, y_, px_, py_, g_, alloc):
        dx, dy, dr = alloc("dx", (P, H, W)), alloc("dy", (P, H, W)), alloc("dr", (P,))
        work = alloc("work", (2 * px_.numel(),))
        cva.ops._call("cdl_msssim_bwd", x_, y_, px_, py_, P, H, W, win, win_size, 0.01, 0.03, R, 5, g_, dx, dy, dr, work,
                      torch.empty(n, device="cuda"), n)
        return dx, dy, dr, work

    got = bwd(xp, yp, px, py, B.put(g, 1, "g_vals"), lambda name, s: B.out(s, 1, name=name))
    ref = bwd(c["x"].cuda().reshape(P, H, W), c["y"].cuda().reshape(P, H, W), ref_px, ref_py, g.cuda(),
              lambda name, s: torch.empty(s, device="cuda"))
    torch.cuda.synchronize()
    B.check()
    for t in (vals, px, py) + got:
        B.assert_defined(t)
    for a, b in zip((vals, px, py) + got, (ref_vals, ref_px, ref_py) + ref):
        assert torch.equal(a, b)
